"""The per-batch planner (csrc/batch_plan.cpp) on the CPU: tests/batch_plan_main.cpp is built with g++ twice (-O2, and -O1 with the
address and undefined-behaviour sanitizers), every case runs through both, and every field of the BatchPlan must equal its restatement
in numpy here: the chunk rule of the reference's `for_extract_embedding` (framework.py:34-47: num_split = ceil(T / maxChunk) chunks of
T // num_split frames, the last one taking the rest), the row layout of DESIGN.md "Data layout in HBM" (gap rows before, between and
behind the segments, the total padded to 256 rows; a grid segment owns frames x pitch rows, its frames halved per stride-2 stage), and
conv_cases.row_layout(), the layout the convolution tests build their inputs on, for the grids it can express (pitch = width + 1)."""

import os
import subprocess

import numpy as np
import pytest

import conv_cases
import helpers

CSRC = os.path.join(helpers.REPO, "asv-subtools_amd", "csrc")
FRAMES, UTTS, GRID = 0, 1, 2
HALO, ROW_TILE = 4, 256
ASV_EINVAL = -22                      # include/asv_amd.h


def dom(kind, shift=0, width=1, pitch=1, reach=1, valid=0):
    return dict(kind=kind, shift=shift, width=width, pitch=pitch, reach=reach, valid=valid)


# domains 0 and 1 are the frames and the utts domain of every net
PADDED = [dom(FRAMES), dom(UTTS), dom(GRID, 0, 80, 81), dom(GRID, 2, 20, 21), dom(GRID, 0, 30, 32, reach=2), dom(GRID, 2, 1, 1)]
UNPADDED = [dom(FRAMES), dom(UTTS), dom(GRID, 1, 39, 40, valid=1)]
LENGTHS = [1, 7, 200, 201, 10000, 10001, 25000]
LENGTHS_UNPADDED = [3] + LENGTHS[1:]          # the unpadded front needs 3 frames: its shortest chunk
MAX_CHUNKS = [0, 100, 10000]


@pytest.fixture(scope="module")
def binaries(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch_plan")
    srcs = [os.path.join(helpers.REPO, "tests", "batch_plan_main.cpp"), os.path.join(CSRC, "batch_plan.cpp")]
    common = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC]
    o2, san = str(d / "bp_o2"), str(d / "bp_san")
    subprocess.check_call(common + ["-O2"] + srcs + ["-o", o2])
    subprocess.check_call(common + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + srcs + ["-o", san])
    return o2, san


def run_plan(binaries, domains, offsets, max_chunk, block_rows=0):
    """The driver's output as {name: [ints]} (or {'rc': ..., 'error': message}): through both binaries, which must agree."""
    text = "%d\n" % len(domains) + "".join("%(kind)d %(shift)d %(width)d %(pitch)d %(reach)d %(valid)d\n" % d for d in domains)
    text += "%d %d\n%s\n%d\n" % (max_chunk, len(offsets) - 1, " ".join(str(int(o)) for o in offsets), block_rows)
    outs = []
    for exe in binaries:
        p = subprocess.run([exe], input=text.encode(), capture_output=True)
        assert p.returncode == 0, (exe, p.returncode, p.stderr.decode()[-2000:])
        assert p.stderr == b"", (exe, p.stderr.decode()[-2000:])
        outs.append(p.stdout.decode())
    assert outs[0] == outs[1], "the -O2 and the sanitizer build disagree"
    got = {}
    for line in outs[0].splitlines():
        if line.startswith("rc "):
            got["rc"] = int(line[3:])
        elif line.startswith("error "):
            got["error"] = line[6:]
        else:
            name, _, vals = line.partition(":")
            got[name] = [int(v) for v in vals.split()]
    return got


def chunks(T, max_chunk):
    """framework.py:34-47."""
    max_chunk = 10000 if max_chunk <= 0 else max_chunk
    num_split = (T + max_chunk - 1) // max_chunk
    split = T // num_split
    return [split] * (num_split - 1) + [T - (num_split - 1) * split]


def expected_plan(domains, lengths, max_chunk):
    want = {"rc": 0, "n_utts": [len(lengths)], "frames": [sum(lengths)], "seg_src0": [], "seg_frames": [], "utt_seg0": [], "utt_nseg": [], "n_dom": [len(domains)]}
    src = 0
    for T in lengths:
        parts = chunks(T, max_chunk)
        want["utt_seg0"].append(len(want["seg_frames"]))
        want["utt_nseg"].append(len(parts))
        want["seg_src0"] += list(src + np.concatenate([[0], np.cumsum(parts[:-1])]).astype(int))
        want["seg_frames"] += parts
        src += T
    S = len(want["seg_frames"])
    want["segments"], want["seg_pad"] = [S], [-(-S // ROW_TILE) * ROW_TILE]
    for i, d in enumerate(domains):
        if d["kind"] == UTTS:                 # one row per segment; one pseudo segment covers the valid rows
            rows, row0, lens = S, [0], [S]
        else:
            frames = list(want["seg_frames"])
            for _ in range(d["shift"]):       # a stride-2 stage: ceil(n / 2) frames, an unpadded one of kernel 3 (n - 1) // 2
                frames = [(n - 1) // 2 if d["valid"] else (n + 1) // 2 for n in frames]
            gap = HALO if d["kind"] == FRAMES else (2 * d["pitch"] + 3 if d["reach"] == 2 else d["pitch"] + 2)
            lens = [n * d["pitch"] for n in frames]
            row0 = list(gap + np.concatenate([[0], np.cumsum([n + gap for n in lens[:-1]])]).astype(int))
            rows = row0[-1] + lens[-1] + gap
            if d["kind"] == GRID and d["reach"] == 1 and (d["pitch"] == d["width"] + 1 or d["pitch"] == 1):
                F = d["pitch"] - 1                # conv_cases.row_layout: pitch F + 1, gaps of F + 3 rows
                assert conv_cases.row_layout(frames, F) == (row0, lens, -(-rows // ROW_TILE) * ROW_TILE)
        want["dom %d rows" % i], want["dom %d rows_pad" % i] = [rows], [-(-rows // ROW_TILE) * ROW_TILE]
        want["dom %d seg_row0" % i], want["dom %d seg_len" % i] = [int(r) for r in row0], lens
    want["seg_src0"] = [int(v) for v in want["seg_src0"]]
    return want


@pytest.mark.parametrize("max_chunk", MAX_CHUNKS)
@pytest.mark.parametrize("name", ["padded", "unpadded"])
def test_plan_matches_the_chunk_rule_and_the_row_layout(binaries, name, max_chunk):
    domains, lengths = (PADDED, LENGTHS) if name == "padded" else (UNPADDED, LENGTHS_UNPADDED)
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    got = run_plan(binaries, domains, offsets, max_chunk)
    want = expected_plan(domains, lengths, max_chunk)
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key
    if name == "unpadded":
        assert min(got["seg_frames"]) == 3


def test_chunk_rule_cases():
    """The restated rule itself, on the lengths around the chunk limit."""
    assert chunks(10000, 0) == [10000] and chunks(10001, 0) == [5000, 5001] and chunks(25000, 10000) == [8333, 8333, 8334]
    assert chunks(201, 100) == [67, 67, 67] and chunks(200, 100) == [100, 100] and chunks(7, 100) == [7] and chunks(1, 100) == [1]


REJECTIONS = {
    "offsets0": (PADDED, [1, 8], 0, "extract: offsets[0] must be 0"),
    "empty": (PADDED, [0, 5, 5, 9], 0, "extract: utterance 1 has 0 frames (the reference asserts T >= tot_context, components.py:119)"),
    "short_unpadded": (UNPADDED, [0, 7, 9], 0,
                       "extract: a chunk of 2 frames is too short for the unpadded subsampling front (1 stride-2 stages of kernel 3: at least 3 frames)"),
    # the 2^30-row limit: one chunk of 2^30 frames + its two gaps (no table grows with the frame count, so nothing large is allocated)
    "too_large": (PADDED, [0, 1 << 30], 1 << 30, "extract: batch too large (%d rows in domain 0)" % ((1 << 30) + 2 * HALO)),
}


@pytest.mark.parametrize("name", sorted(REJECTIONS))
def test_rejections_carry_their_messages(binaries, name):
    domains, offsets, max_chunk, message = REJECTIONS[name]
    got = run_plan(binaries, domains, offsets, max_chunk)
    assert got == {"rc": ASV_EINVAL, "error": message}


def blocks_restated(row0, lens, block_rows):
    """The most segments with a row in any one block of block_rows rows."""
    count = {}
    for a, n in zip(row0, lens):
        for b in range(a // block_rows, (a + n - 1) // block_rows + 1):
            count[b] = count.get(b, 0) + 1
    return count


@pytest.mark.parametrize("n_utts,T,most", [(40, 5, 14), (40, 3, 18), (1, 300, 1)])
def test_max_segments_per_block(binaries, n_utts, T, most):
    """128-row blocks of the frames plan.  40 utterances of 5 frames own 9 rows each with their gap: every full block holds 14 of them,
    still within the 16 slots of the fused pooling; 40 of 3 frames (7 rows each) put 18 into every block they fill, the crowd of tiny
    utterances that turns the fused pooling off; one utterance of 300 frames lies in three blocks, one segment each."""
    offsets = np.arange(n_utts + 1) * T
    got = run_plan(binaries, PADDED, offsets, 0, block_rows=128)
    count = blocks_restated(got["dom 0 seg_row0"], got["dom 0 seg_len"], 128)
    assert got["max_segments_per_block"] == [max(count.values())] == [most]
    if n_utts == 1:
        assert sorted(count) == [0, 1, 2]
    else:
        full = [b for b in count if (b + 1) * 128 <= got["dom 0 rows"][0]]
        assert full and all((count[b] > 16) == (T == 3) for b in full)
