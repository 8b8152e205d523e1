"""Every host-side weight layout (csrc/weight_pack.cpp) on the CPU: tests/weight_pack_main.cpp is built with g++ twice (-O2, and
-O1 with the address and undefined-behaviour sanitizers), every case runs through both, and the bytes must equal the digests of
tests/golden/weight_pack_digests.json - recorded from the packers as they stood before they were rewritten on the shared walker
(their loops moved verbatim out of the host runtime (now net_build.hip) / kernels_conv2d_x3.hip / kernels_conv_taps.hip), so the byte order the kernels
read is pinned.  Besides the digests: the output length is the layout's size function, restated here (where a packer fills a
caller's buffer the driver pre-fills it with 0xa5: the packer must write all of it), and for two layouts the place of every
element is restated in numpy from the layout comment, all else being zero."""

import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import helpers

CSRC = os.path.join(helpers.REPO, "asv-subtools_amd", "csrc")
DIGESTS = os.path.join(helpers.REPO, "tests", "golden", "weight_pack_digests.json")
ET_F32, ET_BF16, ET_F16 = 0, 1, 2
PLAIN, FRAGS, X3P, MX8, CONV2D, UTTS, CONV2D_X3, CONV_TAPS, FOLD, RES2 = range(10)
ESIZE = {ET_F32: 4, ET_BF16: 2, ET_F16: 2}
BF16_TIE = np.array([0x3F808000], dtype=np.uint32).view(np.float32)[0]      # halfway between bf16 1.0 and the next: ties to even


def weights(seed, n, stride):
    """The first values, and once more the values of the first tap of input channels 0 .. 6 (every `stride`-th: the dense weight is
    [out][in][stride], and every case takes tap 0), are the edge cases."""
    w = (np.random.RandomState(seed).standard_normal(n).astype(np.float32) * np.float32(0.1)).astype(np.float32)
    w[:7] = w[:7 * stride:stride] = np.array([0.0, -0.0, 3.0, 1e-6, -2.5e-7, BF16_TIE, -BF16_TIE], dtype=np.float32)
    assert np.isfinite(w).all() and np.abs(w).max() == 3.0
    return w


def case(layout, out_ch, in_ch, taps, cout_pad, cin_pad, et, scaled=0, aux0=0, aux1=0, tot_ctx=None, left_ctx=None, seed=0, n_floats=None):
    left_ctx = taps[0] if left_ctx is None else left_ctx
    tot_ctx = taps[-1] - taps[0] + 1 if tot_ctx is None else tot_ctx
    return dict(layout=layout, out_ch=out_ch, in_ch=in_ch, taps=list(taps), cout_pad=cout_pad, cin_pad=cin_pad, et=et, scaled=scaled, aux0=aux0, aux1=aux1,
                tot_ctx=tot_ctx, left_ctx=left_ctx, seed=seed, n_floats=out_ch * in_ch * tot_ctx if n_floats is None else n_floats)


T3 = (-2, 0, 2)                       # of a dense 5-tap weight, left context -2
T9, T17 = tuple(range(9)), tuple(range(17))
CASES = {
    "plain_f32": case(PLAIN, 40, 24, T3, 256, 32, ET_F32, seed=1),
    "plain_bf16": case(PLAIN, 40, 24, T3, 256, 32, ET_BF16, seed=2),
    "plain_f16": case(PLAIN, 40, 24, T3, 256, 32, ET_F16, seed=3),
    "frags_bf16": case(FRAGS, 72, 80, T3, 256, 80, ET_BF16, seed=4),
    "frags_f16_lo_scaled": case(FRAGS, 72, 80, T3, 256, 80, ET_F16, scaled=1, aux0=1, seed=5),
    "frags_bf16_lo": case(FRAGS, 72, 80, T3, 256, 80, ET_BF16, aux0=1, seed=6),
    "x3p_f16_scaled": case(X3P, 40, 64, (0, 1), 256, 64, ET_F16, scaled=1, seed=7),
    "mx8_1tap_scaled": case(MX8, 64, 48, (0,), 256, 48, ET_F16, scaled=1, seed=8),
    "mx8_3tap_scaled": case(MX8, 64, 48, T3, 256, 48, ET_F16, scaled=1, seed=9),
    "conv2d_32_bf16": case(CONV2D, 32, 32, T9, 32, 32, ET_BF16, seed=10),
    "conv2d_s2d_f16": case(CONV2D, 64, 128, (0, 1, 2, 3), 64, 128, ET_F16, seed=11),
    "utts_split": case(UTTS, 40, 50, (0,), 256, 64, ET_BF16, seed=12),
    "conv2d_x3_32_64_f16_scaled": case(CONV2D_X3, 64, 32, T9, 64, 32, ET_F16, scaled=1, seed=13),
    "conv2d_x3_64_128_bf16": case(CONV2D_X3, 128, 64, T9, 128, 64, ET_BF16, seed=14),
    "conv_taps_f32": case(CONV_TAPS, 40, 20, T17, 64, 32, ET_F32, aux0=2, seed=15),
    "conv_taps_bf16": case(CONV_TAPS, 40, 20, T17, 64, 32, ET_BF16, aux0=2, seed=16),
    "conv_taps_f16": case(CONV_TAPS, 40, 20, T17, 64, 32, ET_F16, aux0=2, seed=17),
    "fold": case(FOLD, 40, 48, (0,), 256, 48, ET_F32, seed=18, n_floats=40 * 48 + 40 + 2 * 48),
    "res2_bf16": case(RES2, 64, 64, T3, 64, 64, ET_BF16, aux0=2, aux1=2, seed=19, n_floats=2 * 64 * 64 * 5),
}


def expected_len(c):
    """The layouts' size functions, restated (bytes)."""
    nt, cop, cip, es = len(c["taps"]), c["cout_pad"], c["cin_pad"], ESIZE[c["et"]]
    rup = lambda x, m: (x + m - 1) // m * m
    return {
        PLAIN: lambda: cop * nt * cip * es,
        FRAGS: lambda: cop * nt * rup(cip, 64) * 2 * (2 if c["aux0"] else 1),
        X3P: lambda: cop * nt * (cip // 32) * 64 * 2,
        MX8: lambda: 2 * (cop // 32) * nt * ((cip + 31) // 32) * 1024,
        CONV2D: lambda: nt * (cip // 16) * ((c["out_ch"] + 31) // 32) * 512 * 2,
        UTTS: lambda: 2 * (cop // 32) * ((cip + 31) // 32) * 1024 * 2,
        CONV2D_X3: lambda: (cip // 32) * nt * 2 * (cop // 32) * 2 * 512 * 2,
        CONV_TAPS: lambda: rup(cip, 128 // es) // (128 // es) * nt * 4 * c["aux0"] * 1024,
        FOLD: lambda: (c["out_ch"] * c["in_ch"] + c["out_ch"]) * 4,
        RES2: lambda: c["aux0"] * 64 * 3 * 64 * 2,
    }[c["layout"]]()


@pytest.fixture(scope="module")
def binaries(tmp_path_factory):
    d = tmp_path_factory.mktemp("weight_pack")
    srcs = [os.path.join(helpers.REPO, "tests", "weight_pack_main.cpp"), os.path.join(CSRC, "weight_pack.cpp")]
    common = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC]
    o2, san = str(d / "wp_o2"), str(d / "wp_san")
    subprocess.check_call(common + ["-O2"] + srcs + ["-o", o2])
    subprocess.check_call(common + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + srcs + ["-o", san])
    return o2, san


_results = {}


def run_case(binaries, name):
    """(w_scale, packed bytes, the float data) of a case: through both binaries, which must agree; computed once."""
    if name not in _results:
        c = CASES[name]
        data = weights(c["seed"], c["n_floats"], c["tot_ctx"])
        if c["layout"] == FOLD:                           # scale around 1 as a BatchNorm's; bias and shift of either sign
            data[c["out_ch"] * c["in_ch"] + c["out_ch"]:][:c["in_ch"]] += np.float32(1.0)
        head = [c["layout"], c["out_ch"], c["in_ch"], c["tot_ctx"], c["left_ctx"], len(c["taps"]), c["cout_pad"], c["cin_pad"], c["et"], c["scaled"], c["aux0"], c["aux1"]]
        blob = struct.pack("<%di" % (len(head) + len(c["taps"]) + 1), *(head + c["taps"] + [data.size])) + data.tobytes()
        outs = []
        for exe in binaries:
            p = subprocess.run([exe], input=blob, capture_output=True)
            assert p.returncode == 0, (name, exe, p.returncode, p.stderr.decode()[-2000:])
            assert p.stderr == b"", (name, exe, p.stderr.decode()[-2000:])
            outs.append(p.stdout)
        assert outs[0] == outs[1], "%s: the -O2 and the sanitizer build disagree" % name
        _results[name] = (np.frombuffer(outs[0][:4], dtype=np.float32)[0], outs[0][4:], data)
    return _results[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_packed_bytes_match_the_recorded_digests(binaries, name):
    w_scale, packed, data = run_case(binaries, name)
    c = CASES[name]
    assert len(packed) == expected_len(c)
    if c["scaled"]:
        assert w_scale == np.float32(2.0 ** 12)           # the largest weight is 3.0 = 0.75 * 2^2: 2^(14 - 2)
    else:
        assert w_scale == np.float32(1.0)
    with open(DIGESTS) as f:
        want = json.load(f)
    assert hashlib.sha256(struct.pack("<f", w_scale) + packed).hexdigest() == want[name]


def test_digest_file_lists_exactly_the_cases():
    with open(DIGESTS) as f:
        assert sorted(json.load(f)) == sorted(CASES)


def _frags_index(c, co, t, ci):
    """[n_frag32][tap][chunk64][k_group16][lane][8]; lane = (k half lh, channel lr): channel n_frag*32 + lr, k = chunk*64 + k_group*16 + lh*8 + e."""
    nt, nchunks = len(c["taps"]), (c["cin_pad"] + 63) // 64
    nf, lr = divmod(co, 32)
    chunk, k = divmod(ci, 64)
    kg, k = divmod(k, 16)
    lh, e = divmod(k, 8)
    return ((((nf * nt + t) * nchunks + chunk) * 4 + kg) * 64 + lh * 32 + lr) * 8 + e


def _conv_taps_index(c, co, t, ci):
    """[chunk][tap][slot pair q][32-channel fragment n][lane = (slot half lh, channel lr)][16 bytes]: input channels
    chunk * (32 | 64) + (2 q + lh) * (4 | 8) + e of output channel n * 32 + lr."""
    per = 16 // ESIZE[c["et"]]
    nt, nf_total = len(c["taps"]), c["aux0"]
    chunk, k = divmod(ci, per * 8)
    slot, e = divmod(k, per)
    q, lh = divmod(slot, 2)
    n, lr = divmod(co, 32)
    return ((((chunk * nt + t) * 4 + q) * nf_total + n) * 64 + lh * 32 + lr) * per + e


@pytest.mark.parametrize("name", ["frags_bf16", "frags_f16_lo_scaled", "frags_bf16_lo", "conv_taps_f32", "conv_taps_bf16", "conv_taps_f16"])
def test_elements_land_where_the_layout_comment_says(binaries, name):
    """An independent restatement of the two layout comments: element index(co, t, ci) holds the converted weight, all else is zero."""
    w_scale, packed, data = run_case(binaries, name)
    c = CASES[name]
    index = _frags_index if c["layout"] == FRAGS else _conv_taps_index
    w = data.reshape(c["out_ch"], c["in_ch"], c["tot_ctx"])
    dtype = np.float32 if c["et"] == ET_F32 else np.uint16
    got = np.frombuffer(packed, dtype=dtype)
    if c["layout"] == FRAGS and c["aux0"]:
        got = got[:got.size // 2]                         # the hi halves; the lo halves share their indices
    want = np.zeros(got.size, dtype=np.float32)
    seen = set()
    for co in range(c["out_ch"]):
        for t, tap in enumerate(c["taps"]):
            for ci in range(c["in_ch"]):
                i = index(c, co, t, ci)
                assert i not in seen
                seen.add(i)
                want[i] = w[co, ci, tap - c["left_ctx"]] * w_scale
    assert len(seen) == c["out_ch"] * c["in_ch"] * len(c["taps"])
    if c["et"] == ET_F32:
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    elif c["et"] == ET_F16:
        assert np.array_equal(got, want.astype(np.float16).view(np.uint16))
    else:
        u = want.view(np.uint32).astype(np.uint64)
        assert np.array_equal(got, ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16))
    if c["layout"] == FRAGS and c["aux0"]:                # lo halves: nothing outside the reachable set
        lo = np.frombuffer(packed, dtype=np.uint16)[got.size:]
        assert set(np.flatnonzero(lo).tolist()) <= seen


def test_res2_helper_is_the_concatenation_of_its_branches(binaries):
    """pack_res2_branch_frags == one `frags` pack per branch (width x width, taps {-d, 0, d}), one after the other."""
    _, packed, data = run_case(binaries, "res2_bf16")
    c = CASES["res2_bf16"]
    per = data.size // c["aux0"]
    parts = []
    for b in range(c["aux0"]):
        one = dict(c, layout=FRAGS, aux0=0, aux1=0, n_floats=per)
        head = [one["layout"], 64, 64, 5, -2, 3, 64, 64, ET_BF16, 0, 0, 0]
        blob = struct.pack("<%di" % (len(head) + 4), *(head + [-2, 0, 2, per])) + data[b * per:(b + 1) * per].tobytes()
        p = subprocess.run([binaries[0]], input=blob, capture_output=True, check=True)
        parts.append(p.stdout[4:])
    assert packed == b"".join(parts)
