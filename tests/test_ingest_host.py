"""Host side of the device ingest (sliding CMN + voiced-frame selection inside extraction): the C ABI declaration, the script's
options, and the VAD table logic of pipeline/onestep/extract_embeddings.py - no GPU: the device side is a stand-in that records what
it is handed (in the style of the gloo tests' stand-in extractors)."""

import importlib.util
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_script():
    spec = importlib.util.spec_from_file_location("extract_embeddings_ingest", os.path.join(REPO, "asv-subtools_amd", "pytorch", "pipeline", "onestep",
                                                                                            "extract_embeddings.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_entry_point_is_declared_and_listed():
    from libs.amd import capi
    hdr = open(os.path.join(REPO, "include", "asv_amd.h")).read()
    assert re.search(r"\bint\s+asv_ingest_frames\s*\(", hdr)
    assert "asv_ingest_frames" in capi.SYMBOLS
    lib = capi.lib()
    assert len(lib.asv_ingest_frames.argtypes) == 12
    # argument errors are the library's: a negative code and a message, no device needed to get that far
    off = (np.array([0, 4], dtype=np.int64)).ctypes.data_as(lib.asv_ingest_frames.argtypes[2])
    assert lib.asv_ingest_frames(None, None, off, off, 1, 30, 0, 100, 1, 0, None, None) < 0
    assert b"asv_ingest_frames" in lib.asv_last_error()


def test_options_and_defaults():
    ee = load_script()
    a = ee.get_args(["model", "scp:feats.scp", "ark:out.ark"])
    assert (a.cmn_window, a.cmn_center, a.cmn_norm_vars, a.cmn_min_window, a.vad_scp) == (0, "true", "false", 100, "")
    assert ee.ingest_options(a) is None                                 # nothing asked for: the plain path, no ingest
    a = ee.get_args(["--cmn-window", "300", "--cmn-center", "false", "--cmn-norm-vars", "true", "--cmn-min-window", "50", "--vad-scp", "vad.scp",
                     "model", "scp:feats.scp", "ark:out.ark"])
    o = ee.ingest_options(a)
    assert (o.cmn_window, o.min_window, o.center, o.norm_vars, o.flags) == (300, 50, False, True, True)
    o = ee.ingest_options(ee.get_args(["--cmn-window", "300", "model", "scp:feats.scp", "ark:out.ark"]))
    assert (o.cmn_window, o.min_window, o.center, o.norm_vars, o.flags) == (300, 100, True, False, False)   # the reference shell script's
    o = ee.ingest_options(ee.get_args(["--vad-scp", "vad.scp", "model", "scp:feats.scp", "ark:out.ark"]))
    assert o.cmn_window == 0 and o.flags
    with pytest.raises(ValueError):
        ee.ingest_options(ee.get_args(["--cmn-window", "300", "--cmn-center", "false", "--cmn-min-window", "0", "model", "scp:f.scp", "ark:o.ark"]))


def test_sharded_with_vad_scp_is_rejected():
    ee = load_script()
    a = ee.get_args(["--sharded", "true", "--vad-scp", "x", "model", "scp:feats.scp", "ark:out.ark"])
    with pytest.raises(ValueError) as e:
        ee.ingest_options(a)
    assert "--sharded" in str(e.value) and "--vad-scp" in str(e.value)
    # sliding CMN alone is available on the sharded path
    assert ee.ingest_options(ee.get_args(["--sharded", "true", "--cmn-window", "300", "model", "scp:feats.scp", "ark:out.ark"])).cmn_window == 300


# ----------------------------------------------------------------------------------------------------------------------------------
KEYS = ["utt%02d" % i for i in range(12)]
LENS = [57, 40, 700, 1, 123, 64, 300, 41, 88, 250, 65, 99]
MISSING, MISMATCH, SILENT = 3, 7, 9                                       # no entry / wrong length / all zero
TEXT = (1, 5, 8)                                                          # written as text vectors, the others binary


def write_vad(tmp_path, poison=None):
    """vad.ark / vad.scp of the 12 keys (shuffled order in the scp: a table is looked up by key).  Returns the flags per key."""
    from libs.support import kaldi_io
    rng = np.random.RandomState(5)
    flags = {}
    ark, scp = tmp_path / "vad.ark", tmp_path / "vad.scp"
    lines = []
    with open(ark, "wb") as f:
        for i, (key, T) in enumerate(zip(KEYS, LENS)):
            v = (rng.rand(T) < 0.6).astype(np.float32)
            if i == SILENT:
                v[:] = 0.0
            if i == 0:
                v[:] = 1.0
            if i == MISMATCH:
                v = v[:-3]
            if poison == i:
                v[T // 2] = 0.5
            flags[key] = v
            if i == MISSING:
                continue
            if i in TEXT:
                path = tmp_path / ("%s.vad.txt" % key)
                path.write_text(" [ " + " ".join("%d" % x if poison != i else "%g" % x for x in v) + " ]\n")
                lines.append("%s %s\n" % (key, path))
                continue
            f.write((key + " ").encode())
            lines.append("%s %s:%d\n" % (key, ark, f.tell()))
            kaldi_io.write_vec_flt(f, v)
    with open(scp, "w") as s:
        for line in lines[::-1]:
            s.write(line)
    return scp, flags


class StandInSets(object):
    """What extract_stream's reader thread and consumer use of libs.amd.pipeline.DeviceSets, recording every submission."""

    def __init__(self, frames):
        self.flags = np.full(frames, 7, dtype=np.uint8)                    # (stale contents: the table has to overwrite them)
        self.calls = []

    def flag_buffer(self, k):
        return self.flags

    def submit(self, k, offsets, frames, voiced=None, kept_off=None):
        self.calls.append((np.array(offsets), frames, voiced.copy(), np.array(kept_off)))


def numpy_restatement(flags):
    """select-voiced-frames' rules over the 12 utterances: (flag bytes, kept counts, kept keys)."""
    out, counts = [], []
    for i, (key, T) in enumerate(zip(KEYS, LENS)):
        ok = i != MISSING and flags[key].shape[0] == T
        out.append((flags[key] != 0).astype(np.uint8) if ok else np.zeros(T, dtype=np.uint8))
        counts.append(int(out[-1].sum()))
    return np.concatenate(out), np.array(counts), [k for k, c in zip(KEYS, counts) if c > 0]


@pytest.mark.parametrize("group", [12, 5])
def test_vad_table_flags_counts_and_skips(tmp_path, group):
    ee = load_script()
    scp, flags = write_vad(tmp_path)
    warned = []
    table = ee.VadTable("scp:%s" % scp, threads=2, warn=warned.append)
    want_flags, want_counts, want_keys = numpy_restatement(flags)
    sets = StandInSets(sum(LENS))
    got_keys, at = [], 0
    for a in range(0, 12, group):                                          # the batches of a stream: one group, or three
        keys, lens = KEYS[a:a + group], LENS[a:a + group]
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        buf = sets.flag_buffer(0)[:int(offsets[-1])]
        kept, kept_off = table.flags_for(keys, offsets, buf)
        sets.submit(0, offsets, int(offsets[-1]), voiced=buf, kept_off=kept_off)
        got_keys += kept
        _, _, sent, sent_off = sets.calls[-1]
        n = int(offsets[-1])
        assert sent.dtype == np.uint8 and np.array_equal(sent, want_flags[at:at + n])
        assert np.array_equal(np.diff(sent_off), want_counts[a:a + group]) and sent_off[0] == 0 and sent_off.dtype == np.int64
        # the compacted offsets the engine is handed: utterances without a kept frame are gone
        from libs.amd.frontend import kept_offsets
        counts, off2 = kept_offsets(sent, offsets)
        assert np.array_equal(off2, sent_off) and np.array_equal(counts, want_counts[a:a + group])
        at += n
    table.close()
    assert got_keys == want_keys and len(want_keys) == 9
    assert table.skipped == 3 and len(warned) == 3
    for i, cause in ((MISSING, "no VAD entry"), (MISMATCH, "entries"), (SILENT, "no voiced frame")):
        line = [w for w in warned if KEYS[i] in w]
        assert len(line) == 1 and line[0].startswith("WARNING: ") and cause in line[0], warned
        assert "Error" not in line[0] and "ERROR" not in line[0]


def test_vad_table_warns_on_stderr_by_default(tmp_path, capsys):
    ee = load_script()
    scp, _ = write_vad(tmp_path)
    table = ee.VadTable(str(scp))
    offsets = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
    table.flags_for(KEYS, offsets, np.zeros(sum(LENS), dtype=np.uint8))
    table.close()
    cap = capsys.readouterr()
    lines = [l for l in cap.err.splitlines() if l.startswith("WARNING: ")]
    assert len(lines) == 3 and "Error" not in cap.err and "ERROR" not in cap.err and "WARNING" not in cap.out


@pytest.mark.parametrize("poison", [4, 5])                                 # a binary entry (the batched reads), a text entry (read_vec_flt)
def test_vad_flag_that_is_not_0_or_1_raises(tmp_path, poison):
    ee = load_script()
    scp, _ = write_vad(tmp_path, poison=poison)
    table = ee.VadTable(str(scp), warn=lambda line: None)
    offsets = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
    with pytest.raises(ValueError) as e:
        table.flags_for(KEYS, offsets, np.zeros(sum(LENS), dtype=np.uint8))
    table.close()
    assert KEYS[poison] in str(e.value) and "0.5" in str(e.value)


def test_short_vector_at_the_end_of_the_archive(tmp_path):
    """A vector shorter than its matrix as the LAST entry of its file: the positioned read of 10 + 4 T bytes runs into the end of the
    file - that is a length mismatch of one utterance, not a failed run."""
    from libs.support import kaldi_io
    ee = load_script()
    ark, scp = tmp_path / "v.ark", tmp_path / "v.scp"
    with open(ark, "wb") as f, open(scp, "w") as s:
        for key, v in (("a", np.ones(30, dtype=np.float32)), ("b", np.ones(10, dtype=np.float32))):
            f.write((key + " ").encode())
            s.write("%s %s:%d\n" % (key, ark, f.tell()))
            kaldi_io.write_vec_flt(f, v)
    warned = []
    table = ee.VadTable(str(scp), warn=warned.append)
    flags = np.zeros(60, dtype=np.uint8)
    kept, kept_off = table.flags_for(["a", "b"], np.array([0, 30, 60], dtype=np.int32), flags)
    table.close()
    assert kept == ["a"] and kept_off.tolist() == [0, 30, 30] and flags[:30].all() and not flags[30:].any()
    assert len(warned) == 1 and "b" in warned[0] and "10 entries" in warned[0]


def test_kept_offsets_restatement():
    from libs.amd.frontend import kept_offsets
    rng = np.random.RandomState(1)
    lens = [5, 0, 9, 1, 0, 64]
    off = np.concatenate([[0], np.cumsum(lens)])
    flags = (rng.rand(off[-1]) < 0.5).astype(np.uint8) * 3                 # any non-zero byte keeps its frame
    counts, kept_off = kept_offsets(flags, off)
    assert counts.tolist() == [int((flags[a:b] != 0).sum()) for a, b in zip(off[:-1], off[1:])]
    assert kept_off.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert kept_offsets(np.zeros(0, dtype=np.uint8), [0, 0])[1].tolist() == [0, 0]
