"""`--sliding true` of pipeline/onestep/extract_embeddings.py (the reference's diarisation mode: one vector per uniform sub-segment, CMN per
sub-segment) against the route that existed before it: the plain script over a range-specified scp 'file:offset[first:last]' of the same
windows with --cmn-window 300, which reads and decodes the whole parent once per window.  Same bits are asked for.  The model is the
`xvector_c1` golden's (30-dimensional input), precision f32, as in tests/test_gpu_pipeline_ingest.py."""

import os
import subprocess
import sys

import numpy as np
import pytest

import compressed_cases as cc
import helpers
from helpers import rel_err

pytestmark = pytest.mark.gpu

SCRIPT = os.path.join(helpers.REPO, "asv-subtools_amd", "pytorch", "pipeline", "onestep", "extract_embeddings.py")
ROWS = [40, 333, 700, 500]                               # three float32 parents and one 'CM ' parent
SEGMENTS = ["p0 rec0 0.0 0.4", "p1 rec1 0.0 3.33", "p2 rec2 0.0 7.0", "p3 rec3 2.5 7.5", "p2 rec2 10.0 13.3"]      # p2 has two segments


class Data(object):
    pass


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    import torch
    from libs.amd import subsegments, synth
    import libs.support.utils as utils
    d = Data()
    d.dir = tmp_path_factory.mktemp("windows")
    d.g, d.sd = helpers.golden_state_dict("xvector_c1")
    d.keys = ["p%d" % i for i in range(len(ROWS))]
    d.mats = [synth.synth_feats(T, 30, 300 + i) * 3.0 + 1.5 for i, T in enumerate(ROWS[:3])]
    body = cc.cm_body(np.random.RandomState(5), ROWS[3], 30)
    d.mats.append(cc.host_decode(1, body))
    d.feats_scp = d.dir / "feats.scp"
    lines = cc.write_ark(str(d.dir / "feats.ark"), [(k, cc.float_payload(m)) for k, m in zip(d.keys[:3], d.mats[:3])] +
                         [(d.keys[3], cc.compressed_payload(1, body))])
    d.feats_scp.write_text("\n".join(lines) + "\n")
    d.segments = d.dir / "segments"
    d.segments.write_text("\n".join(SEGMENTS) + "\n")
    # what the run has to make of the segments: the sub-segments, their rows, parents in scp order and each one's windows in start order
    d.subs = subsegments.uniform_subsegments(SEGMENTS)
    kept, first, last = subsegments.frame_ranges(d.subs, dict(zip(d.keys, ROWS)))
    assert len(kept) == len(d.subs)
    order = sorted(range(len(kept)), key=lambda w: (d.keys.index(kept[w][1]), first[w]))
    d.windows = [(kept[w][0], d.keys.index(kept[w][1]), first[w], last[w]) for w in order]
    d.ranged_scp = d.dir / "ranged.scp"
    rx = dict(line.split(None, 1) for line in lines)
    d.ranged_scp.write_text("".join("%s %s[%d:%d]\n" % (name, rx[d.keys[p]], a, b) for name, p, a, b in d.windows))
    d.params = d.dir / "final.params"
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in d.sd.items()}, str(d.params))
    d.cfg = d.dir / "nnet.config"
    utils.write_nnet_config(os.path.join(helpers.MODEL_DIR, "xvector.py"), str(d.g["creation"]), str(d.cfg))
    d.runs = {}
    return d


def run_script(d, name, rspec, extra, env=None, batch_frames=2048):
    """One run of the script (cached per name): (CompletedProcess, [(key, vector)])."""
    from libs.support import kaldi_io
    if name not in d.runs:
        out_ark = d.dir / ("xvector_%s.ark" % name)
        res = subprocess.run([sys.executable, SCRIPT, "--nnet-config", str(d.cfg), "--use-gpu", "true", "--gpu-id", "0", "--batch-frames", str(batch_frames)] +
                             extra + [str(d.params), rspec, "ark:%s" % out_ark], capture_output=True, text=True,
                             env=dict(os.environ, ASV_AMD_PRECISION="f32", **(env or {})), timeout=600)
        got = list(kaldi_io.read_vec_flt_ark(str(out_ark))) if res.returncode == 0 else []
        d.runs[name] = (res, got)
    return d.runs[name]


def oracle_run(d):
    """The route of the parent commit: every window a range-specified entry, CMN per entry."""
    res, got = run_script(d, "ranged", "scp:%s" % d.ranged_scp, ["--cmn-window", "300"])
    assert res.returncode == 0, res.stdout + res.stderr
    assert [k for k, _ in got] == [w[0] for w in d.windows]
    return got


def sliding_run(d, name, extra=(), **kw):
    res, got = run_script(d, name, "scp:%s" % d.feats_scp, ["--sliding", "true", "--segments", str(d.segments), "--cmn-window", "300"] + list(extra), **kw)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "Error" not in res.stdout + res.stderr and "ERROR" not in res.stdout + res.stderr
    return res, got


def same_bits(got, want):
    assert [k for k, _ in got] == [k for k, _ in want]
    for (k, v), (_, p) in zip(got, want):
        assert v.dtype == np.float32 and np.isfinite(v).all() and np.array_equal(v.view(np.uint32), p.view(np.uint32)), (k, rel_err(v, p))


def test_the_windows_are_what_the_test_means_them_to_be(data):
    d = data
    rows = [b - a + 1 for _, _, a, b in d.windows]
    assert 20 <= len(d.windows) <= 40 and max(rows) == 150 and min(rows) == 40
    assert [p for _, p, _, _ in d.windows] == sorted(p for _, p, _, _ in d.windows)
    assert sum(1 for w in d.windows if w[1] == 2 and w[2] == 0) == 2              # both segments of p2 start at its row 0
    assert max(b for _, p, _, b in d.windows if p == 2) == 699 and max(b for _, p, _, b in d.windows if p == 3) == 499


def test_sliding_equals_the_range_specified_scp_bit_for_bit(data):
    d = data
    res, got = sliding_run(d, "sliding", ["--subsegments-out", str(d.dir / "subsegments")])
    assert "Extracted %d embeddings." % len(d.windows) in res.stdout
    same_bits(got, oracle_run(d))
    want = ["%s %s %.3f %.3f" % s for s in d.subs]
    assert (d.dir / "subsegments").read_text().splitlines() == want and len(want) == len(d.windows)
    assert want[0] == "p0-00000000-00000040 p0 0.000 0.400"


def test_a_long_parent_is_cut_into_spans(data):
    """--batch-frames 256: the 700-row, the 500-row and the 333-row parents do not fit a buffer set; each is read span by span."""
    d = data
    _, got = sliding_run(d, "sliding_256", batch_frames=256)
    same_bits(got, oracle_run(d))


def test_host_decode_of_the_compressed_parent(data):
    d = data
    _, got = sliding_run(d, "sliding_host_decode", env={"ASV_AMD_DEVICE_DECODE": "0"})
    same_bits(got, oracle_run(d))


@pytest.fixture(scope="module")
def model(data):
    m = helpers.build_model("xvector.py", str(data.g["creation"]), data.sd)
    m.cuda()
    m.amd_precision = "f32"
    return m


def test_extract_sliding_equals_the_script(data, model):
    import torch
    from libs.amd import subsegments
    from libs.amd.pipeline import IngestOptions
    d = data
    mine = [w for w in d.windows if w[1] == 2]
    start, rows = [a for _, _, a, _ in mine], [b - a + 1 for _, _, a, b in mine]
    _, script = sliding_run(d, "sliding", ["--subsegments-out", str(d.dir / "subsegments")])
    want = np.stack([v for k, v in script if k.startswith("p2-")])
    for feats in (d.mats[2], torch.from_numpy(d.mats[2]).cuda()):
        got = subsegments.extract_sliding(model, feats, start, rows, ingest=IngestOptions(cmn_window=300))
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), rel_err(got, want)
    # several batches over the resident parent: the same vectors
    got = subsegments.extract_sliding(model, d.mats[2], start, rows, batch_frames=400, batch_utts=3)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_submit_windows_checks_its_arguments(data, model):
    from libs.amd.pipeline import DeviceSets, IngestOptions
    with pytest.raises(ValueError):
        DeviceSets(model, 512, 4, 30, 10000, n_sets=1, warm=False, windows=True)                                     # no ingest: no raw buffer
    with pytest.raises(ValueError):
        DeviceSets(model, 512, 4, 30, 10000, n_sets=1, warm=False, ingest=IngestOptions(300, 100, True, False, True), windows=True)
    plain = DeviceSets(model, 512, 4, 30, 10000, n_sets=1, warm=False, ingest=IngestOptions(300))
    with pytest.raises(ValueError):
        plain.submit_windows(0, 100, [0], [50])                                                                       # made without windows=True
    sets = DeviceSets(model, 512, 4, 30, 10000, n_sets=1, warm=False, ingest=IngestOptions(300), windows=True)
    for frames, start, rows in ((513, [0], [50]),                       # more raw rows than the set holds
                                (400, [0, 100, 200], [200, 200, 200]),  # the windows' rows do not fit
                                (400, [0] * 5, [10] * 5),               # more windows than batch_utts
                                (400, [380], [30]),                     # a window beyond the raw rows
                                (400, [10], [0]),                       # an empty window: the engine takes no empty utterance
                                (400, [-1], [10])):
        with pytest.raises(ValueError):
            sets.submit_windows(0, frames, start, rows)
    assert sets.pending[0] is None and sets.submitted == 0


def test_range_guard_reruns_on_the_gathered_rows(data):
    """A windows batch whose activations leave the half range of the f32x operand split is re-run by finish() on the bf16-halves twin:
    that re-run has to read the gathered, normalised rows of the windows (not the raw parents) - it gives, with the RuntimeWarning,
    what the same windows give as a host-packed batch through submit()."""
    import warnings
    from libs.amd.pipeline import DeviceSets, IngestOptions
    from oracle import fbank_oracle, np_oracle as O
    d = data
    model = helpers.build_model("xvector.py", str(d.g["creation"]), d.sd)
    model.cuda()
    model.amd_precision = "f32x"
    raw = np.concatenate([d.mats[1], (d.mats[0] * 1.0e5).astype(np.float32), d.mats[2][:300]])      # 333 + 40 + 300 rows; the middle parent is loud
    start, rows = [0, 75, 183, 333, 373, 448, 523], [150, 150, 150, 40, 150, 150, 150]
    packed = np.concatenate([raw[a:a + n] for a, n in zip(start, rows)])
    offs = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    sets = DeviceSets(model, 1024, 16, 30, 10000, n_sets=2, ingest=IngestOptions(300), windows=True)
    assert sets.watch
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        sets.host_buffer(0)[:len(raw)] = raw
        sets.submit_windows(0, len(raw), start, rows)
        a = sets.finish(0).copy()
        assert sets.range_reruns == 1 and any("f32x-bf16" in str(x.message) and issubclass(x.category, RuntimeWarning) for x in w)
        sets.host_buffer(1)[:len(packed)] = packed
        sets.submit(1, offs, len(packed))
        b = sets.finish(1).copy()
        assert sets.range_reruns == 2
    assert a.shape == (len(start), sets.embed_dim) and np.isfinite(a).all()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), rel_err(a, b)
    for i in (0, 3):                                                         # a quiet window and the loud one, against the CPU oracle
        feat = fbank_oracle.sliding_cmn(raw[start[i]:start[i] + rows[i]], cmn_window=300, center=True)
        want = O.extract_embedding(lambda c: O.xvector_embed(c, d.sd, "far"), feat)
        print("window %d: rel err vs oracle %.3g" % (i, rel_err(a[i], want)))
        assert rel_err(a[i], want) < 1e-4, (i, rel_err(a[i], want))          # (the bound of test_range_guard_reruns_on_the_compacted_rows)
