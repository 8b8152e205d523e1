"""Raw feats.scp + vad.scp -> embeddings: `--cmn-window` / `--vad-scp` of pipeline/onestep/extract_embeddings.py (sliding CMN and
voiced-frame selection on the device, inside the extraction loop) against the plain path on pre-processed features, and against the
CPU oracle on the float64-restated features.  The model is the `xvector_c1` golden's (30-dimensional input), precision f32."""

import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
from helpers import rel_err

pytestmark = pytest.mark.gpu

SCRIPT = os.path.join(helpers.REPO, "asv-subtools_amd", "pytorch", "pipeline", "onestep", "extract_embeddings.py")
LENS = [412, 40, 700, 133, 64, 300, 555, 41, 256, 97, 688, 350]
NO_ENTRY, WRONG_LENGTH, SILENT = 2, 5, 8
CMN = dict(cmn_window=300, center=True)


class Data(object):
    pass


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """12 utterances of raw features as feats.ark / feats.scp, their VAD vectors as vad.ark / vad.scp (three unusable), the model files,
    and the outputs of the script runs the tests share."""
    import torch
    from libs.amd import synth
    from libs.support import kaldi_io
    import libs.support.utils as utils
    d = Data()
    d.dir = tmp_path_factory.mktemp("ingest")
    d.g, d.sd = helpers.golden_state_dict("xvector_c1")
    d.keys = ["utt%02d" % i for i in range(len(LENS))]
    d.mats = [synth.synth_feats(T, 30, 900 + i) * 3.0 + 1.5 for i, T in enumerate(LENS)]
    rng = np.random.RandomState(3)
    d.flags = [(rng.rand(T) < 0.7).astype(np.float32) for T in LENS]
    d.flags[SILENT][:] = 0.0
    d.feats_ark, d.feats_scp, d.vad_scp = d.dir / "feats.ark", d.dir / "feats.scp", d.dir / "vad.scp"
    with open(d.feats_ark, "wb") as f, open(d.feats_scp, "w") as s:
        for k, m in zip(d.keys, d.mats):
            f.write((k + " ").encode())
            s.write("%s %s:%d\n" % (k, d.feats_ark, f.tell()))
            kaldi_io.write_mat(f, m)
    with open(d.dir / "vad.ark", "wb") as f, open(d.vad_scp, "w") as s:
        for i, (k, v) in enumerate(zip(d.keys, d.flags)):
            if i == NO_ENTRY:
                continue
            f.write((k + " ").encode())
            s.write("%s %s:%d\n" % (k, d.dir / "vad.ark", f.tell()))
            kaldi_io.write_vec_flt(f, v[:-2] if i == WRONG_LENGTH else v)
    d.kept = [i for i in range(len(LENS)) if i not in (NO_ENTRY, WRONG_LENGTH, SILENT)]
    d.params = d.dir / "final.params"
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in d.sd.items()}, str(d.params))
    d.cfg = d.dir / "nnet.config"
    utils.write_nnet_config(os.path.join(helpers.MODEL_DIR, "xvector.py"), str(d.g["creation"]), str(d.cfg))
    d.runs = {}
    return d


def run_script(d, name, rspec, extra):
    """One run of the script (cached per name): (CompletedProcess, [(key, vector)])."""
    from libs.support import kaldi_io
    if name not in d.runs:
        out_ark = d.dir / ("xvector_%s.ark" % name)
        env = dict(os.environ, ASV_AMD_PRECISION="f32")
        res = subprocess.run([sys.executable, SCRIPT, "--nnet-config", str(d.cfg), "--use-gpu", "true", "--gpu-id", "0", "--batch-frames", "1500"] + extra +
                             [str(d.params), rspec, "ark:%s" % out_ark], capture_output=True, text=True, env=env, timeout=600)
        got = list(kaldi_io.read_vec_flt_ark(str(out_ark))) if res.returncode == 0 else []
        d.runs[name] = (res, got)
    return d.runs[name]


def raw_run(d, mode):
    rspec = "ark:cat %s |" % d.feats_ark if mode == "ark" else "scp:%s" % d.feats_scp
    return run_script(d, "raw_" + mode, rspec, ["--cmn-window", "300", "--vad-scp", str(d.vad_scp)])


@pytest.mark.parametrize("mode", ["ark", "scp"])
def test_raw_features_with_cmn_and_vad(data, mode):
    d = data
    res, got = raw_run(d, mode)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "Error" not in res.stdout + res.stderr and "ERROR" not in res.stdout + res.stderr
    assert [k for k, _ in got] == [d.keys[i] for i in d.kept] and len(got) == 9
    warnings = [l for l in res.stderr.splitlines() if l.startswith("WARNING: ")]
    assert len(warnings) == 3, res.stderr
    for i in (NO_ENTRY, WRONG_LENGTH, SILENT):
        assert sum(d.keys[i] in w for w in warnings) == 1
    assert "Extracted 9 embeddings" in res.stdout and "skipped 3" in res.stdout


def test_equals_the_plain_path_on_preprocessed_features(data):
    """The unchanged plain path on an archive prepared on the device with the EXISTING cmvn_sliding + select_voiced: the same bits."""
    import torch
    from libs.amd import frontend
    from libs.support import kaldi_io
    d = data
    pre_ark = d.dir / "pre.ark"
    with open(pre_ark, "wb") as f:
        for i in d.kept:
            x = torch.from_numpy(d.mats[i]).cuda()
            off = np.array([0, LENS[i]], dtype=np.int64)
            voiced = torch.from_numpy(d.flags[i].astype(np.uint8)).cuda()
            rows, _ = frontend.select_voiced(frontend.cmvn_sliding(x, off, min_window=100, **CMN), voiced, off, [int(d.flags[i].sum())])
            kaldi_io.write_mat(f, rows.cpu().numpy(), key=d.keys[i])
    res, plain = run_script(d, "plain", "ark:%s" % pre_ark, [])
    assert res.returncode == 0, res.stdout + res.stderr
    assert "Extracted 9 embeddings." in res.stdout
    for mode in ("ark", "scp"):
        res, got = raw_run(d, mode)
        assert res.returncode == 0, res.stdout + res.stderr
        assert [k for k, _ in got] == [k for k, _ in plain]
        for (k, v), (_, p) in zip(got, plain):
            assert v.dtype == np.float32 and np.array_equal(v.view(np.uint32), p.view(np.uint32)), (mode, k, rel_err(v, p))


def test_within_the_gate_of_the_cpu_oracle(data):
    from oracle import fbank_oracle, np_oracle as O
    d = data
    res, got = raw_run(d, "ark")
    assert res.returncode == 0, res.stdout + res.stderr
    assert len(got) == len(d.kept)
    for (k, v), i in zip(got, d.kept):
        feat = fbank_oracle.sliding_cmn(d.mats[i], **CMN)[d.flags[i] > 0]
        want = O.extract_embedding(lambda c: O.xvector_embed(c, d.sd, "far"), feat)
        err = rel_err(v, want)
        assert err < 1e-4, (k, err)


def test_sharded_cmn_equals_the_stream_path(data):
    d = data
    res, stream = run_script(d, "cmn_stream", "scp:%s" % d.feats_scp, ["--cmn-window", "300"])
    assert res.returncode == 0, res.stdout + res.stderr
    res, sharded = run_script(d, "cmn_sharded", "scp:%s" % d.feats_scp, ["--cmn-window", "300", "--sharded", "true"])
    assert res.returncode == 0, res.stdout + res.stderr
    assert "Extracted 12 embeddings." in res.stdout
    assert [k for k, _ in stream] == d.keys and [k for k, _ in sharded] == d.keys
    for (k, a), (_, b) in zip(stream, sharded):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (k, rel_err(b, a))


def test_device_sets_with_and_without_ingest(data):
    """libs.amd.pipeline.DeviceSets directly: ingest=None allocates nothing; with ingest the buffer path, the over-long-utterance path
    (an ndarray of its own) and a batch that keeps nothing; results equal the model on the rows prepared by the existing launches."""
    import torch
    from libs.amd import frontend
    from libs.amd.pipeline import DeviceSets, IngestOptions
    d = data
    model = helpers.build_model("xvector.py", str(d.g["creation"]), d.sd)
    model.cuda()
    model.amd_precision = "f32"
    plain = DeviceSets(model, 2048, 16, 30, 10000, n_sets=2, warm=False)
    assert plain.ingest is None and plain.dev_raw is None and plain.host_flags is None and plain.flags_np is None and plain.dev_flags is None
    use = [0, 3, 8, 1, 4]                                                      # (8 keeps nothing)
    mats = [d.mats[i] for i in use]
    flags = np.concatenate([d.flags[i] for i in use]).astype(np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(m) for m in mats])]).astype(np.int32)
    rows = int(offs[-1])
    prepared = []
    for i in use:
        if i == SILENT:
            continue
        x = torch.from_numpy(d.mats[i]).cuda()
        off = np.array([0, LENS[i]], dtype=np.int64)
        prepared.append(frontend.select_voiced(frontend.cmvn_sliding(x, off, min_window=100, **CMN), torch.from_numpy(d.flags[i].astype(np.uint8)).cuda(), off,
                                               [int(d.flags[i].sum())])[0].cpu().numpy())
    want = model.extract_embedding_batch(prepared).numpy()
    for results in ("host", "device"):
        sets = DeviceSets(model, rows + 8, 16, 30, 10000, n_sets=2, results=results, ingest=IngestOptions(300, 100, True, False, True))
        assert len(sets.dev_raw) == 2 and sets.dev_raw[0].shape == (rows + 8, 30) and sets.host_flags[0].is_pinned()
        assert sets.flag_buffer(1).shape == (rows + 8,) and sets.dev_flags[0].dtype == torch.uint8
        sets.host_buffer(0)[:rows] = np.concatenate(mats)
        sets.flag_buffer(0)[:rows] = flags
        sets.submit(0, offs, rows, voiced=sets.flag_buffer(0)[:rows])
        a = sets.finish(0)
        a = a.copy() if results == "host" else a.cpu().numpy()
        sets.submit(1, offs, np.concatenate(mats), voiced=flags)               # the ndarray path (an utterance longer than the buffer takes it)
        b = sets.finish(1)
        b = b.copy() if results == "host" else b.cpu().numpy()
        silent = np.zeros(LENS[SILENT], dtype=np.uint8)
        sets.host_buffer(0)[:LENS[SILENT]] = d.mats[SILENT]
        assert sets.submit(0, np.array([0, LENS[SILENT]], dtype=np.int32), LENS[SILENT], voiced=silent) is None and sets.finish(0) is None
        with pytest.raises(ValueError):
            sets.submit(0, offs, rows)                                         # flags are expected
        sets.flush()
        assert a.shape == want.shape and np.array_equal(a, want) and np.array_equal(b, want), (results, rel_err(a, want), rel_err(b, want))


def test_range_guard_reruns_on_the_compacted_rows(data):
    """A batch whose activations leave the half range of the f32x operand split is re-run by finish() on the bf16-halves twin: with
    ingest that re-run has to read the normalised, compacted rows and offsets (not the raw buffer), on both input branches."""
    import warnings
    from libs.amd.pipeline import DeviceSets, IngestOptions
    from oracle import fbank_oracle, np_oracle as O
    d = data
    model = helpers.build_model("xvector.py", str(d.g["creation"]), d.sd)
    model.cuda()
    model.amd_precision = "f32x"
    use = [3, 8, 9, 4]                                                         # (8 keeps nothing)
    mats = [d.mats[i].copy() for i in use]
    mats[2] = (mats[2] * 1.0e5).astype(np.float32)
    flags = np.concatenate([d.flags[i] for i in use]).astype(np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(m) for m in mats])]).astype(np.int32)
    rows = int(offs[-1])
    want = np.stack([O.extract_embedding(lambda c: O.xvector_embed(c, d.sd, "far"), fbank_oracle.sliding_cmn(m, **CMN)[d.flags[i] > 0])
                     for m, i in zip(mats, use) if i != SILENT])
    assert np.isfinite(want).all()
    sets = DeviceSets(model, rows + 8, 16, 30, 10000, n_sets=2, ingest=IngestOptions(300, 100, True, False, True))
    assert sets.watch
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        sets.host_buffer(0)[:rows] = np.concatenate(mats)
        sets.flag_buffer(0)[:rows] = flags
        sets.submit(0, offs, rows, voiced=sets.flag_buffer(0)[:rows])
        a = sets.finish(0).copy()
        assert sets.range_reruns == 1 and any("f32x-bf16" in str(x.message) for x in w)
        sets.submit(1, offs, np.concatenate(mats), voiced=flags)               # the ndarray branch
        b = sets.finish(1).copy()
        assert sets.range_reruns == 2
    assert a.shape == want.shape
    for i in range(len(want)):
        assert rel_err(a[i], want[i]) < 1e-4 and rel_err(b[i], want[i]) < 1e-4, (i, rel_err(a[i], want[i]), rel_err(b[i], want[i]))
