"""The reference's benchmark ECAPA-TDNN blueprint (model/ecapa-tdnn-xvector.py) on the MI355X against the reference's own outputs
(tests/golden/ecapa_bench_*.npz, tests/gen_ecapa_bench_golden.py), and its 64-wide Res2 chains as one kernel each
(res2n_chain_kernel, kernels_res2n.hip) against the per-branch layers they replace."""

import numpy as np
import pytest

import helpers
from helpers import rel_err

pytestmark = pytest.mark.gpu

TOL_F32 = 1e-4
CASES = ["ecapa_bench_default", "ecapa_bench_launcher", "ecapa_bench_c1024_far", "ecapa_bench_stats", "ecapa_bench_multihead"]
_models = {}


def _model(name):
    if name not in _models:
        g, sd, model = helpers.golden_model(name)
        _models[name] = (g, model.cuda())
    return _models[name]


def _cos(a, b):
    return (a * b).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1)


@pytest.mark.parametrize("precision", ["f32", "f32x", "f32m"])
@pytest.mark.parametrize("name", CASES)
def test_parity_modes_vs_reference_golden(name, precision):
    g, model = _model(name)
    model.amd_precision = precision
    got = model.extract_embedding_batch(helpers.golden_feats(g)).numpy()
    assert got.shape == g["embeddings"].shape and "res2n" not in model._amd_engine().describe()       # the parity modes keep one layer per branch
    errs = [rel_err(got[i], g["embeddings"][i]) for i in range(len(got))]
    print("[ecapa-bench] %s %s rel_err per utterance: %s" % (name, precision, " ".join("%.2e" % e for e in errs)))
    for (T, _), e in zip(g["utts"], errs):
        assert e < TOL_F32, "%s %s: utterance of %d frames: %.3g" % (name, precision, T, e)


@pytest.mark.parametrize("precision", ["bf16", "f16"])
@pytest.mark.parametrize("name", ["ecapa_bench_default", "ecapa_bench_launcher"])
def test_16_bit_modes_are_close(name, precision):
    g, model = _model(name)
    model.amd_precision = precision
    got = model.extract_embedding_batch(helpers.golden_feats(g)).numpy()
    cos = _cos(got, g["embeddings"])
    print("[ecapa-bench] %s %s cosine min %.6f" % (name, precision, cos.min()))
    assert cos.min() > 0.999, cos


@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_res2n_kernel_matches_per_branch_layers(precision, monkeypatch):
    """The 16-bit modes run each Res2Conv1dReluBn as one launch; ASV_AMD_NO_FUSE=1 keeps one launch per branch.  Same operands and the
    same rounding of every intermediate: the embeddings agree to the f32 summation order - on a ragged batch with tiny utterances and
    lengths around the recomputed margin (27, 28, 29), at all three dilations."""
    from libs.amd import capi, synth
    L = capi.lib()
    g, model = _model("ecapa_bench_default")
    model.amd_precision = precision
    batches = [helpers.golden_feats(g), [synth.synth_feats(T, 80, 7500 + i) for i, T in enumerate([1, 2, 7, 27, 28, 29, 33, 129, 300, 517])]]
    assert all(len(b) <= 16 for b in batches)
    n0 = L.asv_kernel_launch_count(capi.KERNEL_RES2N)
    fused = np.concatenate([model.extract_embedding_batch(b).numpy() for b in batches])
    assert L.asv_kernel_launch_count(capi.KERNEL_RES2N) == n0 + 3 * len(batches)      # three blocks, one launch each, per extraction
    assert model._amd_engine().describe().count("res2n") == 3
    monkeypatch.setenv("ASV_AMD_NO_FUSE", "1")
    plain = np.concatenate([model.extract_embedding_batch(b).numpy() for b in batches])
    assert L.asv_kernel_launch_count(capi.KERNEL_RES2N) == n0 + 3 * len(batches)      # did not rise
    assert "res2n" not in model._amd_engine().describe()
    assert np.isfinite(fused).all() and np.isfinite(plain).all()
    cos = _cos(fused, plain)
    print("[ecapa-bench] fused vs per-branch %s: cosine min %.6f rel_err %.2e" % (precision, cos.min(), rel_err(fused, plain)))
    assert cos.min() > 0.9999 and rel_err(fused, plain) < 1e-2, (cos.min(), rel_err(fused, plain))


def test_the_switch_keeps_the_per_branch_layers(monkeypatch):
    g, model = _model("ecapa_bench_launcher")
    model.amd_precision = "bf16"
    monkeypatch.setenv("ASV_AMD_RES2N", "0")
    got = model.extract_embedding_batch(helpers.golden_feats(g)[:3]).numpy()
    assert "res2n" not in model._amd_engine().describe() and np.isfinite(got).all()


def test_neighbour_independence_in_bf16():
    """An utterance's embedding is bit-equal alone and inside a batch, between longer and shorter neighbours, and a neighbour scaled by
    1e5 changes nothing in the others (its own rows may overflow: they are its own)."""
    from libs.amd import synth
    g, model = _model("ecapa_bench_default")
    model.amd_precision = "bf16"
    lens = [517, 2, 40, 300, 64, 1, 300, 9]
    mats = [synth.synth_feats(T, 80, 7600 + i) for i, T in enumerate(lens)]
    full = model.extract_embedding_batch(mats).numpy()
    assert np.isfinite(full).all()
    for i in (1, 4, 6):                                                  # 2, 64 and 300 frames
        assert np.array_equal(model.extract_embedding(mats[i]).numpy(), full[i]), lens[i]
    loud = list(mats)
    loud[3] = (mats[3] * 1.0e5).astype(np.float32)
    other = model.extract_embedding_batch(loud).numpy()
    keep = [i for i in range(len(mats)) if i != 3]
    assert np.array_equal(other[keep], full[keep])
