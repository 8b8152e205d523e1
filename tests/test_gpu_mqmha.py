"""ECAPA-TDNN with multi-query multi-head attentive pooling (MQMHASP, reference libs/nnet/pooling.py:590-701) on the MI355X: against
the reference's own outputs (tests/golden/ecapa_mqmha_*.npz, tests/gen_mqmha_golden.py), and the one-launch pooling kernel
(mq_attentive_pool_kernel) against the heads x queries separate launches of attentive_pool_kernel it replaces - bit for bit."""

import numpy as np
import pytest

import helpers
from helpers import rel_err

pytestmark = pytest.mark.gpu

FIXTURES = ["ecapa_mqmha_roadmap", "ecapa_mqmha_shared", "ecapa_mqmha_q1"]
RAGGED = [300, 211, 300, 64, 500, 300, 2, 129, 1]
_models = {}


def _model(name):
    if name not in _models:
        g, sd, model = helpers.golden_model(name)
        model.cuda()
        _models[name] = (g, model)
    return _models[name]


def _ragged(dim):
    from libs.amd import synth
    return [synth.synth_feats(T, dim, 7400 + i) for i, T in enumerate(RAGGED)]


@pytest.mark.parametrize("precision", ["f32", "f32x", "f32m"])
@pytest.mark.parametrize("name", FIXTURES)
def test_mqmha_vs_reference_golden(name, precision):
    g, model = _model(name)
    model.amd_precision = precision
    got = model.extract_embedding_batch(helpers.golden_feats(g)).numpy()
    assert "mq_attentive_pool" in model._amd_engine().describe()
    assert got.shape == g["embeddings"].shape
    for i, (T, _) in enumerate(g["utts"]):
        err = rel_err(got[i], g["embeddings"][i])
        print("%s %s T=%d: rel err %.3g" % (name, precision, T, err))
        assert err < 1e-4, "%s %s: utterance of %d frames: %.3g" % (name, precision, T, err)
    assert model._amd_engine().status() == 0


def test_mqmha_bf16_is_close():
    g, model = _model("ecapa_mqmha_roadmap")
    model.amd_precision = "bf16"
    got = model.extract_embedding_batch(helpers.golden_feats(g)).numpy()
    ref = g["embeddings"]
    cos = (got * ref).sum(1) / np.linalg.norm(got, axis=1) / np.linalg.norm(ref, axis=1)
    print("bf16 cosines", cos)
    assert cos.min() > 0.999, cos


@pytest.mark.parametrize("precision", ["f32", "f32x", "f32m", "bf16", "f16"])
@pytest.mark.parametrize("name", FIXTURES)
def test_one_launch_pooling_gives_the_bits_of_the_separate_launches(name, precision, monkeypatch):
    """The fused kernel keeps attentive_pool_kernel's thread-to-(row, channel) mapping, reductions and accumulation statements per
    query, and writes the same columns: every embedding of a ragged batch (one- and two-frame utterances included) must be the
    same bits - in the f32 grades (two passes, libm exponentials) and in the 16-bit modes (one pass, running maxima)."""
    from libs.amd import capi
    L = capi.lib()
    g, model = _model(name)
    model.amd_precision = precision
    mats = _ragged(int(g["dim"]))
    n0 = L.asv_kernel_launch_count(capi.KERNEL_MQ_ATTPOOL)
    fused = model.extract_embedding_batch(mats).numpy()
    eng = model._amd_engine()
    assert L.asv_kernel_launch_count(capi.KERNEL_MQ_ATTPOOL) == n0 + 1            # one launch per extraction
    assert eng.describe().count("mq_attentive_pool") == 1 and " attentive_pool" not in eng.describe()
    assert [op.kind for op in eng.ops].count("mqattpool") == 1
    assert eng.status() == 0
    monkeypatch.setenv("ASV_AMD_MQPOOL", "0")
    plain = model.extract_embedding_batch(mats).numpy()
    eng0 = model._amd_engine()
    assert eng0 is not eng and "mq_attentive_pool" not in eng0.describe()
    n_pairs = model.stats.num_head * model.stats.num_q
    assert eng0.describe().count(" attentive_pool") == n_pairs and [op.kind for op in eng0.ops].count("attpool") == n_pairs
    assert L.asv_kernel_launch_count(capi.KERNEL_MQ_ATTPOOL) == n0 + 1            # did not rise
    assert eng0.status() == 0
    assert np.isfinite(fused).all()
    assert np.array_equal(fused, plain), (name, precision, int((fused != plain).sum()), rel_err(fused, plain))


@pytest.mark.parametrize("precision", ["bf16", "f32x"])
def test_mqmha_neighbour_independence(precision):
    """Utterances 0, 3, 8 of the ragged batch extracted alone give the bits they have in the batch (the modes of
    test_ecapa_batch_composition_invariance and the neighbour tests; not f32m, whose GEMM kernel choice moves with the batch size)."""
    g, model = _model("ecapa_mqmha_roadmap")
    model.amd_precision = precision
    mats = _ragged(int(g["dim"]))
    full = model.extract_embedding_batch(mats).numpy()
    assert np.isfinite(full).all()
    for i in (0, 3, 8):
        assert np.array_equal(model.extract_embedding(mats[i]).numpy(), full[i]), (precision, i)
    assert model._amd_engine().status() == 0
