"""Models whose layers use the activations beyond relu / tanh / sigmoid, or LayerNorm in place of the BatchNorm (`ln_replace`), on
the MI355X: against the embeddings the reference itself produced (tests/golden/rowop_*.npz, tests/gen_rowop_golden.py)."""

import numpy as np
import pytest

import helpers
from helpers import rel_err
from rowop_cases import FIXTURES, golden_model

pytestmark = pytest.mark.gpu

RAGGED = [300, 211, 64, 2, 1]
_models = {}


def _model(name):
    if name not in _models:
        g, sd, model = golden_model(name)
        model.cuda()
        _models[name] = (g, model)
    return _models[name]


@pytest.mark.parametrize("precision", ["f32", "f32x", "f32m"])
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_rowop_models_vs_reference_golden(name, precision):
    from libs.amd import capi
    L = capi.lib()
    g, model = _model(name)
    model.amd_precision = precision
    n0 = L.asv_kernel_launch_count(capi.KERNEL_ROWOP)
    got = model.extract_embedding_batch(helpers.golden_feats(g)).numpy()
    eng = model._amd_engine()
    assert eng.describe().count(": rowop ") == len(FIXTURES[name]) == [op.kind for op in eng.ops].count("rowop")
    assert L.asv_kernel_launch_count(capi.KERNEL_ROWOP) == n0 + len(FIXTURES[name])
    assert got.shape == g["embeddings"].shape and np.isfinite(got).all()
    for i, (T, _) in enumerate(g["utts"]):
        err = rel_err(got[i], g["embeddings"][i])
        print("%s %s T=%d: rel err %.3g" % (name, precision, T, err))
        assert err < 1e-4, "%s %s: utterance of %d frames: %.3g" % (name, precision, T, err)
    assert eng.status() == 0


def test_rowop_model_bf16_is_close():
    g, model = _model("rowop_lx_mish_ln")
    model.amd_precision = "bf16"
    got = model.extract_embedding_batch(helpers.golden_feats(g)).numpy()
    ref = g["embeddings"]
    cos = (got * ref).sum(1) / np.linalg.norm(got, axis=1) / np.linalg.norm(ref, axis=1)
    print("bf16 cosines", cos)
    assert cos.min() > 0.999, cos


@pytest.mark.parametrize("precision", ["bf16", "f32x"])
def test_rowop_model_neighbour_independence(precision):
    """Utterances of a ragged batch (300, 211, 64, 2, 1 frames) extracted alone give the bits they have in the batch."""
    from libs.amd import synth
    g, model = _model("rowop_lx_mish_ln")
    model.amd_precision = precision
    mats = [synth.synth_feats(T, int(g["dim"]), 9100 + i) for i, T in enumerate(RAGGED)]
    full = model.extract_embedding_batch(mats).numpy()
    assert np.isfinite(full).all()
    for i in range(len(mats)):
        assert np.array_equal(model.extract_embedding(mats[i]).numpy(), full[i]), (precision, i)
    assert model._amd_engine().status() == 0


def test_a_relu_xvector_has_no_row_op_and_does_not_move_the_counter():
    from libs.amd import capi
    L = capi.lib()
    g, sd, model = helpers.golden_model("xvector_near_ragged")
    model.cuda()
    model.amd_precision = "f32m"
    n0 = L.asv_kernel_launch_count(capi.KERNEL_ROWOP)
    got = model.extract_embedding_batch(helpers.golden_feats(g)[:5]).numpy()
    assert np.isfinite(got).all() and "rowop" not in model._amd_engine().describe()
    assert L.asv_kernel_launch_count(capi.KERNEL_ROWOP) == n0
