"""RepVGG / RepSPK x-vector extraction on the MI355X against the reference's own outputs (tests/golden/repvgg_*.npz): the parity
modes at the project's gate, both checkpoint forms, batch independence, and the 16-bit modes against a measured yardstick.

The 16-bit yardstick.  tests/repvgg_interp.run_graph_rounded evaluates a fixture's program on CPU in float64 with exactly the
roundings of a 16-bit mode (features, grid tensors and grid-layer weights stored in the element type; the pooled tail unrounded).
The cosine loss 1 - cos against the reference's embeddings, worst utterance of the fixture:

    fixture                bf16         f16
    repvgg_spk_small       1.45e-05     1.75e-07
    repvgg_vgg_small       2.58e-05     3.99e-07
    repvgg_spk_default     8.56e-06     1.75e-07

(re-measured by tests/test_repvgg_host.py).  The device is allowed twice that loss: floors 1 - 2 x loss, i.e. bf16 0.999971 /
0.999948 / 0.999983 and f16 0.99999965 / 0.99999920 / 0.99999965.  Cosines are formed in float64.
"""

import numpy as np
import pytest

import helpers
import repvgg_cases as RC

pytestmark = pytest.mark.gpu

H16_LOSS = {                       # measured on CPU, see the module docstring
    ("repvgg_spk_small", "bf16"): 1.45e-05, ("repvgg_spk_small", "f16"): 1.75e-07,
    ("repvgg_vgg_small", "bf16"): 2.58e-05, ("repvgg_vgg_small", "f16"): 3.99e-07,
    ("repvgg_spk_default", "bf16"): 8.56e-06, ("repvgg_spk_default", "f16"): 1.75e-07,
}


def _cos(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a * b).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1)


def _taps_launches():
    from libs.amd import capi
    return int(capi.lib().asv_kernel_launch_count(capi.KERNEL_CONV_TAPS))


@pytest.mark.parametrize("precision", ["f32", "f32x", "f32m"])
@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_repvgg_parity_modes_vs_reference_golden(name, precision):
    """every fixture at the project's gate, rel err < 1e-4 per utterance, no range bit raised; RepSPK fixtures run their stride-1
    blocks on the tap-table kernel (one launch per block and extraction), the RepVGG fixture never does"""
    g, model = RC.golden_model(name)
    model.cuda()
    model.amd_precision = precision
    eng = model._amd_engine()
    eng.status()
    before = _taps_launches()
    got = model.extract_embedding_batch(helpers.golden_feats(g)).numpy()
    assert eng.status() == 0
    assert _taps_launches() - before == sum(op.kind == "grid_conv" for op in eng.ops)
    assert any(op.kind == "grid_conv" for op in eng.ops) == ("_vgg_" not in name)
    assert got.shape == g["embeddings"].shape
    for i, (T, _) in enumerate(g["utts"]):
        err = helpers.rel_err(got[i], g["embeddings"][i])
        print("[repvgg] %s %s T=%d rel err %.3g" % (name, precision, T, err))
        assert err < 1e-4, "%s %s: utterance of %d frames: %g" % (name, precision, T, err)


def test_deploy_and_training_form_engines_agree():
    """the two engines fold the same taps and bias from differently rounded float32 weights: 1e-5 relative in f32, not the bits"""
    g, train = RC.golden_model("repvgg_spk_small")
    _, deploy = RC.golden_model("repvgg_spk_deploy")
    mats = helpers.golden_feats(g)
    outs = []
    for model in (train, deploy):
        model.cuda()
        model.amd_precision = "f32"
        outs.append(model.extract_embedding_batch(mats).numpy())
    assert [op.kind for op in train._amd_engine().ops] == [op.kind for op in deploy._amd_engine().ops]
    for i in range(len(mats)):
        assert helpers.rel_err(outs[1][i], outs[0][i]) < 1e-5, (i, helpers.rel_err(outs[1][i], outs[0][i]))


def test_extract_embedding_whole_and_single_utterance_interface():
    g, model = RC.golden_model("repvgg_spk_small")
    model.cuda()
    model.amd_precision = "f32"
    m = helpers.golden_feats(g)[1]
    one = model.extract_embedding(m).numpy()
    assert helpers.rel_err(one, g["embeddings"][1]) < 1e-4
    whole = model.extract_embedding_whole(m, position="near", maxChunk=4000).numpy()
    assert np.array_equal(whole, one)
    halves = model.extract_embedding_whole(m, position="near", maxChunk=20).numpy()      # 37 frames: chunks of 18 and 19, averaged by length
    assert halves.shape == one.shape and np.isfinite(halves).all() and not np.array_equal(halves, one)


@pytest.mark.parametrize("precision", ["bf16", "f32m"])
def test_ragged_batch_neighbour_independence(precision):
    """every utterance of a ragged batch has the bits of its stand-alone extraction"""
    from libs.amd import synth
    g, model = RC.golden_model("repvgg_spk_small")
    model.cuda()
    model.amd_precision = precision
    mats = [synth.synth_feats(T, 40, 9500 + i) for i, T in enumerate([200, 1, 77, 2, 333, 9])]
    full = model.extract_embedding_batch(mats).numpy()
    assert np.isfinite(full).all()
    for i in range(len(mats)):
        assert np.array_equal(model.extract_embedding(mats[i]).numpy(), full[i]), (precision, i)


@pytest.mark.parametrize("precision", ["bf16", "f16"])
@pytest.mark.parametrize("name", ["repvgg_spk_small", "repvgg_vgg_small", "repvgg_spk_default"])
def test_16bit_modes_within_twice_the_format_loss(name, precision):
    g, model = RC.golden_model(name)
    model.cuda()
    model.amd_precision = precision
    got = model.extract_embedding_batch(helpers.golden_feats(g)).numpy()
    assert np.isfinite(got).all()
    loss = 1.0 - _cos(got, g["embeddings"])
    print("[repvgg] %s %s cosine loss %s (format alone: %.3g)" % (name, precision, ["%.3g" % v for v in loss], H16_LOSS[(name, precision)]))
    assert loss.max() <= 2.0 * H16_LOSS[(name, precision)], (name, precision, loss)
