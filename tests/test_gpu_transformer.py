"""Transformer x-vector extraction on the MI355X against the reference's own outputs (tests/golden/transformer_*.npz): the parity
modes at the project's gate, the interfaces, batch independence, the extraction script, and the 16-bit modes against a measured
yardstick.

The 16-bit yardstick.  tests/transformer_interp.run_graph(et=...) evaluates a fixture's program on CPU in float64 with exactly the
roundings of a 16-bit mode (features, every frames / grid / sequence tensor and the weights of the layers on them in the element
type, the attention probabilities rounded for the second product; the pooled tail unrounded).  The cosine loss 1 - cos against the
reference's embeddings, worst utterance of the fixture:

    fixture                   bf16         f16
    transformer_lin_small     6.27e-05     8.02e-07
    transformer_conv_small    7.23e-05     1.10e-06
    transformer_default       3.32e-05     3.25e-07
    transformer_far           1.04e-05     2.12e-07

(re-measured by tests/test_transformer_host.py).  The device is allowed twice that loss.  Cosines are formed in float64.
"""

import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import transformer_cases as TC

pytestmark = pytest.mark.gpu

H16_LOSS = {                       # measured on CPU, see the module docstring
    ("transformer_lin_small", "bf16"): 6.27e-05, ("transformer_lin_small", "f16"): 8.02e-07,
    ("transformer_conv_small", "bf16"): 7.23e-05, ("transformer_conv_small", "f16"): 1.10e-06,
    ("transformer_default", "bf16"): 3.32e-05, ("transformer_default", "f16"): 3.25e-07,
    ("transformer_far", "bf16"): 1.04e-05, ("transformer_far", "f16"): 2.12e-07,
}


def _cos(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a * b).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1)


def _launches(which):
    from libs.amd import capi
    return int(capi.lib().asv_kernel_launch_count(which))


@pytest.mark.parametrize("precision", ["f32", "f32x", "f32m"])
@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_transformer_parity_modes_vs_reference_golden(name, precision):
    """every fixture at the project's gate, rel err < 1e-4 per utterance, no range bit raised; one launch of the attention kernel per
    encoder layer and extraction, the front and positional kernels where the program has them"""
    from libs.amd import capi
    g, _, model = TC.golden_model(name)
    model.cuda()
    model.amd_precision = precision
    eng = model._amd_engine()
    eng.status()
    before = [_launches(k) for k in (capi.KERNEL_ATTENTION, capi.KERNEL_POSENC, capi.KERNEL_FRONT_CONV)]
    got = model.extract_embedding_batch(helpers.golden_feats(g)).numpy()
    assert eng.status() == 0
    moved = [_launches(k) - b for k, b in zip((capi.KERNEL_ATTENTION, capi.KERNEL_POSENC, capi.KERNEL_FRONT_CONV), before)]
    kinds = [op.kind for op in eng.ops]
    assert moved == [kinds.count("self_attention"), kinds.count("posenc"), kinds.count("front_conv")]
    assert kinds.count("self_attention") == len(model.transformer.encoders) and ("front_conv" in kinds) == ("_lin_" not in name)
    assert got.shape == g["embeddings"].shape
    for i, (T, _) in enumerate(g["utts"]):
        err = helpers.rel_err(got[i], g["embeddings"][i])
        print("[transformer] %s %s T=%d rel err %.3g" % (name, precision, T, err))
        assert err < 1e-4, "%s %s: utterance of %d frames: %g" % (name, precision, T, err)


@pytest.mark.parametrize("precision", ["bf16", "f16"])
@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_16bit_modes_within_twice_the_format_loss(name, precision):
    g, _, model = TC.golden_model(name)
    model.cuda()
    model.amd_precision = precision
    got = model.extract_embedding_batch(helpers.golden_feats(g)).numpy()
    assert np.isfinite(got).all()
    loss = 1.0 - _cos(got, g["embeddings"])
    print("[transformer] %s %s cosine loss %s (format alone: %.3g)" % (name, precision, ["%.3g" % v for v in loss], H16_LOSS[(name, precision)]))
    assert loss.max() <= 2.0 * H16_LOSS[(name, precision)], (name, precision, loss)


def test_extract_embedding_whole_and_single_utterance_interface():
    g, _, model = TC.golden_model("transformer_conv_small")
    model.cuda()
    model.amd_precision = "f32"
    mats = helpers.golden_feats(g)
    m = mats[3]                                                                         # 37 frames
    one = model.extract_embedding(m).numpy()
    assert helpers.rel_err(one, g["embeddings"][3]) < 1e-4
    whole = model.extract_embedding_whole(m, position="near", maxChunk=4000).numpy()
    assert np.array_equal(whole, one)
    halves = model.extract_embedding_whole(m, position="near", maxChunk=20).numpy()      # chunks of 18 and 19 frames, averaged by length
    assert halves.shape == one.shape and np.isfinite(halves).all() and not np.array_equal(halves, one)
    batch = model.extract_embedding_batch(mats).numpy()
    assert np.array_equal(batch[3], one) and model.embedding_dim() == 64
    long = model.extract_embedding(mats[5]).numpy()                                      # 650 frames: three chunks through the decorator's maxChunk=300
    assert np.array_equal(batch[5], long) and helpers.rel_err(long, g["embeddings"][5]) < 1e-4
    with pytest.raises(ValueError, match="at least 7"):
        model.extract_embedding(m[:6])
    with pytest.raises(ValueError, match="at least 7"):
        model.extract_embedding_whole(m[:13], maxChunk=7)                                # chunks of 6 and 7 frames


@pytest.mark.parametrize("precision", ["bf16", "f32m"])
def test_ragged_batch_neighbour_independence(precision):
    """every utterance of a ragged batch has the bits of its stand-alone extraction"""
    from libs.amd import synth
    g, _, model = TC.golden_model("transformer_conv_small")
    model.cuda()
    model.amd_precision = precision
    mats = [synth.synth_feats(T, 40, 9950 + i) for i, T in enumerate([200, 7, 77, 8, 333, 11])]
    full = model.extract_embedding_batch(mats).numpy()
    assert np.isfinite(full).all()
    for i in range(len(mats)):
        assert np.array_equal(model.extract_embedding(mats[i]).numpy(), full[i]), (precision, i)


def test_extract_embeddings_script_ark_to_ark(tmp_path):
    """pipeline/onestep/extract_embeddings.py with a generated nnet.config on five utterances equals the direct call"""
    import torch
    from libs.support import kaldi_io
    import libs.support.utils as utils
    from libs.amd import synth
    g, shapes, model = TC.golden_model("transformer_conv_small")
    sd = synth.synth_state_dict(shapes, int(g["wseed"]))
    mats = helpers.golden_feats(g)[1:]                                                   # 8, 11, 37, 301, 650 frames
    keys = ["utt%03d" % i for i in range(len(mats))]
    feats_ark = tmp_path / "feats.ark"
    with open(feats_ark, "wb") as f:
        for k, m in zip(keys, mats):
            kaldi_io.write_mat(f, m, key=k)
    params = tmp_path / "final.params"
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, str(params))
    cfg = tmp_path / "nnet.config"
    utils.write_nnet_config(os.path.join(helpers.MODEL_DIR, TC.BLUEPRINT), str(g["creation"]), str(cfg))
    out_ark = tmp_path / "xvector.ark"
    script = os.path.join(helpers.REPO, "asv-subtools_amd", "pytorch", "pipeline", "onestep", "extract_embeddings.py")
    res = subprocess.run([sys.executable, script, "--nnet-config", str(cfg), "--use-gpu", "true", "--gpu-id", "0", "--batch-frames", "700",
                          str(params), "ark:cat %s |" % feats_ark, "ark:| cat > %s" % out_ark], capture_output=True, text=True,
                         env=dict(os.environ, ASV_AMD_PRECISION="f32"), timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "Error" not in res.stdout + res.stderr
    import time
    for _ in range(100):
        if out_ark.exists() and out_ark.stat().st_size >= len(keys) * (64 * 4 + 10):
            break
        time.sleep(0.05)
    got = list(kaldi_io.read_vec_flt_ark(str(out_ark)))
    assert [k for k, _ in got] == keys
    model.cuda()
    model.amd_precision = "f32"
    for (k, v), m, ref in zip(got, mats, g["embeddings"][1:]):
        assert v.dtype == np.float32 and v.shape == (64,)
        assert np.array_equal(v, model.extract_embedding(m).numpy()), k
        assert helpers.rel_err(v, ref) < 1e-4, k
