"""PLP and spectrogram features on the device (csrc/frontend.hip: the ASV_FEAT_PLP / ASV_FEAT_SPECTROGRAM instantiations of the two feature
kernels and plp_lpc_kernel) against the reference's own outputs, tests/golden/plp_spectrogram.npz (written by tests/gen_plp_golden.py
from the reference's code; nothing here runs that code).

The bound, per case: max |device - float64 restatement| <= 4 e_ref, where e_ref = max |reference float32 - float64 restatement| is
stored in the fixture (2.1e-6 .. 1.2e-4 for PLP, whose recursion amplifies input rounding; 2.4e-5 .. 3.2e-5 for the spectrograms with
the emptiest 0.5 % of the bins left out).  The factor 4 is the one the attention kernel and the PLDA score normalisation use: it allows
for the device's FFT and mel summation orders differing from torch's rfft + mm.  Every test prints its figures before it asserts.
Measured on one MI355X (DESIGN.md section 4.3.4 has the table): the device lies 0.65 .. 1.19 e_ref from the restatement in the PLP cases
(sre-plp-20 1.21e-5 at e_ref 1.40e-5, asvspoof-plp-40 1.20e-4 at 1.24e-4) and 0.94 .. 1.84 e_ref in the spectrogram cases
(asvspoof-spectrogram 3.04e-5 at 3.23e-5, spectrogram-8k 5.05e-5 at 2.74e-5).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import plp_cases as P

pytestmark = pytest.mark.gpu


def _device(name, waves=None, **extra):
    from libs.amd import frontend
    _, kind, kw, _ = P.case(name)
    feats, off = frontend.fbank_packed(P.golden_waves(name) if waves is None else waves, kind=kind, **dict(kw, **extra))
    return feats.cpu().numpy(), off


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_case_against_the_reference(name):
    ref, off, e_ref = P.golden_reference(name)
    got, got_off = _device(name)
    assert got.shape == ref.shape and list(got_off) == list(off) and np.isfinite(got).all()
    err, to_ref = P.max_err(got, name), float(np.abs(got.astype(np.float64) - ref)[P.compared(name)].max())
    print("%s: e_ref %.3e, device %.3e from the float64 restatement (%.2f e_ref), %.3e from the reference" % (name, e_ref, err, err / e_ref, to_ref))
    assert err <= 4.0 * e_ref


@pytest.mark.parametrize("name", ["sre-plp-20", "asvspoof-plp-40", "asvspoof-spectrogram", "spectrogram-8k", "plp-no-snip"])
def test_pcm16_equals_float_input_bit_for_bit(name):
    as_i16, off16 = _device(name)                                               # the fixture's waves are int16
    as_f32, off32 = _device(name, waves=[w.astype(np.float32) for w in P.golden_waves(name)])
    assert list(off16) == list(off32) and as_i16.shape[0] > 0 and np.array_equal(as_i16, as_f32)


@pytest.mark.parametrize("name", ["sre-plp-20", "asvspoof-plp-40", "asvspoof-spectrogram", "plp-short-utterance", "plp-one-frame"])
def test_rows_do_not_depend_on_the_neighbours(name):
    """An utterance alone gives the rows it gives inside the batch (other frame numbers, other lanes of plp_lpc_kernel, other waves)."""
    waves = P.golden_waves(name)
    batch, off = _device(name)
    for i, w in enumerate(waves):
        if off[i + 1] == off[i]:
            continue                                                            # no frame: nothing to launch for it alone
        alone, _ = _device(name, waves=[w])
        assert np.array_equal(alone, batch[off[i]:off[i + 1]]), (name, i)
    rev, roff = _device(name, waves=waves[::-1])
    n = len(waves)
    for i in range(n):
        assert np.array_equal(rev[roff[n - 1 - i]:roff[n - i]], batch[off[i]:off[i + 1]]), (name, i)


def test_dim_of_the_c_interface_is_the_written_width():
    """asv_fbank_dim = the row pitch asv_fbank writes with: the rows are written into a buffer of NaN of exactly that size."""
    import torch
    from libs.amd import capi, frontend
    for name in ("sre-plp-20", "asvspoof-spectrogram", "spectrogram-8k", "plp-fewer-ceps"):
        _, kind, kw, _ = P.case(name)
        ref, off, _ = P.golden_reference(name)
        opts, _ = frontend.fbank_options(kind, **kw)
        dim = capi.lib().asv_fbank_dim(C.byref(opts))
        waves = P.golden_waves(name)
        sample_off = np.zeros(len(waves) + 1, dtype=np.int64)
        np.cumsum([len(w) for w in waves], out=sample_off[1:])
        wave = torch.from_numpy(np.concatenate(waves)).cuda()
        out = torch.full((int(off[-1]) * dim + 64,), float("nan"), dtype=torch.float32, device="cuda")
        capi.check(capi.lib().asv_fbank_pcm16(C.byref(opts), C.c_void_p(wave.data_ptr()), sample_off.ctypes.data_as(C.POINTER(C.c_longlong)), len(waves),
                                              C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "asv_fbank_pcm16")
        host = out.cpu().numpy()
        assert dim == ref.shape[1] and np.isfinite(host[:off[-1] * dim]).all() and np.isnan(host[off[-1] * dim:]).all(), name
        assert np.array_equal(host[:off[-1] * dim].reshape(-1, dim), _device(name)[0]), name


def test_kind_zero_with_the_longer_struct_is_the_old_call():
    """feature_kind 0 through the longer options block = the call with the struct_size of before, bit for bit (fbank and MFCC, both kernels)."""
    import torch
    from libs.amd import capi, frontend
    waves = P.golden_waves("sre-plp-20")
    sample_off = np.zeros(len(waves) + 1, dtype=np.int64)
    np.cumsum([len(w) for w in waves], out=sample_off[1:])
    wave = torch.from_numpy(np.concatenate(waves)).cuda()
    for kind, kw in (("fbank", dict(num_mel_bins=40, use_energy=True)), ("mfcc", dict(num_ceps=20, num_mel_bins=30)), ("fbank", dict(frame_length=50.0, num_mel_bins=80))):
        new, off = frontend.fbank_device(wave, sample_off, kind=kind, **kw)
        opts, o = frontend.fbank_options(kind, **kw)
        opts.struct_size = capi.FBANK_OPTS_SIZE_V1
        opts.feature_kind, opts.lpc_order, opts.return_raw_fft = 2, 99, 1        # behind the declared size: must not be read
        old = torch.full_like(new, float("nan"))
        capi.check(capi.lib().asv_fbank_pcm16(C.byref(opts), C.c_void_p(wave.data_ptr()), sample_off.ctypes.data_as(C.POINTER(C.c_longlong)), len(waves),
                                              C.c_void_p(old.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "asv_fbank_pcm16")
        assert new.shape[0] == off[-1] > 0 and torch.equal(new, old), (kind, kw)


def test_kaldi_feature_plp_and_mean_norm():
    import torch
    from libs.amd import frontend
    from libs.egs.kaldi_features import KaldiFeature
    waves = [w.astype(np.float32) for w in P.golden_waves("sre-plp-20")[:3]]
    n = max(len(w) for w in waves)
    batch = torch.zeros(len(waves), n)
    for i, w in enumerate(waves):
        batch[i, :len(w)] = torch.from_numpy(w)
    kw = dict(P.case("sre-plp-20")[2])
    got = KaldiFeature("plp", kw, {"mean_norm": True})(batch.cuda(), torch.tensor([len(w) / n for w in waves]))
    want = frontend.plp(waves, mean_norm=True, **kw)
    assert len(got) == 3 and all(torch.equal(a, b) and a.shape[1] == 20 for a, b in zip(got, want))


def test_online_script_with_plp_features(tmp_path):
    """extract_embeddings_online.py with feature_type: plp on a tiny x-vector = extract_embedding_batch on frontend.plp features; a feature
    width that is not the model's inputs_dim is a ValueError naming both numbers."""
    import wave
    import torch
    import yaml
    from libs.amd import frontend
    from libs.support import kaldi_io
    import libs.support.utils as utils
    g, sd = helpers.golden_state_dict("xvector_c1")                # Xvector(30, ...)
    waves = [P.golden()["wave_" + u] for u in "aec"]               # 0.6 s, 0.4 s, 0.31 s
    scp = tmp_path / "wav.scp"
    with open(scp, "w") as f:
        for i, wv in enumerate(waves):
            path = tmp_path / ("u%d.wav" % i)
            with wave.open(str(path), "wb") as wf:
                wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(16000)
                wf.writeframes(wv.tobytes())
            f.write("utt%d %s\n" % (i, path))
    featset = {"num_mel_bins": 40, "lpc_order": 29, "num_ceps": 30, "dither": 0.0}
    params = tmp_path / "final.params"
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, str(params))
    cfg = tmp_path / "nnet.config"
    utils.write_nnet_config(os.path.join(helpers.MODEL_DIR, "xvector.py"), str(g["creation"]), str(cfg))
    script = os.path.join(helpers.REPO, "asv-subtools_amd", "pytorch", "pipeline", "onestep", "extract_embeddings_online.py")
    env = dict(os.environ, ASV_AMD_PRECISION="f32")

    def run(conf_dict, out_ark):
        conf = tmp_path / "feat.yaml"
        conf.write_text(yaml.safe_dump(conf_dict))
        return subprocess.run([sys.executable, script, "--nnet-config", str(cfg), "--data-type", "raw", "--feat-config", str(conf), "--gpu-id", "0",
                               str(params), str(scp), str(out_ark)], capture_output=True, text=True, env=env, timeout=600)

    res = run({"feature_type": "plp", "kaldi_featset": featset, "mean_var_conf": {"mean_norm": True, "std_norm": False}}, tmp_path / "xvector.ark")
    assert res.returncode == 0, res.stdout + res.stderr
    got = list(kaldi_io.read_vec_flt_ark(str(tmp_path / "xvector.ark")))
    assert [k for k, _ in got] == ["utt0", "utt1", "utt2"]
    model = helpers.build_model("xvector.py", str(g["creation"]), sd)
    model.cuda()
    model.amd_precision = "f32"
    direct = model.extract_embedding_batch(frontend.plp(waves, mean_norm=True, **featset)).numpy()
    for (k, v), d in zip(got, direct):
        assert np.array_equal(v, d), k
    bad = run({"feature_type": "plp", "kaldi_featset": dict(featset, num_ceps=20), "mean_var_conf": {}}, tmp_path / "bad.ark")
    assert bad.returncode != 0 and "ValueError" in bad.stdout + bad.stderr and "width 20" in bad.stdout + bad.stderr and "inputs_dim is 30" in bad.stdout + bad.stderr
