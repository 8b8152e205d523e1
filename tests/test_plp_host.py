"""PLP and spectrogram features, host side (no GPU): the numpy restatement of tests/plp_cases.py against the reference's own outputs in
tests/golden/plp_spectrogram.npz, the widths and frame counts of every case, the refusals of the Python and of the C interface (which
come before anything touches a device), the KaldiFeature kinds, and header / ctypes agreement.

Bounds.  e_ref (stored per case) = max |reference float32 - float64 restatement|; it is recomputed here.  The float32 restatement is one
more float32 evaluation of the same chain in another summation order, so it is held to the rule the device is held to: within 4 e_ref of
the float64 restatement (measured: 0.4 .. 1.1 e_ref), hence within 5 e_ref of the reference (measured: 0.9 .. 1.7 e_ref).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import plp_cases as P


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_restatement_matches_the_reference(name):
    ref, off, e_ref = P.golden_reference(name)
    want, keep = P.restated(name), P.compared(name)
    assert np.isfinite(ref).all() and ref.shape == want.shape and ref.shape[0] == off[-1] > 0
    assert (~keep).sum() <= P.EXCLUDE_FRACTION * keep.size and (P.case(name)[1] == "spectrogram" or keep.all())
    assert e_ref > 0.0 and abs(P.max_err(ref, name) - e_ref) <= 1e-6 * e_ref                 # the fixture's yardstick is reproducible
    w32 = P.restated(name, "f32")
    print("%s: e_ref %.3e, float32 restatement %.3e from float64, %.3e from the reference" % (
        name, e_ref, P.max_err(w32, name), np.abs(w32.astype(np.float64) - ref)[keep].max()))
    assert P.max_err(w32, name) <= 4.0 * e_ref
    assert np.abs(w32.astype(np.float64) - ref)[keep].max() <= 5.0 * e_ref


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_widths_and_frame_counts(name):
    from libs.amd import capi, frontend
    _, kind, kw, utts = P.case(name)
    ref, off, _ = P.golden_reference(name)
    opts, o = frontend.fbank_options(kind, **kw)
    assert frontend.feature_dim(kind, **kw) == ref.shape[1] == capi.lib().asv_fbank_dim(C.byref(opts))
    waves = P.golden_waves(name)
    assert [len(w) for w in waves] == [P.BANK_LEN[u] for u in utts] and all(w.dtype == np.int16 for w in waves)
    counts = [int(capi.lib().asv_fbank_num_frames(C.byref(opts), len(w))) for w in waves]
    assert counts == list(np.diff(off)) == list(frontend._frame_counts([len(w) for w in waves], o))
    if name == "plp-short-utterance":
        assert counts[utts.index("g")] == 0
    if name == "plp-one-frame":
        assert counts[utts.index("h")] == 1
    if name == "asvspoof-plp-40":
        assert counts[utts.index("b")] == 1


def test_dims_of_the_shipped_configurations():
    from libs.amd import frontend
    assert frontend.feature_dim("plp") == 13 and frontend.feature_dim("plp", lpc_order=19, num_ceps=20) == 20
    assert frontend.feature_dim("plp", lpc_order=39, num_ceps=40, num_mel_bins=160, frame_length=50.0) == 40
    assert frontend.feature_dim("spectrogram") == 257 and frontend.feature_dim("spectrogram", frame_length=50.0) == 513
    assert frontend.feature_dim("spectrogram", sample_frequency=8000.0) == 129
    assert frontend.feature_dim("fbank", num_mel_bins=40, use_energy=True) == 41 and frontend.feature_dim("mfcc", num_ceps=20) == 20
    assert callable(frontend.plp) and callable(frontend.spectrogram)


def test_python_refusals():
    from libs.amd import capi, frontend
    for kw, word in ((dict(lpc_order=0), "lpc_order"), (dict(lpc_order=capi.PLP_MAX_LPC_ORDER + 1, num_ceps=13), "lpc_order"),
                     (dict(lpc_order=12, num_ceps=14), "num_ceps"), (dict(num_ceps=0), "num_ceps"), (dict(compress_factor=0.0), "compress_factor"),
                     (dict(compress_factor=-0.5), "compress_factor"), (dict(dither=1.0), "dither")):
        with pytest.raises(ValueError, match=word):
            frontend.fbank_options("plp", **kw)
    frontend.fbank_options("plp", lpc_order=39, num_ceps=40)                  # asvspoof-plp-40.conf
    frontend.fbank_options("plp", lpc_order=capi.PLP_MAX_LPC_ORDER, num_ceps=capi.PLP_MAX_LPC_ORDER + 1)
    with pytest.raises(ValueError, match="return_raw_fft"):
        frontend.fbank_options("spectrogram", return_raw_fft=True)
    with pytest.raises(TypeError, match="num_mel_bins"):
        frontend.fbank_options("spectrogram", num_mel_bins=40)                 # a spectrogram has no mel options
    with pytest.raises(TypeError, match="lpc_order"):
        frontend.fbank_options("mfcc", lpc_order=12)
    with pytest.raises(ValueError, match="kind"):
        frontend.fbank_options("pitch")


def test_c_interface_refuses_before_touching_a_device():
    """Every refusal of asv_fbank for the new fields is decided from the options alone: the pointers below are never read."""
    from libs.amd import capi, frontend
    lib = capi.lib()
    off = np.array([0, 16000], dtype=np.int64)
    bogus = C.c_void_p(4096)

    def call(opts):
        rc = lib.asv_fbank(C.byref(opts), bogus, off.ctypes.data_as(C.POINTER(C.c_longlong)), 1, bogus, None)
        return rc, lib.asv_last_error().decode()

    def plp(**fields):
        opts, _ = frontend.fbank_options("plp")
        for k, v in fields.items():
            setattr(opts, k, v)
        return opts

    for opts, word in ((plp(lpc_order=-1), "lpc_order"), (plp(lpc_order=capi.PLP_MAX_LPC_ORDER + 1), "lpc_order"), (plp(num_ceps=14), "num_ceps"),
                       (plp(compress_factor=-1.0), "compress_factor"), (plp(return_raw_fft=1), "return_raw_fft"), (plp(feature_kind=7), "feature_kind"),
                       (plp(struct_size=capi.FBANK_OPTS_SIZE_V1 + 4), "struct_size")):
        rc, msg = call(opts)
        assert rc < 0 and word in msg, (rc, msg)
        assert lib.asv_fbank_dim(C.byref(opts)) == -1 or word == "compress_factor" or word == "return_raw_fft"
    spec, _ = frontend.fbank_options("spectrogram")
    spec.return_raw_fft = 1
    rc, msg = call(spec)
    assert rc < 0 and "return_raw_fft" in msg
    # a zero-filled tail asks for the reference's defaults; the old struct_size is feature_kind 0
    opts = plp(lpc_order=0, num_ceps=0, compress_factor=0.0, cepstral_scale=0.0)
    assert lib.asv_fbank_dim(C.byref(opts)) == 13
    old, _ = frontend.fbank_options("fbank", num_mel_bins=40, use_energy=True)
    old.struct_size = capi.FBANK_OPTS_SIZE_V1
    old.feature_kind = 2                                                        # beyond the size the caller declares: not read
    assert lib.asv_fbank_dim(C.byref(old)) == 41 and lib.asv_fbank_num_frames(C.byref(old), 16000) == 98


def test_kaldi_feature_kinds():
    from libs.egs.kaldi_features import KaldiFeature
    KaldiFeature("plp", {"lpc_order": 19, "num_ceps": 20, "low_freq": 40.0, "high_freq": -200.0})
    KaldiFeature("spectrogram", {"frame_shift": 4.0, "raw_energy": False})
    KaldiFeature("fbank", {"num_mel_bins": 40})
    with pytest.raises(ValueError, match="num_ceps"):
        KaldiFeature("plp", {"lpc_order": 12, "num_ceps": 20})
    with pytest.raises(AssertionError):
        KaldiFeature("pitch")


def test_header_and_ctypes_agree(tmp_path, repo_root):
    from libs.amd import capi, frontend
    src = tmp_path / "plp_abi.c"
    src.write_text(r'''#include <stdio.h>
#include <stddef.h>
#include "asv_amd.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %u\n", sizeof(asv_fbank_opts_t), offsetof(asv_fbank_opts_t, feature_kind), offsetof(asv_fbank_opts_t, lpc_order),
         offsetof(asv_fbank_opts_t, compress_factor), offsetof(asv_fbank_opts_t, cepstral_scale), offsetof(asv_fbank_opts_t, return_raw_fft), ASV_FBANK_OPTS_SIZE_V1);
  printf("%d %d %d %d\n", ASV_FEAT_FBANK, ASV_FEAT_SPECTROGRAM, ASV_FEAT_PLP, ASV_PLP_MAX_LPC_ORDER);
  return 0;
}''')
    exe = tmp_path / "plp_abi"
    subprocess.check_call(["gcc", "-I", os.path.join(repo_root, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    f = capi.FbankOpts
    assert [int(v) for v in lines[0].split()] == [C.sizeof(f), f.feature_kind.offset, f.lpc_order.offset, f.compress_factor.offset, f.cepstral_scale.offset,
                                                  f.return_raw_fft.offset, capi.FBANK_OPTS_SIZE_V1]
    assert f.feature_kind.offset == capi.FBANK_OPTS_SIZE_V1 == f.vtln_high.offset + 4          # the new fields are appended, nothing moved
    assert [int(v) for v in lines[1].split()] == [capi.FEATURE_KINDS["fbank"], capi.FEATURE_KINDS["spectrogram"], capi.FEATURE_KINDS["plp"], capi.PLP_MAX_LPC_ORDER]
    assert capi.FEATURE_KINDS["mfcc"] == capi.FEATURE_KINDS["fbank"] and capi.PLP_MAX_LPC_ORDER >= 39
    # the defaults the header documents are the ones the Python layer fills in
    hdr = open(os.path.join(repo_root, "include", "asv_amd.h")).read()
    doc = {m.group(1): m.group(2) for m in re.finditer(r"^\s*(?:int32_t|float)\s+(\w+);\s*/\*\s*([-0-9.]+)", hdr, re.M)}
    d = frontend._PLP_DEFAULTS
    assert float(doc["lpc_order"]) == d["lpc_order"] == 12 and float(doc["compress_factor"]) == d["compress_factor"] == 0.33333
    assert float(doc["cepstral_scale"]) == d["cepstral_scale"] == 1.0 and float(doc["return_raw_fft"]) == 0
    assert d["num_ceps"] == 13 and d["cepstral_lifter"] == float(doc["cepstral_lifter"]) == 22.0
    assert "asv_fbank_dim" in capi.SYMBOLS and re.search(r"int\s+asv_fbank_dim\(", hdr)
