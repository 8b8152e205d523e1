"""PLP and spectrogram features: the test cases and a numpy restatement of the reference's code (runtime/kaldifeat/csrc:
feature-plp.cc:80-183, feature-spectrogram.cc:22-64, mel-computations.cc:203-349, feature-functions.cc:13-31), in float64 and in
float32.  Shared by tests/gen_plp_golden.py (which writes tests/golden/plp_spectrogram.npz from the reference's own code),
tests/test_plp_host.py and tests/test_gpu_plp.py.

The tables (window, mel filters, equal loudness, IDFT bases, lifter) are built in the reference's float arithmetic in both
precisions: they are constants of the computation, not part of its rounding error.  Everything behind them runs in `dtype`.
In float32 the statements of Durbin's recursion and of Lpc2Cepstrum follow the reference one by one (numpy rounds every
operation on its own), including the double inner sum of the latter; only the FFT is numpy's float64 one, rounded afterwards.

Option names are torchaudio's (libs.amd.frontend); a case is (name, kind, options, utterances of the wave bank).
"""
import functools
import json
import os

import numpy as np

from oracle import fbank_oracle as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plp_spectrogram.npz")
FLT_EPS = np.float32(1.1920928955078125e-07)

# ---- the wave bank: noise plus tones (no silent or constant frame: the reference's Durbin gives 0 / 0 there), int16 --------
# 16 kHz: 0.6 s, 0.05 s, an odd length, 0.2 s, 0.4 s, an odd length; "g" is shorter than a 25 ms window, "h" exactly one.
BANK_LEN = {"a": 9600, "b": 800, "c": 4967, "d": 3200, "e": 6400, "f": 2011, "g": 300, "h": 400,
            "p": 4800, "q": 400, "r": 2000, "s": 1601}          # p .. s: the 8 kHz utterances (0.6 s, 0.05 s, two odd ones)


def make_bank(seed=20240611):
    rng = np.random.RandomState(seed)
    bank = {}
    for i, (name, n) in enumerate(sorted(BANK_LEN.items())):
        rate = 8000.0 if name in "pqrs" else 16000.0
        t = np.arange(n) / rate
        x = 1500.0 * rng.standard_normal(n)
        for k in range(3):
            x += rng.uniform(500.0, 3000.0) * np.sin(2.0 * np.pi * rng.uniform(80.0, 0.45 * rate) * t + rng.uniform(0.0, 6.28))
        x += 300.0 * (i - 5)                                      # a DC offset of its own (remove_dc_offset has something to remove)
        bank[name] = np.clip(np.round(x), -32000, 32000).astype(np.int16)
    return bank


_SRE = dict(num_mel_bins=23, lpc_order=19, num_ceps=20, low_freq=40.0, high_freq=-200.0)
CASES = [
    # the three configurations the reference ships (conf/sre-plp-20.conf, asvspoof-plp-40.conf, asvspoof-spectrogram.conf)
    ("sre-plp-20", "plp", dict(_SRE), "abcdf"),
    ("asvspoof-plp-40", "plp", dict(use_energy=False, frame_length=50.0, frame_shift=4.0, low_freq=0.0, high_freq=0.0, num_mel_bins=160,
                                    lpc_order=39, num_ceps=40, remove_dc_offset=False), "dbfc"),          # 1024-point frames; "b" is exactly one
    ("asvspoof-spectrogram", "spectrogram", dict(frame_length=25.0, frame_shift=4.0, raw_energy=False, remove_dc_offset=False, energy_floor=0.0), "dbfh"),
    ("plp-defaults", "plp", dict(), "abcde"),                                                               # order 12, 13 cepstra
    ("plp-8k", "plp", dict(sample_frequency=8000.0, num_mel_bins=15, lpc_order=12, num_ceps=13), "pqrs"),   # 200 samples -> 256 points
    ("spectrogram-8k", "spectrogram", dict(sample_frequency=8000.0, energy_floor=0.0), "pqrs"),
    ("plp-no-snip", "plp", dict(_SRE, snip_edges=False), "abcdf"),
    ("spectrogram-no-snip", "spectrogram", dict(snip_edges=False, frame_shift=10.0, energy_floor=3.0e9), "bfhd"),   # a floor above some frames' energy
    ("plp-htk", "plp", dict(_SRE, htk_compat=True), "abcdf"),
    ("plp-htk-c0", "plp", dict(_SRE, htk_compat=True, use_energy=False), "bcdf"),
    ("plp-no-lifter", "plp", dict(_SRE, cepstral_lifter=0.0), "abcdf"),
    ("plp-scale", "plp", dict(_SRE, cepstral_scale=0.5), "abcdf"),
    ("plp-windowed-energy", "plp", dict(_SRE, raw_energy=False), "abcdf"),
    ("plp-energy-floor", "plp", dict(_SRE, energy_floor=3.0e9), "abcdf"),
    ("plp-fewer-ceps", "plp", dict(_SRE, num_ceps=8, use_energy=False, window_type="hamming", preemphasis_coefficient=0.0), "abcdf"),
    ("plp-vtln", "plp", dict(_SRE, vtln_warp=1.1), "bcdf"),
    ("plp-short-utterance", "plp", dict(), "cgdbf"),                                                        # "g": no frame at all
    ("plp-one-frame", "plp", dict(), "hcdbf"),                                                              # "h": exactly one frame, first
]
CASE_NAMES = [c[0] for c in CASES]
EXCLUDE_FRACTION = 0.005          # of a spectrogram case's values: the emptiest bins (cancellation), by the float64 restatement


def case(name):
    return CASES[CASE_NAMES.index(name)]


def full_options(kind, kw):
    from libs.amd import frontend
    return frontend.fbank_options(kind, **kw)[1]


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _windowed_frames(wave, o, dtype):
    """feature-window.cc / feature-common-inl.h: [frames, padded] windowed frames and the raw log energies (before pre-emphasis)."""
    sr, length = o["sample_frequency"], F.window_size(o["sample_frequency"], o["frame_length"])
    shift = F.window_size(sr, o["frame_shift"])
    wave = np.asarray(wave, dtype=np.float32)
    n = F.num_frames(len(wave), sr, o["frame_length"], o["frame_shift"], o["snip_edges"])
    padded = F.padded_size(length, o["round_to_power_of_two"])
    if n == 0:
        return np.zeros((0, padded), dtype=dtype), np.zeros(0, dtype=dtype)
    if not o["snip_edges"]:
        pad = (n - 1) * shift + length - len(wave)
        left = (length - shift) // 2
        right = pad - left
        wave = np.concatenate([wave[:left][::-1], wave, wave[len(wave) - right:][::-1] if right > 0 else wave[:0]])
    frames = wave[np.arange(n)[:, None] * shift + np.arange(length)[None, :]].astype(dtype)
    if o["remove_dc_offset"]:
        frames = frames - frames.mean(axis=1, keepdims=True, dtype=dtype)
    raw = np.log(np.maximum((frames * frames).sum(axis=1, dtype=dtype), FLT_EPS))
    pre = o["preemphasis_coefficient"]
    if pre != 0.0:
        out = np.empty_like(frames)
        out[:, 1:] = frames[:, 1:] - dtype(pre) * frames[:, :-1]
        out[:, 0] = frames[:, 0] - dtype(pre) * frames[:, 0]
        frames = out
    frames = frames * F.window_function(length, o["window_type"], o["blackman_coeff"]).astype(dtype)[None, :]
    if padded > length:
        frames = np.concatenate([frames, np.zeros((n, padded - length), dtype=dtype)], axis=1)
    return frames, raw


def _log_energy(frames, raw, o, dtype):
    e = raw if o["raw_energy"] else np.log(np.maximum((frames * frames).sum(axis=1, dtype=dtype), FLT_EPS))
    if o["energy_floor"] > 0.0:
        e = np.maximum(e, dtype(np.log(np.float32(o["energy_floor"]))))
    return e


def _power(frames, dtype):
    return (np.abs(np.fft.rfft(frames.astype(np.float64), axis=1)) ** 2).astype(dtype)


def spectrogram(wave, o, dtype=np.float64):
    frames, raw = _windowed_frames(wave, o, dtype)
    out = np.log(np.maximum(_power(frames, dtype), dtype(FLT_EPS)))
    out[:, 0] = _log_energy(frames, raw, o, dtype)
    return out


def centre_freqs(o, padded):
    """InverseMelScale of the (warped) bin centres, mel-computations.cc:149-162, float."""
    nyquist = np.float32(0.5 * o["sample_frequency"])
    high = np.float32(o["high_freq"]) if o["high_freq"] > 0.0 else np.float32(nyquist + np.float32(o["high_freq"]))
    vt_high = o["vtln_high"] + float(nyquist) if o["vtln_high"] < 0.0 else o["vtln_high"]
    mel_low, mel_high = F.mel_scale(o["low_freq"]), F.mel_scale(high)
    delta = np.float32((mel_high - mel_low) / np.float32(o["num_mel_bins"] + 1))
    out = np.empty(o["num_mel_bins"], dtype=np.float32)
    for b in range(o["num_mel_bins"]):
        m = np.float32(mel_low + np.float32(b + 1) * delta)
        if o["vtln_warp"] != 1.0:
            m = F.mel_scale(F.vtln_warp_freq(o["vtln_low"], vt_high, o["low_freq"], high, o["vtln_warp"], F.inverse_mel_scale(m)))
        out[b] = F.inverse_mel_scale(m)
    return out


def equal_loudness(f0):
    """GetEqualLoudnessVector, mel-computations.cc:214-227: float squares, double sums, float results."""
    fsq = (f0 * f0).astype(np.float32)
    fsub = (fsq.astype(np.float64) / (fsq.astype(np.float64) + 1.6e5)).astype(np.float32)
    return ((fsub * fsub).astype(np.float64) * ((fsq.astype(np.float64) + 1.44e6) / (fsq.astype(np.float64) + 9.61e6))).astype(np.float32)


def idft_bases(n_bases, dimension):
    """InitIdftBases, feature-functions.cc:13-31: [n_bases, dimension], float angle and float cosine."""
    angle = np.float32(np.pi / (dimension - 1))
    scale = np.float32(1.0) / np.float32(2 * (dimension - 1))
    i = np.arange(n_bases, dtype=np.float32)[:, None]
    j = np.arange(dimension, dtype=np.float32)[None, :]
    cosf = lambda x: np.cos(x.astype(np.float64)).astype(np.float32)          # the C library's cosf: correctly rounded but for rare cases
    out = (np.float32(2.0) * scale * cosf((angle * i) * j)).astype(np.float32)
    out[:, 0] = scale
    out[:, -1] = scale * cosf((angle * i[:, 0]) * np.float32(dimension - 1))
    return out


def durbin(ac, dtype):
    """Durbin, mel-computations.cc:235-266, for all frames at once: ac [frames, n + 1] -> (lpc [frames, n], E [frames])."""
    n = ac.shape[1] - 1
    lp = np.zeros((ac.shape[0], n), dtype=dtype)
    e = ac[:, 0].copy()
    floor = dtype(1.0e-5)
    for i in range(n):
        ki = ac[:, i + 1].copy()
        for j in range(i):
            ki = ki + lp[:, j] * ac[:, i - j]
        ki = ki / e
        c = dtype(1.0) - ki * ki
        c = np.where(c.astype(np.float64) < 1.0e-5, floor, c)
        e = e * c
        tmp = lp.copy()
        tmp[:, i] = -ki
        for j in range(i):
            tmp[:, j] = lp[:, j] - ki * lp[:, i - j - 1]
        lp = tmp
    return lp, e


def lpc_to_cepstrum(lp, dtype):
    """Lpc2CepstrumInternal, mel-computations.cc:313-321: products in `dtype`, the sum in double."""
    n = lp.shape[1]
    cep = np.zeros_like(lp)
    for i in range(n):
        s = np.zeros(lp.shape[0], dtype=np.float64)
        for j in range(i):
            s = s + ((dtype(i - j) * lp[:, j]) * cep[:, i - j - 1]).astype(np.float64)
        cep[:, i] = (-lp[:, i].astype(np.float64) - s / (i + 1)).astype(dtype)
    return cep


def plp(wave, o, dtype=np.float64):
    frames, raw = _windowed_frames(wave, o, dtype)
    padded = frames.shape[1]
    nb, order, nc = o["num_mel_bins"], o["lpc_order"], o["num_ceps"]
    banks = F.mel_banks(nb, padded, o["sample_frequency"], o["low_freq"], o["high_freq"], o["vtln_warp"], o["vtln_low"], o["vtln_high"])
    mel = _power(frames, dtype)[:, :-1] @ banks.astype(dtype)
    mel = mel * equal_loudness(centre_freqs(o, padded)).astype(dtype)[None, :]
    mel = np.power(mel, dtype(np.float32(o["compress_factor"])))
    mel = np.concatenate([mel[:, :1], mel, mel[:, -1:]], axis=1)
    ac = mel @ idft_bases(order + 1, nb + 2).astype(dtype).T
    lp, e = durbin(ac, dtype)
    if dtype == np.float32:
        c0 = -np.log((1.0 / e.astype(np.float64)).astype(np.float32))
    else:
        c0 = -np.log(1.0 / e)
    c0 = np.maximum(c0, dtype(FLT_EPS))
    feats = np.concatenate([c0[:, None], lpc_to_cepstrum(lp, dtype)[:, :nc - 1]], axis=1).astype(dtype)
    if o["cepstral_lifter"] != 0.0:
        feats = feats * F.lifter_coeffs(float(np.float32(o["cepstral_lifter"])), nc).astype(dtype)[None, :]
    if o["cepstral_scale"] != 1.0:
        feats = feats * dtype(np.float32(o["cepstral_scale"]))
    if o["use_energy"]:
        feats[:, 0] = _log_energy(frames, raw, o, dtype)
    if o["htk_compat"]:
        feats = np.roll(feats, -1, axis=1)
    return feats


def restate(kind, wave, o, dtype=np.float64):
    return (plp if kind == "plp" else spectrogram)(wave, o, dtype)


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def golden_waves(name):
    """The case's int16 utterances, in order."""
    g = golden()
    return [g["wave_" + u] for u in case(name)[3]]


def golden_reference(name):
    """(reference float32 rows of all utterances back to back, frame offsets, e_ref)."""
    g = golden()
    return g["ref_" + name], g["off_" + name], float(g["eref_" + name])


@functools.lru_cache(maxsize=None)
def restated(name, precision="f64"):
    """The restatement of a whole case (rows back to back), computed once per process; callers must not write into it."""
    _, kind, kw, _ = case(name)
    o = full_options(kind, kw)
    dtype = np.float64 if precision == "f64" else np.float32
    out = np.concatenate([restate(kind, w.astype(np.float32), o, dtype) for w in golden_waves(name)], axis=0)
    out.setflags(write=False)
    return out


def mask_of(kind, want):
    """Boolean mask of the values a comparison covers: everything, but for a spectrogram not the emptiest EXCLUDE_FRACTION of the
    values (by the float64 restatement `want` of the whole case; column 0, the energy, always stays)."""
    keep = np.ones(want.shape, dtype=bool)
    k = int(EXCLUDE_FRACTION * want.size)
    if kind == "spectrogram" and k > 0:
        body = want[:, 1:]
        keep[:, 1:] = body > np.partition(body.ravel(), k - 1)[k - 1]
        assert (~keep).sum() <= EXCLUDE_FRACTION * want.size
    return keep


@functools.lru_cache(maxsize=None)
def compared(name):
    keep = mask_of(case(name)[1], restated(name))
    keep.setflags(write=False)
    return keep


def max_err(got, name):
    """max |got - float64 restatement| over the compared values of the case."""
    want, keep = restated(name), compared(name)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got.astype(np.float64) - want)[keep].max()) if keep.any() else 0.0


def options_json(name):
    _, kind, kw, utts = case(name)
    return json.dumps({"kind": kind, "options": kw, "utterances": utts}, sort_keys=True)
