# -*- coding:utf-8 -*-
"""Acoustic front-end on the MI355X: Kaldi-compatible log-mel filterbank, MFCC, PLP and spectrogram features (+ per-utterance
mean/variance normalisation) of a batch of waveforms in one launch (PLP: two), through asv_fbank / asv_cmvn of libasv_amd.so.

Replaces the per-utterance torchaudio.compliance.kaldi.fbank loop of reference
pytorch/libs/egs/kaldi_features.py:107-137 (and kaldifeat::Fbank of runtime/kaldifeat/csrc); option names and defaults
below are torchaudio's, so a `kaldi_featset` dict of a reference config passes through unchanged.
"""

import ctypes as C

import numpy as np

from . import capi

# torchaudio.compliance.kaldi.fbank keyword -> (asv_fbank_opts_t field, default)
_DEFAULTS = dict(
    blackman_coeff=0.42, channel=-1, dither=0.0, energy_floor=1.0, frame_length=25.0, frame_shift=10.0, high_freq=0.0,
    htk_compat=False, low_freq=20.0, min_duration=0.0, num_mel_bins=23, preemphasis_coefficient=0.97, raw_energy=True,
    remove_dc_offset=True, round_to_power_of_two=True, sample_frequency=16000.0, snip_edges=True, subtract_mean=False,
    use_energy=False, use_log_fbank=True, use_power=True, vtln_high=-500.0, vtln_low=100.0, vtln_warp=1.0, window_type="povey")


# torchaudio.compliance.kaldi.mfcc: the same framing / mel options, no use_log_fbank / use_power, plus the cepstral ones
_MFCC_DEFAULTS = dict({k: v for k, v in _DEFAULTS.items() if k not in ("use_log_fbank", "use_power")}, num_ceps=13, cepstral_lifter=22.0)


# PLP (reference runtime/kaldifeat/csrc/feature-plp.h PlpOptions; torchaudio has no PLP): the framing / mel names of above, the
# cepstral ones of mfcc, plus lpc_order / compress_factor / cepstral_scale.  use_energy and energy_floor default as PlpOptions does.
_PLP_DEFAULTS = dict(_MFCC_DEFAULTS, use_energy=True, energy_floor=0.0, lpc_order=12, compress_factor=0.33333, cepstral_scale=1.0)

# torchaudio.compliance.kaldi.spectrogram (= feature-spectrogram.h SpectrogramOptions): framing options and the energy in column 0
_SPECTROGRAM_DEFAULTS = dict({k: _DEFAULTS[k] for k in (
    "blackman_coeff", "channel", "dither", "energy_floor", "frame_length", "frame_shift", "min_duration", "preemphasis_coefficient", "raw_energy",
    "remove_dc_offset", "round_to_power_of_two", "sample_frequency", "snip_edges", "subtract_mean", "window_type")}, return_raw_fft=False)

_KIND_DEFAULTS = {"fbank": _DEFAULTS, "mfcc": _MFCC_DEFAULTS, "plp": _PLP_DEFAULTS, "spectrogram": _SPECTROGRAM_DEFAULTS}


def _padded_window(o):
    length = int(np.float32(o["sample_frequency"]) * np.float32(0.001) * np.float32(o["frame_length"]))
    padded = 1
    while padded < length:
        padded *= 2
    return padded


def fbank_options(_kind="fbank", **kw):
    """A filled asv_fbank_opts_t from torchaudio-style keywords; refuses what the device path does not compute.
    _kind: "fbank", "mfcc", "plp" or "spectrogram"."""
    if _kind not in _KIND_DEFAULTS:
        raise ValueError("unknown feature kind %r (one of %s)" % (_kind, sorted(_KIND_DEFAULTS)))
    defaults = _KIND_DEFAULTS[_kind]
    unknown = set(kw) - set(defaults)
    if unknown:
        raise TypeError("%s: unknown option(s) %s" % (_kind, sorted(unknown)))
    o = dict(defaults, **kw)
    o.setdefault("use_log_fbank", True)
    o.setdefault("use_power", True)
    o.setdefault("num_ceps", 0)
    o.setdefault("cepstral_lifter", 0.0)
    for k in ("htk_compat", "use_energy", "vtln_high", "vtln_low", "vtln_warp", "low_freq", "high_freq", "num_mel_bins"):      # (spectrogram has none of these)
        o.setdefault(k, _DEFAULTS[k])
    o.setdefault("lpc_order", 0)
    o.setdefault("compress_factor", 0.0)
    o.setdefault("cepstral_scale", 0.0)
    o.setdefault("return_raw_fft", False)
    if _kind == "spectrogram":
        o["dim"] = _padded_window(o) // 2 + 1
    else:
        o["dim"] = o["num_ceps"] if _kind in ("mfcc", "plp") else o["num_mel_bins"] + int(o["use_energy"])
    if _kind == "mfcc" and not 1 <= o["num_ceps"] <= o["num_mel_bins"]:
        raise ValueError("mfcc: num_ceps %d must be in [1, num_mel_bins = %d]" % (o["num_ceps"], o["num_mel_bins"]))
    if _kind == "plp":
        if not 1 <= o["lpc_order"] <= capi.PLP_MAX_LPC_ORDER:
            raise ValueError("plp: lpc_order %d must be in [1, %d]" % (o["lpc_order"], capi.PLP_MAX_LPC_ORDER))
        if not 1 <= o["num_ceps"] <= o["lpc_order"] + 1:
            raise ValueError("plp: num_ceps %d must be in [1, lpc_order + 1 = %d]" % (o["num_ceps"], o["lpc_order"] + 1))
        if not o["compress_factor"] > 0.0:
            raise ValueError("plp: compress_factor %r must be positive" % (o["compress_factor"],))
        if o["cepstral_scale"] == 0.0:
            raise ValueError("plp: cepstral_scale 0 would zero every cepstrum (the C interface reads 0 as 'default 1')")
    if o["return_raw_fft"]:
        raise ValueError("spectrogram: return_raw_fft is not supported (the reference refuses it too)")
    if o["dither"] != 0.0:
        raise ValueError("fbank: dither is random noise and is not offered on the device path; set dither=0.0 (extraction configs do)")
    if o["window_type"] not in capi.WINDOW_TYPES:
        raise ValueError("fbank: unknown window_type %r" % (o["window_type"],))
    if o["channel"] not in (-1, 0):
        raise ValueError("fbank: pass one channel per utterance")
    opts = capi.FbankOpts()
    opts.struct_size = C.sizeof(capi.FbankOpts)
    opts.sample_rate = o["sample_frequency"]
    opts.frame_length_ms, opts.frame_shift_ms = o["frame_length"], o["frame_shift"]
    opts.preemph = o["preemphasis_coefficient"]
    opts.remove_dc_offset = int(o["remove_dc_offset"])
    opts.window_type = capi.WINDOW_TYPES[o["window_type"]]
    opts.round_to_power_of_two = int(o["round_to_power_of_two"])
    opts.snip_edges = int(o["snip_edges"])
    opts.num_bins = o["num_mel_bins"]
    opts.low_freq, opts.high_freq = o["low_freq"], o["high_freq"]
    opts.use_energy = int(o["use_energy"])
    opts.energy_floor = o["energy_floor"]
    opts.raw_energy = int(o["raw_energy"])
    opts.htk_compat = int(o["htk_compat"])
    opts.use_log_fbank = int(o["use_log_fbank"])
    opts.use_power = int(o["use_power"])
    opts.num_ceps = o["num_ceps"]
    opts.cepstral_lifter = o["cepstral_lifter"]
    opts.blackman_coeff = o["blackman_coeff"]
    opts.vtln_warp, opts.vtln_low, opts.vtln_high = o["vtln_warp"], o["vtln_low"], o["vtln_high"]
    opts.feature_kind = capi.FEATURE_KINDS[_kind]
    opts.lpc_order, opts.compress_factor, opts.cepstral_scale = o["lpc_order"], o["compress_factor"], o["cepstral_scale"]
    opts.return_raw_fft = int(o["return_raw_fft"])
    return opts, o


def mfcc_options(**kw):
    return fbank_options("mfcc", **kw)


def plp_options(**kw):
    return fbank_options("plp", **kw)


def spectrogram_options(**kw):
    return fbank_options("spectrogram", **kw)


def feature_dim(kind="fbank", **kw):
    """Columns of a feature row of `kind` under the options `kw`: num_mel_bins + use_energy (fbank), num_ceps (mfcc, plp),
    padded window / 2 + 1 (spectrogram) - what asv_fbank_dim answers for the same options block."""
    return int(fbank_options(kind, **kw)[1]["dim"])


def num_frames(num_samples, **kw):
    opts, _ = fbank_options("fbank", **kw)
    n = capi.lib().asv_fbank_num_frames(C.byref(opts), int(num_samples))
    if n < 0:
        raise capi.AsvError("asv_fbank_num_frames: bad options")
    return int(n)


def _frame_counts(lens, o):
    """asv_fbank_num_frames for an array of lengths (feature-window.cc:71-114), vectorised."""
    lens = np.asarray(lens, dtype=np.int64)
    length = int(np.float32(o["sample_frequency"]) * np.float32(0.001) * np.float32(o["frame_length"]))
    shift = int(np.float32(o["sample_frequency"]) * np.float32(0.001) * np.float32(o["frame_shift"]))
    if o["snip_edges"]:
        return np.where(lens < length, 0, 1 + (lens - length) // shift)
    return (lens + shift // 2) // shift


def fbank_device(wave, sample_off, mean_norm=False, std_norm=False, eps=1e-10, kind="fbank", **kw):
    """wave: 1-D f32 or int16 (16-bit PCM) CUDA tensor holding all utterances back to back, sample_off: int64 numpy [n+1].
    Returns (feats [sum frames, dim] f32 CUDA tensor, frame_offsets int64 numpy [n+1]).  kind="mfcc" / "plp": cepstra,
    "spectrogram": log power spectra."""
    import torch
    opts, o = fbank_options(kind, **kw)
    lib = capi.lib()
    sample_off = np.ascontiguousarray(sample_off, dtype=np.int64)
    n = len(sample_off) - 1
    if n < 1 or wave.dim() != 1 or wave.dtype not in (torch.float32, torch.int16) or not wave.is_cuda or not wave.is_contiguous() or int(sample_off[-1]) != wave.shape[0]:
        raise ValueError("fbank_device: wave must be a contiguous 1-D f32 / int16 CUDA tensor of sample_off[-1] samples")
    entry = lib.asv_fbank if wave.dtype == torch.float32 else lib.asv_fbank_pcm16
    frame_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(_frame_counts(np.diff(sample_off), o), out=frame_off[1:])
    dim = o["dim"]
    feats = torch.empty((int(frame_off[-1]), dim), dtype=torch.float32, device=wave.device)
    stream = C.c_void_p(torch.cuda.current_stream(wave.device).cuda_stream)
    with torch.cuda.device(wave.device):
        capi.check(entry(C.byref(opts), C.c_void_p(wave.data_ptr()), sample_off.ctypes.data_as(C.POINTER(C.c_longlong)),
                         n, C.c_void_p(feats.data_ptr()), stream), "asv_fbank")
        if (o["subtract_mean"] or mean_norm or std_norm) and feats.shape[0] > 0:
            capi.check(lib.asv_cmvn(C.c_void_p(feats.data_ptr()), frame_off.ctypes.data_as(C.POINTER(C.c_longlong)), n, dim,
                                    int(bool(o["subtract_mean"] or mean_norm)), int(bool(std_norm)), float(eps), stream), "asv_cmvn")
    return feats, frame_off


def de_silence_host(samples, sample_rate, win_len=0.1, min_eng=50):
    """The reference's waveform trimming (pytorch/libs/egs/signal_processing.py:13-55 de_silence as processor.py:149-175 de_sil calls
    it for --de-silence true) for one int16 utterance, in numpy: blocks of n = int(win_len * sample_rate) samples plus one tail block of
    the rest; a block of m samples is kept iff sum |s_i| > min_eng * m - the integer form of mean(|s / 32768|) > min_eng / 32768, which
    decides as the reference's float32 mean does while min_eng * m stays well below 2^24; the kept blocks in order.  An
    utterance in which no block survives is returned whole (processor.py:170-171; the threshold halving of lines 166-169 never changes
    what an utterance yields, and its carry-over to later utterances of a DataLoader worker is not reproduced).  Returns int16."""
    x = np.ascontiguousarray(samples)
    if x.dtype != np.int16 or x.ndim != 1:
        raise ValueError("de_silence: one 1-D int16 (16-bit PCM) utterance, got %s %s" % (x.dtype, x.shape))
    n = int(win_len * sample_rate)
    if n < 1:
        raise ValueError("de_silence: win_len %r at %r Hz is shorter than one sample" % (win_len, sample_rate))
    min_eng = float(min_eng)
    if not (np.isfinite(min_eng) and min_eng >= 0.0):
        raise ValueError("de_silence: min_eng %r" % (min_eng,))
    if len(x) == 0:
        return x
    starts = np.arange(0, len(x), n)
    sums = np.add.reduceat(np.abs(x.astype(np.int64)), starts)                 # |-32768| = 32768: not in 16 bits
    sizes = np.minimum(n, len(x) - starts)
    keep = sums.astype(np.float64) > min_eng * sizes.astype(np.float64)
    if not keep.any():
        return x
    return x[np.repeat(keep, sizes)]


def de_silence_device(wave, sample_off, sample_rate, win_len=0.1, min_eng=50):
    """de_silence_host for a packed batch of 16-bit PCM on the device (asv_desilence_pcm16), sample for sample.  wave: 1-D int16 CUDA
    tensor of sample_off[-1] samples, sample_off: int64 numpy [n+1] from 0.  Returns (wave_out - a view of the first out_off[-1] samples of
    a new tensor -, out_off int64 numpy [n+1]): the pair fbank_device takes.  The call waits for the stream once (the host needs the kept
    counts).  float32 waves are refused: the integer rule is what pins the parity with the reference."""
    import torch
    sample_off = _off(sample_off)
    n = len(sample_off) - 1
    if isinstance(wave, torch.Tensor) and wave.dtype != torch.int16:
        raise ValueError("de_silence_device: 16-bit PCM (int16) only, got %s" % (wave.dtype,))
    if n < 1 or not isinstance(wave, torch.Tensor) or wave.dim() != 1 or not wave.is_cuda or not wave.is_contiguous() or int(sample_off[-1]) != wave.shape[0]:
        raise ValueError("de_silence_device: wave must be a contiguous 1-D int16 CUDA tensor of sample_off[-1] samples")
    if int(sample_off[0]) != 0 or (np.diff(sample_off) < 0).any():
        raise ValueError("de_silence_device: sample_off must start at 0 and not decrease")
    win = int(win_len * sample_rate)                                             # signal_processing.py:38
    if win < 1:
        raise ValueError("de_silence_device: win_len %r at %r Hz is shorter than one sample" % (win_len, sample_rate))
    out = torch.empty_like(wave)
    out_off = np.zeros(n + 1, dtype=np.int64)
    if wave.shape[0] == 0:
        return out, out_off                                # no sample: no launch (an empty tensor has no address to hand over)
    with torch.cuda.device(wave.device):
        capi.check(capi.lib().asv_desilence_pcm16(C.c_void_p(wave.data_ptr()), _i64p(sample_off), n, win, float(min_eng), C.c_void_p(out.data_ptr()),
                                                  _i64p(out_off), C.c_void_p(torch.cuda.current_stream(wave.device).cuda_stream)), "asv_desilence_pcm16")
    return out[:int(out_off[-1])], out_off


def fbank_packed(waveforms, device=None, de_silence=None, kind="fbank", **kw):
    """waveforms: list of 1-D float arrays / tensors (host or device), samples in the int16 value range.
    Returns (feats [sum frames, dim] f32 CUDA tensor, frame_offsets int64 numpy [n+1]) - the packed layout
    asv_net_extract consumes, so features never visit the host.  de_silence: {"win_len": seconds, "min_eng": threshold} trims the
    (int16) waveforms on the device between the upload and the features (de_silence_device, at kw's sample_frequency); None: no trimming.
    kind: "fbank", "mfcc", "plp" or "spectrogram" (fbank_options)."""
    import torch
    if len(waveforms) == 0:
        raise ValueError("fbank: empty batch")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    for w in waveforms:
        if w.ndim != 1:
            raise ValueError("fbank: every waveform must be 1-D (one channel), got shape %s" % (tuple(w.shape),))
    sample_off = np.zeros(len(waveforms) + 1, dtype=np.int64)
    np.cumsum([int(w.shape[0]) for w in waveforms], out=sample_off[1:])
    pcm16 = all((w.dtype == torch.int16) if isinstance(w, torch.Tensor) else (np.asarray(w).dtype == np.int16) for w in waveforms)
    dt = torch.int16 if pcm16 else torch.float32                      # 16-bit PCM is shipped and read as it is (half the ingest)
    if all(isinstance(w, torch.Tensor) and w.is_cuda for w in waveforms):
        wave = torch.cat([w.to(dt) for w in waveforms]) if len(waveforms) > 1 else waveforms[0].to(dt).contiguous()
    else:
        host = torch.empty(int(sample_off[-1]), dtype=dt).pin_memory()
        hv = host.numpy()
        for w, a, b in zip(waveforms, sample_off[:-1], sample_off[1:]):
            hv[a:b] = w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else np.asarray(w)
        wave = host.to(dev, non_blocking=True)
    if de_silence is not None:
        unknown = set(de_silence) - {"win_len", "min_eng"}
        if unknown:
            raise TypeError("fbank: unknown de_silence option(s) %s" % sorted(unknown))
        wave, sample_off = de_silence_device(wave, sample_off, kw.get("sample_frequency", _DEFAULTS["sample_frequency"]), **de_silence)
    return fbank_device(wave, sample_off, kind=kind, **kw)


def fbank(waveforms, **kw):
    """List of per-utterance [frames, dim] CUDA tensors (views of one packed allocation)."""
    feats, off = fbank_packed(waveforms, **kw)
    return [feats[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]


def mfcc(waveforms, **kw):
    """torchaudio.compliance.kaldi.mfcc for a batch: list of [frames, num_ceps] CUDA tensors."""
    return fbank(waveforms, kind="mfcc", **kw)


def plp(waveforms, **kw):
    """Kaldi PLP features (kaldifeat::Plp of the reference's runtime) for a batch: list of [frames, num_ceps] CUDA tensors."""
    return fbank(waveforms, kind="plp", **kw)


def spectrogram(waveforms, **kw):
    """torchaudio.compliance.kaldi.spectrogram for a batch: list of [frames, padded window / 2 + 1] CUDA tensors, log energy in column 0."""
    return fbank(waveforms, kind="spectrogram", **kw)


def _off(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _i64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_longlong))


def cmvn_sliding(feats, frame_off, cmn_window=600, min_window=100, center=False, norm_vars=False):
    """Kaldi apply-cmvn-sliding on packed device features (defaults are Kaldi's; the reference's extraction pipeline uses
    cmn_window=300, center=True: extract_xvectors_for_pytorch.sh:105-118).  Returns a new tensor."""
    import torch
    frame_off = _off(frame_off)
    out = torch.empty_like(feats)
    with torch.cuda.device(feats.device):
        capi.check(capi.lib().asv_cmvn_sliding(C.c_void_p(feats.data_ptr()), C.c_void_p(out.data_ptr()), _i64p(frame_off), len(frame_off) - 1,
                                               feats.shape[1], int(cmn_window), int(min_window), int(center), int(norm_vars),
                                               C.c_void_p(torch.cuda.current_stream(feats.device).cuda_stream)), "asv_cmvn_sliding")
    return out


def vad_energy(feats, frame_off, vad_energy_threshold=5.0, vad_energy_mean_scale=0.5, vad_frames_context=2, vad_proportion_threshold=0.12):
    """Energy VAD on column 0 (defaults: VadEnergyOptions of runtime/extractor/torch_asv_extractor.h:24-27).
    Returns (voiced uint8 CUDA tensor [frames], voiced_counts int64 numpy [n])."""
    import torch
    frame_off = _off(frame_off)
    n = len(frame_off) - 1
    voiced = torch.empty(feats.shape[0], dtype=torch.uint8, device=feats.device)
    counts = np.zeros(n, dtype=np.int64)
    with torch.cuda.device(feats.device):
        capi.check(capi.lib().asv_vad_energy(C.c_void_p(feats.data_ptr()), _i64p(frame_off), n, feats.shape[1], float(vad_energy_threshold),
                                             float(vad_energy_mean_scale), int(vad_frames_context), float(vad_proportion_threshold),
                                             C.c_void_p(voiced.data_ptr()), _i64p(counts),
                                             C.c_void_p(torch.cuda.current_stream(feats.device).cuda_stream)), "asv_vad_energy")
    return voiced, counts


def select_voiced(feats, voiced, frame_off, counts):
    """select-voiced-frames: (kept rows packed [sum counts, dim], new offsets int64 [n+1])."""
    import torch
    frame_off = _off(frame_off)
    out_off = np.zeros(len(frame_off), dtype=np.int64)
    np.cumsum(counts, out=out_off[1:])
    out = torch.empty((int(out_off[-1]), feats.shape[1]), dtype=torch.float32, device=feats.device)
    with torch.cuda.device(feats.device):
        capi.check(capi.lib().asv_select_frames(C.c_void_p(feats.data_ptr()), C.c_void_p(voiced.data_ptr()), _i64p(frame_off), _i64p(out_off),
                                                len(frame_off) - 1, feats.shape[1], C.c_void_p(out.data_ptr()),
                                                C.c_void_p(torch.cuda.current_stream(feats.device).cuda_stream)), "asv_select_frames")
    return out, out_off


def kept_offsets(voiced, frame_off):
    """Host side of a selection: (kept frames per utterance int64 [n], their running sum int64 [n+1]) of host flags (any non-zero
    byte keeps its frame)."""
    frame_off = _off(frame_off)
    rows = np.diff(frame_off)
    counts = np.zeros(len(rows), dtype=np.int64)
    some = rows > 0
    if some.any():
        # (sums over [start, next start): empty utterances have no width, so the starts of the others still delimit their frames)
        kept = (np.asarray(voiced[int(frame_off[0]):int(frame_off[-1])]) != 0).view(np.uint8)
        counts[some] = np.add.reduceat(kept, frame_off[:-1][some] - frame_off[0], dtype=np.int64)
    kept_off = np.zeros(len(frame_off), dtype=np.int64)
    np.cumsum(counts, out=kept_off[1:])
    return counts, kept_off


def ingest(feats, frame_off, voiced=None, cmn_window=0, min_window=100, center=True, norm_vars=False, out=None, kept_off=None):
    """Raw packed device features -> the rows the extractor reads, in one launch (asv_ingest_frames): Kaldi apply-cmvn-sliding over all
    raw frames (cmn_window > 0; the defaults center=True, norm_vars=False are those of the reference's
    extract_xvectors_for_pytorch.sh:105-118), then select-voiced-frames (voiced: one flag per raw frame, non-zero = keep - a CUDA uint8
    tensor as vad_energy returns it, or a host array; None keeps every frame, and the result equals cmvn_sliding's bit for bit).
    cmn_window=0: selection only.  Returns (kept rows [sum kept, dim] f32 CUDA tensor - `out[:sum kept]` when `out` is given -, kept_off
    int64 numpy [n+1]).  The kept counts come from the host flags, or from one small device-to-host copy for device flags; `kept_off`
    hands them in where the caller has them already (no copy, no synchronisation)."""
    import torch
    frame_off = _off(frame_off)
    n = len(frame_off) - 1
    if feats.dim() != 2 or feats.dtype != torch.float32 or not feats.is_cuda or not feats.is_contiguous() or n < 1 or int(frame_off[-1]) != feats.shape[0]:
        raise ValueError("ingest: feats must be a contiguous [frame_off[-1], dim] f32 CUDA tensor")
    dev_flags = None
    if voiced is not None:
        if isinstance(voiced, torch.Tensor) and voiced.is_cuda:
            if voiced.dtype != torch.uint8 or voiced.dim() != 1 or voiced.shape[0] < feats.shape[0] or not voiced.is_contiguous():
                raise ValueError("ingest: voiced must hold one uint8 flag per raw frame")
            dev_flags = voiced
            if kept_off is None:
                run = torch.zeros(feats.shape[0] + 1, dtype=torch.int64, device=feats.device)
                torch.cumsum(voiced[:feats.shape[0]] != 0, 0, out=run[1:])
                kept_off = run[torch.from_numpy(frame_off).to(feats.device)].cpu().numpy()
        else:
            host = np.ascontiguousarray(voiced.numpy() if isinstance(voiced, torch.Tensor) else voiced).astype(np.uint8, copy=False)
            if host.ndim != 1 or host.shape[0] < feats.shape[0]:
                raise ValueError("ingest: voiced must hold one uint8 flag per raw frame")
            if kept_off is None:
                kept_off = kept_offsets(host, frame_off)[1]
            dev_flags = torch.from_numpy(host).to(feats.device)
        if dev_flags.dtype != torch.uint8 or dev_flags.dim() != 1 or dev_flags.shape[0] < feats.shape[0] or not dev_flags.is_contiguous():
            raise ValueError("ingest: voiced must hold one uint8 flag per raw frame")
    kept_off = frame_off if kept_off is None else _off(kept_off)
    if len(kept_off) != n + 1:
        raise ValueError("ingest: kept_off must have one entry per utterance plus one")
    rows = max(int(kept_off[-1]), 0)
    if out is None:
        out = torch.empty((rows, feats.shape[1]), dtype=torch.float32, device=feats.device)
    elif out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or out.dim() != 2 or out.shape[1] != feats.shape[1] or out.shape[0] < rows:
        raise ValueError("ingest: out must be a contiguous f32 CUDA tensor of at least [%d, %d]" % (rows, feats.shape[1]))
    if rows == 0 and bool((np.diff(kept_off) == 0).all()):
        return out[:0], kept_off                          # nothing is kept: no launch (an empty tensor has no address to hand over)
    with torch.cuda.device(feats.device):
        capi.check(capi.lib().asv_ingest_frames(C.c_void_p(feats.data_ptr()), C.c_void_p(dev_flags.data_ptr()) if dev_flags is not None else None,
                                                _i64p(frame_off), _i64p(kept_off), n, feats.shape[1], int(cmn_window), int(min_window), int(bool(center)),
                                                int(bool(norm_vars)), C.c_void_p(out.data_ptr()),
                                                C.c_void_p(torch.cuda.current_stream(feats.device).cuda_stream)), "asv_ingest_frames")
    return out[:rows], kept_off


def ingest_windows(feats, win_start, win_len, cmn_window=0, min_window=100, center=True, norm_vars=False, out=None):
    """Windows of rows that lie on the device -> the rows the extractor reads, in one launch (asv_ingest_windows): window w is rows
    [win_start[w], win_start[w] + win_len[w]) of `feats` ([rows, dim] f32 CUDA tensor: one parent matrix or several, packed) and an
    utterance of its own for Kaldi's apply-cmvn-sliding - what the reference's sliding (diarisation) mode computes through range-specified
    scp entries.  Windows may overlap, repeat and come in any order; an empty one writes nothing.  cmn_window=0: the rows are copied as
    they are.  Returns (rows [sum win_len, dim] f32 CUDA tensor - `out[:sum win_len]` when `out` is given -, offsets int64 numpy [n + 1] of
    the windows in it); bit for bit what ingest() gives for a packed copy of the windows."""
    import torch
    win_start, win_len = _off(win_start), _off(win_len)
    n = len(win_start)
    if feats.dim() != 2 or feats.dtype != torch.float32 or not feats.is_cuda or not feats.is_contiguous():
        raise ValueError("ingest_windows: feats must be a contiguous [rows, dim] f32 CUDA tensor")
    if n < 1 or win_start.ndim != 1 or win_len.shape != win_start.shape:
        raise ValueError("ingest_windows: one start and one length per window, at least one window")
    if (win_start < 0).any() or (win_len < 0).any() or (win_start + win_len > feats.shape[0]).any():
        raise ValueError("ingest_windows: a window lies outside the %d rows of feats" % feats.shape[0])
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(win_len, out=offsets[1:])
    rows = int(offsets[-1])
    if out is None:
        out = torch.empty((rows, feats.shape[1]), dtype=torch.float32, device=feats.device)
    elif out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or out.dim() != 2 or out.shape[1] != feats.shape[1] or out.shape[0] < rows:
        raise ValueError("ingest_windows: out must be a contiguous f32 CUDA tensor of at least [%d, %d]" % (rows, feats.shape[1]))
    if rows == 0:
        return out[:0], offsets                            # nothing but empty windows: no launch (an empty tensor has no address to hand over)
    with torch.cuda.device(feats.device):
        capi.check(capi.lib().asv_ingest_windows(C.c_void_p(feats.data_ptr()), feats.shape[0], _i64p(win_start), _i64p(win_len), n, feats.shape[1],
                                                 int(cmn_window), int(min_window), int(bool(center)), int(bool(norm_vars)), C.c_void_p(out.data_ptr()),
                                                 C.c_void_p(torch.cuda.current_stream(feats.device).cuda_stream)), "asv_ingest_windows")
    return out[:rows], offsets


COMPRESSED_FORMATS = {"CM ": 1, "CM2": 2, "CM3": 3}          # Kaldi's token -> the format byte of asv_decode_compressed


def compressed_body_bytes(fmt, rows, cols):
    """Bytes of the body of a Kaldi compressed matrix (from its 16-byte global header to its end); numbers or arrays."""
    fmt, data = np.asarray(fmt), np.asarray(rows, dtype=np.int64) * np.asarray(cols, dtype=np.int64)
    return 16 + np.where(fmt == 1, 8 * np.asarray(cols, dtype=np.int64) + data, np.where(fmt == 2, 2 * data, data))


def decode_compressed(bytes_dev, byte_off, frame_off, formats, dim, out=None):
    """The bodies of Kaldi compressed matrices ('CM ' / 'CM2' / 'CM3', each from its 16-byte global header, as they lie on disk) in a
    uint8 CUDA tensor -> packed float32 rows, in one launch on the current stream (asv_decode_compressed); bit for bit what
    libs.support.kaldi_io.read_mat gives for the same bytes.  byte_off int64 [n]: start of each body in bytes_dev, multiples of 16;
    frame_off int64 [n + 1] from 0; formats uint8 [n] (COMPRESSED_FORMATS).  The rows and columns used are those of frame_off and dim -
    whoever filled the bytes has compared them with the headers (ScpBatchLoader.load_compressed does); here every body only has to lie
    inside bytes_dev.  Returns `out[:frame_off[-1]]` ([rows, dim] f32 CUDA tensor; allocated when not given)."""
    import torch
    byte_off, frame_off = _off(byte_off), _off(frame_off)
    formats = np.ascontiguousarray(formats, dtype=np.uint8)
    n = len(frame_off) - 1
    dim = int(dim)
    if bytes_dev.dim() != 1 or bytes_dev.dtype != torch.uint8 or not bytes_dev.is_cuda or not bytes_dev.is_contiguous():
        raise ValueError("decode_compressed: bytes_dev must be a contiguous 1-D uint8 CUDA tensor")
    if n < 1 or len(byte_off) != n or len(formats) != n or dim < 1:
        raise ValueError("decode_compressed: one byte offset and one format per utterance, frame_off with one entry more, dim >= 1")
    if bytes_dev.data_ptr() % 16:
        raise ValueError("decode_compressed: bytes_dev must start at a 16-byte boundary")
    rows_of = np.diff(frame_off)
    if int(frame_off[0]) != 0 or (rows_of < 0).any():
        raise ValueError("decode_compressed: frame_off must start at 0 and not decrease")
    if not np.isin(formats, (1, 2, 3)).all():
        raise ValueError("decode_compressed: formats are 1 ('CM '), 2 ('CM2') or 3 ('CM3')")
    ends = byte_off + compressed_body_bytes(formats, rows_of, dim)
    if (byte_off < 0).any() or (ends > bytes_dev.shape[0]).any():
        raise ValueError("decode_compressed: a body reaches beyond the %d bytes handed over" % bytes_dev.shape[0])
    rows = int(frame_off[-1])
    if out is None:
        out = torch.empty((rows, dim), dtype=torch.float32, device=bytes_dev.device)
    elif out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or out.dim() != 2 or out.shape[1] != dim or out.shape[0] < rows:
        raise ValueError("decode_compressed: out must be a contiguous f32 CUDA tensor of at least [%d, %d]" % (rows, dim))
    if rows == 0:
        return out[:0]
    with torch.cuda.device(bytes_dev.device):
        capi.check(capi.lib().asv_decode_compressed(C.c_void_p(bytes_dev.data_ptr()), _i64p(byte_off), _i64p(frame_off),
                                                    formats.ctypes.data_as(C.POINTER(C.c_ubyte)), n, dim, C.c_void_p(out.data_ptr()),
                                                    C.c_void_p(torch.cuda.current_stream(bytes_dev.device).cuda_stream)), "asv_decode_compressed")
    return out[:rows]


def compressed_auto_format(rows):
    """Kaldi's automatic compression method (what copy-feats --compress=true uses): more than 8 rows -> 'CM ' (1), otherwise 'CM2' (2)."""
    return np.where(np.asarray(rows) > 8, 1, 2).astype(np.uint8)


def encode_compressed(feats, frame_off, out=None, formats=None):
    """Packed float32 rows on the device -> the bodies of Kaldi compressed matrices, as they lie on disk behind the token, in three
    launches on the current stream (asv_encode_compressed).  feats: contiguous [frame_off[-1], dim] f32 CUDA tensor;
    frame_off: int64 [n + 1] from 0, every utterance at least one row.  The format of each utterance is Kaldi's automatic choice
    (compressed_auto_format; `formats` overrides it, 1 / 2 per utterance) and the bodies are laid out one behind the other, each at a
    16-byte boundary of `out` (a contiguous 1-D uint8 CUDA tensor that starts at one; allocated when not given - only the bodies are
    written, the padding bytes between them keep what they held).  Returns (bytes uint8 CUDA tensor, byte_off int64 [n], formats
    uint8 [n], status int32 CUDA tensor [n]: 0 = ok, 1 = the utterance holds a NaN or an infinity and its body is unspecified).  Body u
    is bytes[byte_off[u] : byte_off[u] + compressed_body_bytes(formats[u], rows[u], dim)]; no synchronisation in here."""
    import torch
    frame_off = _off(frame_off)
    n = len(frame_off) - 1
    if feats.dim() != 2 or feats.dtype != torch.float32 or not feats.is_cuda or not feats.is_contiguous() or n < 1 or int(frame_off[-1]) != feats.shape[0]:
        raise ValueError("encode_compressed: feats must be a contiguous [frame_off[-1], dim] f32 CUDA tensor")
    rows_of = np.diff(frame_off)
    if int(frame_off[0]) != 0 or (rows_of < 1).any():
        raise ValueError("encode_compressed: frame_off must start at 0 and increase (an empty matrix has no compressed form)")
    dim = int(feats.shape[1])
    if dim < 1:
        raise ValueError("encode_compressed: dim %d" % dim)
    formats = compressed_auto_format(rows_of) if formats is None else np.ascontiguousarray(formats, dtype=np.uint8)
    if len(formats) != n or not np.isin(formats, (1, 2)).all():
        raise ValueError("encode_compressed: one format per utterance, 1 ('CM ') or 2 ('CM2')")
    sizes = (compressed_body_bytes(formats, rows_of, dim) + 15) // 16 * 16
    byte_off = np.zeros(n, dtype=np.int64)
    np.cumsum(sizes[:-1], out=byte_off[1:])
    total = int(byte_off[-1] + sizes[-1])
    if out is None:
        out = torch.empty(total, dtype=torch.uint8, device=feats.device)
    elif out.dim() != 1 or out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.shape[0] < total or out.data_ptr() % 16:
        raise ValueError("encode_compressed: out must be a contiguous 1-D uint8 CUDA tensor of at least %d bytes at a 16-byte boundary" % total)
    status = torch.empty(n, dtype=torch.int32, device=feats.device)
    with torch.cuda.device(feats.device):
        capi.check(capi.lib().asv_encode_compressed(C.c_void_p(feats.data_ptr()), _i64p(frame_off), _i64p(byte_off), formats.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                                    n, dim, C.c_void_p(out.data_ptr()), C.c_void_p(status.data_ptr()),
                                                    C.c_void_p(torch.cuda.current_stream(feats.device).cuda_stream)), "asv_encode_compressed")
    return out[:total], byte_off, formats, status


def read_wav_pcm16(path):
    """(int16 samples of channel 0, sample rate).  16-bit PCM only - anything else is an error, not a silent conversion."""
    import wave
    with wave.open(path, "rb") as f:
        if f.getsampwidth() != 2 or f.getcomptype() != "NONE":
            raise ValueError("%s: only 16-bit PCM WAV is supported (sample width %d, %s)" % (path, f.getsampwidth(), f.getcomptype()))
        ch, sr, n = f.getnchannels(), f.getframerate(), f.getnframes()
        data = np.frombuffer(f.readframes(n), dtype="<i2")
    return (data.reshape(-1, ch)[:, 0] if ch > 1 else data), sr
