# -*- coding:utf-8 -*-
"""Kaldi `.conf` files (`--some-key=value` lines, `#` comments) -> the keyword dicts of libs.amd.frontend, for makeFeatures.py and
computeVad.py.

A key the file omits takes the default of the Kaldi BINARY of that feature kind (compute-fbank-feats, compute-mfcc-feats, ...) - not
torchaudio's, which libs.amd.frontend's own defaults follow.  They are the initialisers of the option structs in the reference's
runtime/kaldifeat/csrc:
    feature-window.h:31-44       samp_freq 16000, frame_shift_ms 10, frame_length_ms 25, dither 1.0, preemph_coeff 0.97, remove_dc_offset true,
                                 window_type "povey", round_to_power_of_two true, blackman_coeff 0.42, snip_edges true
    mel-computations.h:18-35     num_bins 25 (every feature's constructor sets 23), low_freq 20, high_freq 0, vtln_low 100, vtln_high -500
    feature-fbank.h:23-43        use_energy false, energy_floor 0, raw_energy true, htk_compat false, use_log_fbank true, use_power true, num_bins 23
    feature-mfcc.h:27-52         num_ceps 13, use_energy TRUE, energy_floor 0, raw_energy true, cepstral_lifter 22, htk_compat false, num_bins 23
    feature-plp.h:32-60          lpc_order 12, num_ceps 13, use_energy true, energy_floor 0, raw_energy true, compress_factor 0.33333,
                                 cepstral_lifter 22, cepstral_scale 1, htk_compat false, num_bins 23
    feature-spectrogram.h:26-33  energy_floor 0, raw_energy true, return_raw_fft false
dither is the exception: Kaldi's default is 1.0 (random noise), which the device path does not offer - a file without the key is read as
dither 0 with one logged line saying so, and an explicit non-zero value is refused as libs.amd.frontend.fbank_options refuses it.
"""

import logging

log = logging.getLogger("asv_amd.kaldi_conf")

_FRAME = dict(sample_frequency=16000.0, frame_shift=10.0, frame_length=25.0, preemphasis_coefficient=0.97, remove_dc_offset=True,
              window_type="povey", round_to_power_of_two=True, blackman_coeff=0.42, snip_edges=True)
_MEL = dict(num_mel_bins=23, low_freq=20.0, high_freq=0.0, vtln_low=100.0, vtln_high=-500.0)

KALDI_DEFAULTS = {
    "fbank": dict(_FRAME, **dict(_MEL, use_energy=False, energy_floor=0.0, raw_energy=True, htk_compat=False, use_log_fbank=True, use_power=True)),
    "mfcc": dict(_FRAME, **dict(_MEL, num_ceps=13, use_energy=True, energy_floor=0.0, raw_energy=True, cepstral_lifter=22.0, htk_compat=False)),
    "plp": dict(_FRAME, **dict(_MEL, lpc_order=12, num_ceps=13, use_energy=True, energy_floor=0.0, raw_energy=True, compress_factor=0.33333,
                               cepstral_lifter=22.0, cepstral_scale=1.0, htk_compat=False)),
    "spectrogram": dict(_FRAME, energy_floor=0.0, raw_energy=True, return_raw_fft=False),
}

# compute-vad (Kaldi ivector/voice-activity-detection.h VadEnergyOptions) - NOT the 2 / 0.12 of the reference's C++ runtime that
# libs.amd.frontend.vad_energy defaults to
VAD_DEFAULTS = dict(vad_energy_threshold=5.0, vad_energy_mean_scale=0.5, vad_frames_context=0, vad_proportion_threshold=0.6)


def _typed(key, text, like):
    try:
        if isinstance(like, bool):
            if text.lower() not in ("true", "false", "t", "f", "1", "0"):
                raise ValueError(text)
            return text.lower() in ("true", "t", "1")
        if isinstance(like, int):
            return int(text)
        if isinstance(like, float):
            return float(text)
        return text
    except ValueError:
        raise ValueError("conf: --%s=%s is not a %s" % (key.replace("_", "-"), text, type(like).__name__))


def parse_conf(text):
    """[(key with '_' for '-', value text)] of the `--key=value` lines; anything else but blank lines and comments is an error."""
    out = []
    for no, line in enumerate(text.splitlines(), 1):
        line = line.split("#", 1)[0].strip()
        if not line:
            continue
        if not line.startswith("--") or "=" not in line:
            raise ValueError("conf line %d: expected --key=value, got %r" % (no, line))
        key, value = line[2:].split("=", 1)
        out.append((key.strip().replace("-", "_"), value.strip()))
    return out


def _read(conf):
    if "\n" in conf or conf.lstrip().startswith("--") or conf.strip() == "":
        return conf
    with open(conf, "r") as f:
        return f.read()


def read_feature_conf(conf, kind):
    """conf: a path, or the text itself.  Returns the full keyword dict for libs.amd.frontend of feature `kind`: the file's keys typed,
    the others at the Kaldi binary's defaults, dither 0."""
    if kind not in KALDI_DEFAULTS:
        raise ValueError("unknown feature kind %r (one of %s)" % (kind, sorted(KALDI_DEFAULTS)))
    defaults = dict(KALDI_DEFAULTS[kind], dither=0.0)
    out, seen = dict(defaults), set()
    for key, text in parse_conf(_read(conf)):
        if key not in defaults:
            raise ValueError("conf: unknown option --%s for %s features" % (key.replace("_", "-"), kind))
        out[key] = _typed(key, text, defaults[key])
        seen.add(key)
    if "dither" not in seen:
        log.warning("%s conf has no --dither: Kaldi's default 1.0 is random noise and is not applied on the device path (dither = 0)", kind)
    elif out["dither"] != 0.0:
        raise ValueError("fbank: dither is random noise and is not offered on the device path; set dither=0.0 (extraction configs do)")
    return out


def read_vad_conf(conf):
    """(energy threshold, mean scale, frames context, proportion threshold) with compute-vad's defaults for the keys left out."""
    out = dict(VAD_DEFAULTS)
    for key, text in parse_conf(_read(conf)):
        if key not in VAD_DEFAULTS:
            raise ValueError("conf: unknown option --%s for the energy VAD" % key.replace("_", "-"))
        out[key] = _typed(key, text, VAD_DEFAULTS[key])
    return out
