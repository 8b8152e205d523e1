#!/usr/bin/env python3
"""Front-end throughput: asv_fbank (+ asv_cmvn) over a batch of synthetic waveforms resident in HBM.
    python tools/bench_fbank.py [--utts 512] [--seconds 2.0] [--bins 80] [--iters 50]
Prints one JSON line: frames/s, x real time, algorithmic HBM GB/s (4 B/sample in + 4*dim B/frame out).
    python tools/bench_fbank.py --kind plp|spectrogram [--out profiles/plp_ab.txt]
measures the configurations the reference ships for that kind (sre-plp-20 and asvspoof-plp-40, or asvspoof-spectrogram) next to the
80-bin filterbank in the same run, no CMN: one JSON line each (frames/s; for PLP also the share of the device time that
plp_lpc_kernel, the lane-per-frame stage, takes, from the profiler's kernel records), appended to --out when given."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "asv-subtools_amd", "pytorch")]


KIND_CONFIGS = {
    "plp": [("sre-plp-20", "plp", dict(num_mel_bins=23, lpc_order=19, num_ceps=20, low_freq=40.0, high_freq=-200.0)),
            ("asvspoof-plp-40", "plp", dict(use_energy=False, frame_length=50.0, frame_shift=4.0, low_freq=0.0, high_freq=0.0, num_mel_bins=160, lpc_order=39,
                                            num_ceps=40, remove_dc_offset=False))],
    "spectrogram": [("asvspoof-spectrogram", "spectrogram", dict(frame_length=25.0, frame_shift=4.0, raw_energy=False, remove_dc_offset=False, energy_floor=0.0))],
}


def bench_kinds(a):
    """The shipped configurations of a.kind and the filterbank, interleaved rounds of a.iters calls each, the median round per configuration."""
    import torch
    from libs.amd import frontend, synth
    n = int(a.seconds * 16000)
    base = [torch.from_numpy(synth.synth_wave(n, 900 + i)).cuda() for i in range(8)]
    wave = torch.cat([base[i % 8] for i in range(a.utts)])
    soff = np.arange(a.utts + 1, dtype=np.int64) * n
    configs = [("fbank-%d" % a.bins, "fbank", dict(num_mel_bins=a.bins))] + KIND_CONFIGS[a.kind]
    run = lambda kind, kw: frontend.fbank_device(wave, soff, kind=kind, **kw)
    frames, times = {}, {name: [] for name, _, _ in configs}
    for name, kind, kw in configs:
        for _ in range(10):
            frames[name] = int(run(kind, kw)[1][-1])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(5):
        for name, kind, kw in configs:
            e0.record()
            for _ in range(a.iters):
                run(kind, kw)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.iters)
    lines = []
    for name, kind, kw in configs:
        ms = float(np.median(times[name]))
        rec = {"metric": "%s_frames_per_sec" % kind, "config": name, "value": frames[name] / ms * 1e3, "ms_per_batch": ms, "utts": a.utts, "seconds": a.seconds,
               "frames": frames[name], "dim": frontend.feature_dim(kind, **kw), "x_real_time": a.utts * a.seconds / (ms * 1e-3)}
        if kind == "plp":
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(5):
                    run(kind, kw)
                torch.cuda.synchronize()
            dur = {}
            for ev in prof.events():
                if ev.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in ev.name and "Memset" not in ev.name:
                    dur[ev.name] = dur.get(ev.name, 0.0) + ev.device_time_total
            tail = sum(v for k, v in dur.items() if "plp_lpc_kernel" in k)
            rec["lane_per_frame_share_of_kernel_time"] = tail / sum(dur.values()) if dur else None
        lines.append(json.dumps(rec))
        print(lines[-1])
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=512)
    ap.add_argument("--seconds", type=float, default=2.015)          # 200 frames: the C2 utterance
    ap.add_argument("--bins", type=int, default=80)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--cmn", type=int, default=1)
    ap.add_argument("--kind", choices=["fbank", "plp", "spectrogram"], default="fbank")
    ap.add_argument("--out", default="", help="--kind plp|spectrogram: append the JSON lines to this file")
    a = ap.parse_args()
    if a.kind != "fbank":
        return bench_kinds(a)
    import torch
    from libs.amd import frontend, synth
    n = int(a.seconds * 16000)
    base = [torch.from_numpy(synth.synth_wave(n, 900 + i)).cuda() for i in range(8)]
    waves = [base[i % 8] for i in range(a.utts)]
    wave = torch.cat(waves)
    soff = np.arange(a.utts + 1, dtype=np.int64) * n
    feats, off = frontend.fbank_device(wave, soff, num_mel_bins=a.bins, mean_norm=bool(a.cmn))
    frames = int(off[-1])
    for _ in range(20):
        frontend.fbank_device(wave, soff, num_mel_bins=a.bins, mean_norm=bool(a.cmn))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        frontend.fbank_device(wave, soff, num_mel_bins=a.bins, mean_norm=bool(a.cmn))
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.iters
    alg = 4.0 * n * a.utts + 4.0 * a.bins * frames * (3 if a.cmn else 1)
    print(json.dumps({"metric": "fbank_frames_per_sec", "value": frames / ms * 1e3, "ms_per_batch": ms, "utts": a.utts, "frames": frames,
                      "x_real_time": a.utts * a.seconds / (ms * 1e-3), "algorithmic_GBps": alg / ms * 1e-6, "bins": a.bins, "cmn": bool(a.cmn),
                      "note": "waveforms packed in HBM; includes the offsets upload of every call"}))


if __name__ == "__main__":
    main()
