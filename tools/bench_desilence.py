#!/usr/bin/env python3
"""The device de-silence (asv_desilence_pcm16, csrc/kernels_desilence.hip; profiles/desilence_ab.txt), alone and in the waveform-in script:

    python tools/bench_desilence.py entry  [--reps 15] [--calls 50]
    python tools/bench_desilence.py script [--wavs 3000] [--parent-script PATH] [--dir /tmp/asv_desilence]

entry: one batch of 512 x 2 s and one of 64 x 20 s of 16 kHz PCM with about 30 % silent 0.1 s blocks, trimmed through the C ABI.
Event-timed: a window of --calls back-to-back calls between two events, per-call time = window / calls, median / min / max over --reps
windows after 3 warm-up windows.  A call launches four kernels, copies the offsets back and WAITS for the stream (the host needs the kept
counts), so the per-call time includes the launches and that wait - it is not the kernels' time.  Bytes are counted from the rule: every
sample read twice (2 x 2 B) and every kept sample written (2 B).  What the wait costs is measured, not guessed: the same windows run in
three child processes - the product library, the developer library (libasv_amd_dev.so, ASV_AMD_LIB), and the developer library with
ASV_AMD_DESILENCE_NOWAIT=1, which launches the same kernels and returns without the copy and the wait (out_offsets is then not filled;
only that library knows the switch).  The first batch is compared with libs.amd.frontend.de_silence_host before anything is timed.

script: --wavs synthetic 16-bit wav files of 2 - 6 s (32 base signals, about 30 % silent blocks) written once and read from the page cache,
then pipeline/onestep/extract_embeddings_online.py (Xvector(30, ...), f32m default precision) with --de-silence true on the device, with
ASV_AMD_DEVICE_DESILENCE=0 (the reader threads trim), with --de-silence false, and - --parent-script - another checkout's script with the
flag off on the same files; every variant in both positions of the run order.  Per run: the script's loop clock and device clock
(ASV_AMD_REPORT_TIMING), its RTF line, and the process's wall clock end to end.
"""
import argparse
import ctypes as C
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import time
import wave

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "asv-subtools_amd", "pytorch")
sys.path.insert(0, PKG)
SCRIPT = os.path.join(PKG, "pipeline", "onestep", "extract_embeddings_online.py")

HBM_PEAK_TBS = 8.0
WIN = 1600


def silent_mix(rng, samples, share=0.3):
    """int16 noise of +-3000 with `share` of the 0.1 s blocks silent (zeros or +-2 counts)."""
    import numpy as np
    x = rng.randint(-3000, 3001, size=samples).astype(np.int16)
    blocks = -(-samples // WIN)
    kind = rng.rand(blocks)
    for b in np.nonzero(kind < share)[0]:
        a, e = b * WIN, min(samples, (b + 1) * WIN)
        x[a:e] = 0 if kind[b] < share / 2 else rng.randint(-2, 3, size=e - a)
    return x


def entry_child(a):
    import numpy as np
    import torch
    from libs.amd import capi, frontend
    lib = capi.lib()
    dev = torch.device("cuda", 0)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p64 = lambda x: x.ctypes.data_as(C.POINTER(C.c_longlong))
    no_wait = os.environ.get("ASV_AMD_DESILENCE_NOWAIT") is not None
    for utts, seconds in ((512, 2), (64, 20)):
        rng = np.random.RandomState(utts)
        n = seconds * 16000
        host = np.concatenate([silent_mix(rng, n) for _ in range(utts)])
        off = np.arange(utts + 1, dtype=np.int64) * n
        d_wave = torch.from_numpy(host).to(dev)
        out = torch.empty_like(d_wave)
        out_off = np.zeros(utts + 1, dtype=np.int64)

        def call():
            capi.check(lib.asv_desilence_pcm16(d_wave.data_ptr(), p64(off), utts, WIN, 50.0, out.data_ptr(), p64(out_off), stream), "asv_desilence_pcm16")

        call()
        torch.cuda.synchronize(dev)
        got = out.cpu().numpy()
        want = [frontend.de_silence_host(host[u * n:(u + 1) * n], 16000, min_eng=50) for u in range(utts)]
        kept = sum(len(w) for w in want)
        same = None
        if not no_wait:
            same = bool(out_off[-1] == kept and np.array_equal(got[:kept], np.concatenate(want)))
        times = []
        for rep in range(a.reps + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            e0.record()
            for _ in range(a.calls):
                call()
            e1.record()
            e1.synchronize()
            if rep >= 3:
                times.append(e0.elapsed_time(e1) * 1e3 / a.calls)
        t = sorted(times)
        med = statistics.median(t)
        moved = 4 * host.size + 2 * kept
        print(json.dumps({"batch": [utts, seconds], "library": os.path.basename(capi.library_path()), "waits": not no_wait, "equal_to_host_rule": same,
                          "silent_share_of_samples": round(1.0 - kept / host.size, 3), "reps": a.reps, "calls_per_window": a.calls, "bytes_by_rule": moved,
                          "median_us_per_call": round(med, 2), "min_us": round(t[0], 2), "max_us": round(t[-1], 2), "gb_s": round(moved / med / 1e3, 1),
                          "share_of_hbm_peak": round(moved / med / 1e6 / HBM_PEAK_TBS, 3)}), flush=True)
        assert same is not False


def entry(a):
    dev_lib = os.path.join(REPO, "asv-subtools_amd", "libasv_amd_dev.so")
    variants = [("product", {}), ("developer", {"ASV_AMD_LIB": dev_lib}), ("developer, launch only", {"ASV_AMD_LIB": dev_lib, "ASV_AMD_DESILENCE_NOWAIT": "1"})]
    for name, extra in variants + variants[::-1]:
        env = {k: v for k, v in os.environ.items() if k not in ("ASV_AMD_LIB", "ASV_AMD_DESILENCE_NOWAIT")}
        print("# " + name, flush=True)
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "entry-child", "--reps", str(a.reps), "--calls", str(a.calls)], env=dict(env, **extra),
                            timeout=240).returncode
        if rc != 0:
            sys.exit("entry-child (%s) ended with %d: nothing more is started" % (name, rc))


def prepare(directory, wavs):
    import numpy as np
    import torch
    import yaml
    import libs.support.utils as utils
    from libs.amd import frontend, synth
    os.makedirs(directory, exist_ok=True)
    blueprint = os.path.join(PKG, "model", "xvector.py")
    creation = "Xvector(30,10,training=False)"
    model = utils.create_model_from_py(blueprint, creation)
    sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 0)
    files = {k: os.path.join(directory, v) for k, v in (("params", "final.params"), ("cfg", "nnet.config"), ("conf", "feat.yaml"), ("scp", "wav.scp"))}
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, files["params"])
    utils.write_nnet_config(blueprint, creation, files["cfg"])
    with open(files["conf"], "w") as f:
        yaml.safe_dump({"feature_type": "fbank", "kaldi_featset": {"num_mel_bins": 30, "dither": 0.0, "energy_floor": 0.0},
                        "mean_var_conf": {"mean_norm": True, "std_norm": False}}, f)
    rng = np.random.RandomState(11)
    base = [silent_mix(rng, int(rng.randint(2 * 16000, 6 * 16000 + 1))) for _ in range(32)]
    kept = [len(frontend.de_silence_host(x, 16000, min_eng=50)) for x in base]
    samples = trimmed = 0
    with open(files["scp"], "w") as s:
        for i in range(wavs):
            j = (i * 13) % 32
            path = os.path.join(directory, "w%06d.wav" % i)
            with wave.open(path, "wb") as wf:
                wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(16000)
                wf.writeframes(base[j].tobytes())
            s.write("utt%06d %s\n" % (i, path))
            samples += len(base[j])
            trimmed += kept[j]
    files.update(wavs=wavs, seconds=samples / 16000.0, seconds_after_trimming=trimmed / 16000.0)
    return files


def run_once(files, name, script, flags, env_extra, directory):
    out = os.path.join(directory, "xvector.ark")
    env = dict({k: v for k, v in os.environ.items() if k != "ASV_AMD_DEVICE_DESILENCE"}, ASV_AMD_REPORT_TIMING="1", PYTHONPATH=PKG, **env_extra)
    t0 = time.perf_counter()
    res = subprocess.run([sys.executable, script, "--nnet-config", files["cfg"], "--data-type", "raw", "--feat-config", files["conf"], "--gpu-id", "0"] + flags +
                         [files["params"], files["scp"], out], capture_output=True, text=True, env=env, timeout=600)
    dt = time.perf_counter() - t0
    if res.returncode != 0:
        print(res.stdout[-1500:] + res.stderr[-1500:], flush=True)
        sys.exit("%s ended with %d: nothing more is started" % (name, res.returncode))
    rec = {"run": name, "end_to_end_seconds": round(dt, 2)}
    m = re.search(r"Loop: (\d+) utterances in ([0-9.]+) s = ([0-9.]+) utterances/s, device ([0-9.]+) s, ([0-9.]+) s of audio", res.stdout)
    if m:
        rec.update(utterances=int(m.group(1)), loop_seconds=float(m.group(2)), loop_utts_per_s=float(m.group(3)), device_seconds=float(m.group(4)),
                   audio_seconds_by_frames=float(m.group(5)))
    m = re.search(r"RTF:([0-9.]+)", res.stdout)
    rec["rtf"] = float(m.group(1)) if m else None
    m = re.search(r"Extracted (\d+) embeddings", res.stdout)
    rec["extracted"] = int(m.group(1)) if m else None
    os.remove(out)
    print(json.dumps(rec), flush=True)
    return rec


def script_runs(a):
    files = prepare(a.dir, a.wavs)
    try:
        print(json.dumps({"workload": "%d wav files, %.0f s of 16 kHz PCM (%.0f s after trimming at --amp-th 50), page cache" % (
            files["wavs"], files["seconds"], files["seconds_after_trimming"])}), flush=True)
        on = ["--de-silence", "true", "--amp-th", "50"]
        variants = [("this_device", SCRIPT, on, {"ASV_AMD_DEVICE_DESILENCE": "1"}), ("this_host", SCRIPT, on, {"ASV_AMD_DEVICE_DESILENCE": "0"}),
                    ("this_off", SCRIPT, ["--de-silence", "false"], {})]
        if a.parent_script:
            variants.append(("parent_off", a.parent_script, ["--de-silence", "false"], {}))
        run_once(files, "warm-up (this_device)", SCRIPT, on, {}, a.dir)              # untimed in spirit: the files enter the page cache, the code its caches
        for name, script, flags, extra in variants + variants[::-1]:
            run_once(files, name, script, flags, extra, a.dir)
    finally:
        shutil.rmtree(a.dir, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["entry", "entry-child", "script"])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--wavs", type=int, default=3000)
    ap.add_argument("--parent-script", default=None)
    ap.add_argument("--dir", default="/tmp/asv_desilence")
    a = ap.parse_args()
    {"entry": entry, "entry-child": entry_child, "script": script_runs}[a.mode](a)


if __name__ == "__main__":
    main()
