#!/usr/bin/env python3
"""Two measurements of the device ingest (sliding CMN + voiced-frame selection inside extraction; profiles/ingest_ab.txt):

    python tools/bench_ingest.py kernel [--reps 25]
        asv_ingest_frames against the three launches it replaces (asv_cmvn_sliding -> asv_select_frames = rank + gather), event-timed
        through the C ABI, interleaved, median of --reps after warm-up, on one batch of 321 x 200 x 30 and one of 256 x 200 x 80 with 70 %
        of the frames voiced; outputs compared bit for bit.  Bytes are counted from the shapes.  The event-timed figures are those of the
        ENTRY POINTS: the old ones upload their offsets and synchronise the stream in every call; the fused one is timed twice - with
        the same offsets every call (its staged upload is reused: no copy) and with the flags, hence the kept offsets, alternating
        between two sets (an asynchronous upload per call, as in the --vad-scp loop).  Kernel times alone: run this under
        `rocprofv3 --kernel-trace --stats`.

    python tools/bench_ingest.py script [--utts 50000] [--dim 80] [--precision f32x] [--dir /tmp/asv_ingest]
        the extraction script's loop rate (ASV_AMD_REPORT_TIMING) on tools/bench_pipeline.py's table of --utts x 200 frames from the page
        cache: the plain path against `--cmn-window 300 --vad-scp vad.scp` of the same build, two runs each in alternation, the better
        one reported, with the consumer thread's breakdown of the ingest run.
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "asv-subtools_amd", "pytorch"))
sys.path.insert(0, os.path.join(REPO, "tools"))


def kernel_ab(reps):
    import numpy as np
    import torch
    from libs.amd import capi, frontend, synth
    lib = capi.lib()
    dev = torch.device("cuda", 0)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_longlong))
    for utts, frames, dim in ((321, 200, 30), (256, 200, 80)):
        off = (np.arange(utts + 1, dtype=np.int64) * frames)
        base = [synth.synth_feats(frames, dim, 70 + i) * 3.0 + 1.5 for i in range(16)]
        x = torch.from_numpy(np.concatenate([base[i % 16] for i in range(utts)])).to(dev)
        flags = (np.random.RandomState(1).rand(utts * frames) < 0.7).astype(np.uint8)
        voiced = torch.from_numpy(flags).to(dev)
        kept_off = frontend.kept_offsets(flags, off)[1]
        rows = int(kept_off[-1])
        normed, composed, fused = torch.empty_like(x), torch.empty((rows, dim), device=dev), torch.empty((rows, dim), device=dev)
        flags2 = (np.random.RandomState(2).rand(utts * frames) < 0.7).astype(np.uint8)
        alt = [(voiced, kept_off, fused), (torch.from_numpy(flags2).to(dev), frontend.kept_offsets(flags2, off)[1], torch.empty((utts * frames, dim), device=dev))]
        turn = [0]

        def three_launches():
            capi.check(lib.asv_cmvn_sliding(x.data_ptr(), normed.data_ptr(), p64(off), utts, dim, 300, 100, 1, 0, stream))
            capi.check(lib.asv_select_frames(normed.data_ptr(), voiced.data_ptr(), p64(off), p64(kept_off), utts, dim, composed.data_ptr(), stream))

        def one_launch():
            capi.check(lib.asv_ingest_frames(x.data_ptr(), voiced.data_ptr(), p64(off), p64(kept_off), utts, dim, 300, 100, 1, 0, fused.data_ptr(), stream))

        def one_launch_new_offsets():
            turn[0] ^= 1
            v, k, o = alt[turn[0]]
            capi.check(lib.asv_ingest_frames(x.data_ptr(), v.data_ptr(), p64(off), p64(k), utts, dim, 300, 100, 1, 0, o.data_ptr(), stream))

        times = {"three launches": [], "fused": [], "fused, offsets changed": []}
        for rep in range(reps + 5):
            for name, fn in (("three launches", three_launches), ("fused", one_launch), ("fused, offsets changed", one_launch_new_offsets)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                a.record()
                fn()
                b.record()
                b.synchronize()
                if rep >= 5:
                    times[name].append(a.elapsed_time(b) * 1e3)
        same = bool(torch.equal(composed.view(torch.int32), fused.view(torch.int32)))
        raw, kept = utts * frames * dim * 4, rows * dim * 4
        moved = {"three launches": raw + raw + utts * frames + rows * 8 + rows * 8 + kept + kept, "fused": raw + utts * frames + kept}
        moved["fused, offsets changed"] = moved["fused"]
        rec = {"batch": [utts, frames, dim], "voiced_share": round(rows / (utts * frames), 3), "bit_equal": same, "reps": reps}
        for name in times:
            t = sorted(times[name])
            rec[name] = {"median_us": round(statistics.median(t), 1), "min_us": round(t[0], 1), "max_us": round(t[-1], 1), "hbm_bytes_by_shape": moved[name]}
        rec["fused_over_three"] = round(rec["fused"]["median_us"] / rec["three launches"]["median_us"], 3)
        print(json.dumps(rec))
        assert same


def script_rate(utts, dim, precision, directory):
    import numpy as np
    import bench_pipeline
    from libs.support import kaldi_io
    files = bench_pipeline.prepare(directory, utts, 200, dim=dim)
    vad_ark, vad_scp = os.path.join(directory, "vad.ark"), os.path.join(directory, "vad.scp")
    rng = np.random.RandomState(2)
    base = [b"\0BFV \4" + np.int32(200).tobytes() + (rng.rand(200) < 0.7).astype(np.float32).tobytes() for _ in range(64)]
    with open(vad_ark, "wb") as f, open(vad_scp, "w") as s:
        pos = 0
        for i in range(utts):
            key = ("utt%07d " % i).encode()
            f.write(key)
            pos += len(key)
            s.write("utt%07d %s:%d\n" % (i, vad_ark, pos))
            f.write(base[i % 64])
            pos += len(base[i % 64])
    script = bench_pipeline.SCRIPT
    env = dict(os.environ, ASV_AMD_PRECISION=precision, ASV_AMD_REPORT_TIMING="1")
    best = {}
    try:
        for rnd in range(2):
            for name, extra in (("plain", []), ("ingest", ["--cmn-window", "300", "--vad-scp", vad_scp])):
                out = os.path.join(directory, "xvector_%s.ark" % name)
                res = subprocess.run([sys.executable, script, "--nnet-config", files["cfg"], "--use-gpu", "true", "--gpu-id", "0"] + extra +
                                     [files["params"], "scp:" + files["scp"], "ark:" + out], capture_output=True, text=True, env=env, timeout=900)
                if res.returncode != 0:
                    print((res.stdout + res.stderr)[-3000:])
                    raise SystemExit(1)
                n = sum(1 for _ in kaldi_io.read_vec_flt_ark(out))
                os.remove(out)
                m = re.search(r"Loop\[(\w+)\]: (\d+) utterances in ([0-9.]+) s = ([0-9.]+) utterances/s", res.stdout)
                rate = float(m.group(4))
                lines = [l for l in res.stdout.splitlines() if l.startswith("Loop[")]
                print("run %d %-6s %d vectors  %s" % (rnd, name, n, " | ".join(lines)))
                if name not in best or rate > best[name][0]:
                    best[name] = (rate, lines)
        print(json.dumps({"table": [utts, 200, dim], "precision": precision, "plain_loop_utts_per_s": best["plain"][0], "ingest_loop_utts_per_s": best["ingest"][0],
                          "ingest_over_plain": round(best["ingest"][0] / best["plain"][0], 3)}))
    finally:
        for name in ("feats.ark", "feats.scp", "final.params", "nnet.config", "vad.ark", "vad.scp", "xvector_plain.ark", "xvector_ingest.ark"):
            try:
                os.remove(os.path.join(directory, name))
            except OSError:
                pass
        try:
            os.rmdir(directory)
        except OSError:
            pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "script"])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--utts", type=int, default=50000)
    ap.add_argument("--dim", type=int, default=80)
    ap.add_argument("--precision", default="f32x")
    ap.add_argument("--dir", default="/tmp/asv_ingest")
    a = ap.parse_args()
    if a.what == "kernel":
        kernel_ab(a.reps)
    else:
        script_rate(a.utts, a.dim, a.precision, a.dir)


if __name__ == "__main__":
    main()
