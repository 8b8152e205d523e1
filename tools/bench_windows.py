#!/usr/bin/env python3
"""Sliding (diarisation) extraction, two routes over the same windows:

    (a) sliding   extract_embeddings.py --sliding true --segments ... --cmn-window 300 scp:feats.scp
                  every parent is read once per batch that holds windows of it; asv_ingest_windows builds the windows on the device
    (b) ranged    extract_embeddings.py --cmn-window 300 scp:ranged.scp, one 'file:offset[first:last]' entry per window
                  the route that existed before --sliding: the WHOLE parent is read and decoded on the host once per window

on a synthetic table of R parents x T x 80, one whole-parent segment each, written as float32 and as 'CM ' compressed matrices.  Route
(b) is quadratic in T (windows x parent length), so it is only run on the SMALL table (--ranged-frames); route (a) runs on that table
too - the like-for-like comparison - and on the large one (--frames).  Per run: the script's own clock around its loop
(ASV_AMD_REPORT_TIMING; route (a)'s includes making the windows from the segments file, route (b)'s scp comes ready-made) and process
start to exit, both per window; every run is made in both positions of the run sequence, as
tools/bench_pipeline.py does.

    python tools/bench_windows.py [--parents 8] [--frames 60000] [--ranged-frames 6000] [--formats f32,cm] [--out profiles/windows_ab.txt]
"""
import argparse
import os
import re
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "asv-subtools_amd", "pytorch"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(REPO, "asv-subtools_amd", "pytorch", "pipeline", "onestep", "extract_embeddings.py")
DIM = 80


def prepare_model(directory):
    import torch
    import libs.support.utils as utils
    from libs.amd import synth
    blueprint = os.path.join(REPO, "asv-subtools_amd", "pytorch", "model", "xvector.py")
    creation = "Xvector(%d,10,training=False)" % DIM
    model = utils.create_model_from_py(blueprint, creation)
    sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 0)
    params, cfg = os.path.join(directory, "final.params"), os.path.join(directory, "nnet.config")
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, params)
    utils.write_nnet_config(blueprint, creation, cfg)
    return params, cfg


def prepare_table(directory, name, parents, frames, compress):
    """<name>.ark / .scp / .segments / .ranged.scp: `parents` matrices of `frames` x 80, one segment over each, and the range-specified
    entries of the windows the sliding mode makes of them (the same rules: libs.amd.subsegments).  Returns the paths and the window count."""
    import numpy as np
    from bench_pipeline import compress_cm
    from libs.amd import subsegments, synth
    base = [synth.synth_feats(frames, DIM, 60_000 + i) for i in range(min(parents, 4))]
    if compress:
        payload = [compress_cm(m) for m in base]
    else:
        payload = [b"\0BFM \4" + np.int32(frames).tobytes() + b"\4" + np.int32(DIM).tobytes() + m.tobytes() for m in base]
    files = {k: os.path.join(directory, "%s.%s" % (name, k)) for k in ("ark", "scp", "segments", "ranged.scp")}
    keys, rx = ["par%04d" % i for i in range(parents)], {}
    with open(files["ark"], "wb") as f, open(files["scp"], "w") as s, open(files["segments"], "w") as g:
        for i, key in enumerate(keys):
            f.write((key + " ").encode())
            rx[key] = "%s:%d" % (files["ark"], f.tell())
            s.write("%s %s\n" % (key, rx[key]))
            f.write(payload[i % len(payload)])
            g.write("%s rec%04d 0.00 %.2f\n" % (key, i, frames * 0.01))
    with open(files["segments"]) as g:
        subs = subsegments.uniform_subsegments(g.read().splitlines())
    kept, first, last = subsegments.frame_ranges(subs, {key: frames for key in keys})
    with open(files["ranged.scp"], "w") as s:
        for (new_utt, utt, _, _), a, b in zip(kept, first, last):
            s.write("%s %s[%d:%d]\n" % (new_utt, rx[utt], a, b))
    files["windows"] = len(kept)
    files["bytes"] = os.path.getsize(files["ark"])
    return files


def run_once(route, table, model, precision, directory, timeout=900):
    from libs.support import kaldi_io
    params, cfg = model
    out = os.path.join(directory, "xvector_%s.ark" % route)
    if route == "sliding":
        extra, rspec = ["--sliding", "true", "--segments", table["segments"]], "scp:" + table["scp"]
    else:
        extra, rspec = [], "scp:" + table["ranged.scp"]
    env = dict(os.environ, ASV_AMD_PRECISION=precision, ASV_AMD_REPORT_TIMING="1")
    t0 = time.perf_counter()
    res = subprocess.run([sys.executable, SCRIPT, "--nnet-config", cfg, "--use-gpu", "true", "--gpu-id", "0", "--cmn-window", "300"] + extra +
                         [params, rspec, "ark:" + out], capture_output=True, text=True, env=env, timeout=timeout)
    dt = time.perf_counter() - t0
    if res.returncode != 0:
        return {"error": (res.stdout + res.stderr)[-1500:]}
    n = sum(1 for _ in kaldi_io.read_vec_flt_ark(out))
    os.remove(out)
    rec = {"windows": n, "complete": n == table["windows"], "process_seconds": dt}
    m = re.search(r"Loop\[(\w+)\]: (\d+) utterances in ([0-9.]+) s", res.stdout)
    if m:
        rec["loop_seconds"] = float(m.group(3))
    m = re.search(r"submit pieces: (.*)", res.stdout)
    if m:
        rec["submit"] = m.group(1)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parents", type=int, default=8)
    ap.add_argument("--frames", type=int, default=60000, help="rows per parent of the large table (route (a) only): 60000 = ten minutes")
    ap.add_argument("--ranged-frames", type=int, default=6000, help="rows per parent of the small table, the one route (b) is run on")
    ap.add_argument("--formats", default="f32,cm")
    ap.add_argument("--precision", default="f32x")
    ap.add_argument("--dir", default="/tmp/asv_windows")
    ap.add_argument("--out", default="", help="also write the report here")
    args = ap.parse_args()
    os.makedirs(args.dir, exist_ok=True)
    lines = []

    def say(line=""):
        print(line, flush=True)
        lines.append(line)

    say("# sliding extraction A/B (tools/bench_windows.py): %d parents x T x %d, window 1.5 s / period 0.75 s, --cmn-window 300, precision %s" % (
        args.parents, DIM, args.precision))
    say("# (a) sliding = --sliding true over the parents; (b) ranged = the plain script over one range-specified scp entry per window")
    say("# route (b) reads and decodes the whole parent once per window - quadratic in T - so it runs on the SMALL table (T = %d) only;" % args.ranged_frames)
    say("# route (a) runs on the small table too (like for like) and on the large one (T = %d)" % args.frames)
    say("# per run: loop = the script's own clock around read -> device -> write; process = start to exit (model load, engine warm-up included)")
    model = prepare_model(args.dir)
    made = []
    try:
        for fmt in args.formats.split(","):
            small = prepare_table(args.dir, "small_" + fmt, args.parents, args.ranged_frames, fmt == "cm")
            large = prepare_table(args.dir, "large_" + fmt, args.parents, args.frames, fmt == "cm")
            made += [small, large]
            say("")
            say("## %s: small table %d windows (%.1f MB), large table %d windows (%.1f MB)" % (
                "'CM ' compressed" if fmt == "cm" else "float32", small["windows"], small["bytes"] / 1e6, large["windows"], large["bytes"] / 1e6))
            run_once("sliding", small, model, args.precision, args.dir)               # one untimed run: cold code pages, the table into the page cache
            plan = [("(a) sliding, small", "sliding", small), ("(b) ranged,  small", "ranged", small), ("(a) sliding, large", "sliding", large)]
            best = {}
            for position, order in enumerate((plan, list(reversed(plan)))):
                for name, route, table in order:
                    rec = run_once(route, table, model, args.precision, args.dir)
                    if "error" in rec:
                        say("%s  position %d  FAILED: %s" % (name, position, rec["error"][-300:].replace("\n", " | ")))
                        continue
                    n = rec["windows"]
                    loop = rec.get("loop_seconds", float("nan"))
                    say("%s  sequence %d  windows %6d%s  loop %8.3f s = %8.1f us/window   process %7.2f s = %8.1f us/window" % (
                        name, position, n, "" if rec["complete"] else " (INCOMPLETE)", loop, 1e6 * loop / n, rec["process_seconds"], 1e6 * rec["process_seconds"] / n))
                    if "submit" in rec:
                        say("    submit pieces: " + rec["submit"])
                    if name not in best or loop < best[name][0]:
                        best[name] = (loop, rec["process_seconds"], n)
            a, b = best.get("(a) sliding, small"), best.get("(b) ranged,  small")
            if a and b:
                say("=> small table, best of two: (a) %.1f us/window loop, %.1f us/window process; (b) %.1f and %.1f: (b) / (a) = %.2fx loop, %.2fx process" % (
                    1e6 * a[0] / a[2], 1e6 * a[1] / a[2], 1e6 * b[0] / b[2], 1e6 * b[1] / b[2], b[0] / a[0], b[1] / a[1]))
            c = best.get("(a) sliding, large")
            if c:
                say("=> large table, best of two: (a) %.1f us/window loop, %.1f us/window process" % (1e6 * c[0] / c[2], 1e6 * c[1] / c[2]))
    finally:
        for table in made:
            for k in ("ark", "scp", "segments", "ranged.scp"):
                try:
                    os.remove(table[k])
                except OSError:
                    pass
        for path in model:
            try:
                os.remove(path)
            except OSError:
                pass
        try:
            os.rmdir(args.dir)
        except OSError:
            pass
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
