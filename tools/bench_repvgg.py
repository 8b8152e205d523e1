#!/usr/bin/env python3
"""The default RepSPK x-vector (RepVggXvector(80, ...): blocks [2, 4, 14, 1], base width 32) at 256 x 200 x 80, and the tap-table
grid convolution kernel (csrc/kernels_conv_taps.hip) per stage geometry (profiles/repvgg_ab.txt):

    python tools/bench_repvgg.py [--utts 256] [--frames 200] [--steps 10] [--warmup 3] [--precisions bf16,f32m]

Per precision mode: utterances / s of whole extractions (device-resident features, hipEvents around --steps extractions after --warmup),
then ONE profiled extraction (asv_net_set_profiling(2): an event pair around every launch) whose grid_conv_taps rows are summed per
stage geometry (input -> output channels, bins, time subsampling): launches, microseconds per launch, TFLOP/s of the 17 live taps.
Next to every geometry with equal channels stands the yardstick a later performance change starts from: the EXISTING 3 x 3 kernels
(grid_conv_narrow / grid_conv_wide in the 16-bit modes, the split-product kernels in f32m) on one 3 x 3 layer of the same channels
over a grid of the same bins and frames, profiled the same way, its time scaled by 17 / 9.  Synthetic weights (trunk BatchNorm gammas x 0.6,
as tests/repvgg_cases.py damps them: the work does not depend on the values).  One JSON line per precision mode.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "asv-subtools_amd", "pytorch"), os.path.join(REPO, "tests")]


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def profiled_rows(eng, fn):
    fn()
    eng.set_profiling(2)
    eng.get_profile()
    fn()
    rows = eng.get_profile()
    eng.set_profiling(0)
    return rows


def yardstick_us(channels, bins, frames, utts, precision):
    """one 3 x 3 layer channels -> channels behind a one-channel head, on a reach-1 grid of `bins` bins: microseconds of its launch"""
    import numpy as np
    import torch
    from libs.amd import engine, ir
    r = np.random.RandomState(channels * 1000 + bins)
    g = ir.Graph(bins)
    v = g.grid_input()
    pitch = g.grid_spec(v.tid)[3]
    offs = sorted(dt * pitch + df for dt in (-1, 0, 1) for df in (-1, 0, 1))

    def dense(cout, cin):
        w = np.zeros((cout, cin, offs[-1] - offs[0] + 1), dtype=np.float32)
        for o in offs:
            w[:, :, o - offs[0]] = r.randn(cout, cin) / np.sqrt(9.0 * cin)
        return w

    v = g.tdnn(v, dense(channels, 1), np.zeros(channels, np.float32), offs, offs[0], act1="relu")
    v = g.tdnn(v, dense(channels, channels), np.zeros(channels, np.float32), offs, offs[0], act1="relu")
    g.output = g.pool(v, stddev=True, per_bin=True)
    eng = engine.Engine(g, precision=precision)
    feats = torch.randn(utts * frames, bins, device="cuda")
    offsets = np.arange(utts + 1, dtype=np.int32) * frames
    rows = profiled_rows(eng, lambda: eng.extract_device(feats, offsets))
    us = [1e3 * row["total_ms"] for row in rows if row["op_index"] == 2]
    eng.close()
    return us[0] if len(us) == 1 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precisions", default="bf16,f32m")
    a = ap.parse_args()
    import numpy as np
    import torch
    import helpers
    import repvgg_cases as RC
    from libs.amd import synth

    model = helpers.build_model(RC.BLUEPRINT, "RepVggXvector(80,10,training=False)")
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in RC.scaled_state_dict(synth, shapes, 63, 0.6).items()})
    model.cuda()
    feats = torch.from_numpy(np.concatenate([synth.synth_feats(a.frames, 80, 700 + i) for i in range(a.utts)])).cuda()
    offsets = np.arange(a.utts + 1, dtype=np.int32) * a.frames
    for precision in a.precisions.split(","):
        model.amd_precision = precision
        eng = model._amd_engine()
        run = lambda: eng.extract_device(feats, offsets)
        ms = timed(run, a.steps, a.warmup)
        status = eng.status()
        rows = profiled_rows(eng, run)
        graph = eng.graph
        stages = {}
        for row in rows:
            if row["name"] != "grid_conv_taps":
                continue
            op = eng.ops[row["op_index"]]
            spec = graph.grid_spec(op.inp.tid)
            key = (op.inp.channels, op.out.channels, spec[2], spec[1], len(op.taps))
            s = stages.setdefault(key, dict(launches=0, ms=0.0, flops=0.0))
            s["launches"] += row["launches"]; s["ms"] += row["total_ms"]; s["flops"] += row["flops"]
        out = []
        for (cin, cout, bins, shift, taps), s in sorted(stages.items(), key=lambda kv: (kv[0][3], kv[0][0])):
            us = 1e3 * s["ms"] / s["launches"]
            rec = {"channels": [cin, cout], "bins": bins, "frames": a.frames >> shift, "taps": taps, "launches": s["launches"], "us_per_launch": round(us, 1),
                   "tflops": round(s["flops"] / s["ms"] / 1e9, 1)}
            if cin == cout:
                y = yardstick_us(cin, bins, a.frames >> shift, a.utts, precision)
                if y is not None:
                    rec["yardstick_3x3_us"] = round(y, 1)
                    rec["yardstick_3x3_x_17_9_us"] = round(y * taps / 9.0, 1)
            out.append(rec)
        total = sum(r["total_ms"] for r in rows)
        taps_ms = sum(s["ms"] for s in stages.values())
        print(json.dumps({"model": "RepVggXvector(80) RepSPK [2,4,14,1] base width 32", "precision": precision, "batch": [a.utts, a.frames, 80],
                          "ms_per_extraction": round(ms, 2), "utts_per_s": round(a.utts / ms * 1e3, 1), "status": status,
                          "profiled_ms_all_kernels": round(total, 2), "profiled_ms_grid_conv_taps": round(taps_ms, 2), "grid_conv_taps_by_stage": out}))


if __name__ == "__main__":
    main()
