#!/usr/bin/env python3
"""What the one-launch Res2 chain (res2n_chain_kernel, kernels_res2n.hip) buys on the benchmark ECAPA-TDNN blueprint
(model/ecapa-tdnn-xvector.py, defaults: channels 512): 256 utterances of 300 frames, synthetic weights, one process.

Two engines of the same program - the 16-bit default (three res2n ops) and ASV_AMD_RES2N=0 (21 per-branch layers + 3 copies) - run
alternately after a warm-up.  Reported: the whole step from device events (median and spread over the repeats), then, from a second
pass with per-op profiling on (Engine.get_profile), the time of the Res2 rows of each engine and their share of the profiled step.

    python tools/res2n_profile_workload.py [bf16|f16] [repeats]
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "asv-subtools_amd", "pytorch"), os.path.join(REPO, "tests")]


def build_engines(precision):
    import torch
    import helpers
    from libs.amd import engine, synth
    model = helpers.build_model("ecapa-tdnn-xvector.py", "ECAPA_TDNN(80,10,training=False)")
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 41).items()})
    model.cuda()
    engines = {}
    for tag, switch in (("fused", "1"), ("per-branch", "0")):
        os.environ["ASV_AMD_RES2N"] = switch
        engines[tag] = engine.compile_model(model, precision=precision)
    os.environ.pop("ASV_AMD_RES2N")
    return engines


def res2_rows(eng):
    """indices (in the uploaded program) of the ops that make up the Res2 blocks"""
    return {i for i, op in enumerate(eng.ops)
            if op.kind == "res2n" or (op.kind == "tdnn" and len(op.taps) == 3 and op.inp.channels == 64)
            or (op.kind == "eltwise" and op.a.channels == 64 and op.b is None and op.seg_scale is None)}


def main(precision="bf16", repeats=20, warmup=5):
    import torch
    from libs.amd import synth
    engines = build_engines(precision)
    feats = torch.from_numpy(np.concatenate([synth.synth_feats(300, 80, 7500 + i) for i in range(256)])).cuda()
    offsets = np.arange(257, dtype=np.int32) * 300
    outs = {}
    for _ in range(warmup):
        for tag, eng in engines.items():
            outs[tag] = eng.extract_device(feats, offsets)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(o).all()) for o in outs.values())
    a, b = outs["fused"].cpu().numpy(), outs["per-branch"].cpu().numpy()
    print("%s: fused vs per-branch embeddings: max |diff| / max |ref| = %.3g" % (precision, float(np.abs(a - b).max() / np.abs(b).max())))
    times = {tag: [] for tag in engines}
    for _ in range(repeats):
        for tag, eng in engines.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            eng.extract_device(feats, offsets)
            t1.record()
            t1.synchronize()
            times[tag].append(t0.elapsed_time(t1))
    for tag, t in times.items():
        t = np.sort(np.asarray(t))
        print("%s %-10s step: median %.3f ms  min %.3f  max %.3f  (%d repeats; %d ops, %d of them Res2)" % (
            precision, tag, float(np.median(t)), t[0], t[-1], len(t), len(engines[tag].ops), len(res2_rows(engines[tag]))))
    for tag, eng in engines.items():
        eng.set_profiling(2)
        eng.extract_device(feats, offsets)
        eng.get_profile()                                     # the first profiled step creates the events
        per = []
        for _ in range(5):
            eng.extract_device(feats, offsets)
            rows = eng.get_profile()
            idx = res2_rows(eng)
            res2 = sum(r["total_ms"] for r in rows if r["op_index"] in idx)
            per.append((res2, sum(r["total_ms"] for r in rows), sum(r["launches"] for r in rows if r["op_index"] in idx)))
        eng.set_profiling(0)
        res2, total, launches = (float(np.median([p[k] for p in per])) for k in range(3))
        print("%s %-10s Res2 rows: %.3f ms in %d launches (range %.3f - %.3f) = %.1f %% of the %.3f ms the profiled ops take" % (
            precision, tag, res2, launches, min(p[0] for p in per), max(p[0] for p in per), 100.0 * res2 / total, total))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "bf16", int(sys.argv[2]) if len(sys.argv) > 2 else 20)
