#!/usr/bin/env python3
"""The default transformer x-vector (TransformerXvector(80, ..., transformer_type='transformer'): conv2d front, d = 256, 4 heads, 6
blocks, 2048 units, out_dim 1536) at 256 x 300 x 80, one stream, and the share of its own kernels (profiles/transformer_ab.txt):

    python tools/bench_transformer.py [--utts 256] [--frames 300] [--steps 10] [--warmup 3] [--precisions bf16,f32m]
    python tools/bench_transformer.py --cpu-reference /path/to/reference [--utts 8]

Per precision mode: utterances / s of whole extractions (device-resident features, hipEvents around --steps extractions after
--warmup, max_chunk 300 as the blueprint's decorator sets it), then ONE profiled extraction (asv_net_set_profiling(1): an event pair
around every launch) as the per-kernel table of asv_net_get_profile: launches, milliseconds, share of the profiled time, TFLOP/s where
the kernel reports its algorithmic FLOPs.  Synthetic weights (the work does not depend on the values).  One JSON line per mode.

--cpu-reference: the reference's own model (its tree is given on the command line; build container only) on this host's CPU, one
utterance at a time as its extraction loop runs them - context for the device figures, never read on the GPU machine.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CREATION = "TransformerXvector(80,10,training=False,transformer_type='transformer')"
OWN_KERNELS = ("self_attention", "posenc", "front_conv")


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


def cpu_reference(ref_root, utts, frames):
    sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
    from oracle import gen_golden as G
    G.install_shims()
    sys.path.insert(0, os.path.join(ref_root, "pytorch"))
    import torch
    import libs.support.utils as utils
    synth = G.load_synth()
    model = utils.create_model_from_py(os.path.join(ref_root, "pytorch", "model", "transformer_xvector.py"), CREATION)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 73).items()}, strict=True)
    model.eval()
    mats = [synth.synth_feats(frames, 80, 700 + i) for i in range(utts)]
    model.extract_embedding(mats[0])
    t0 = time.time()
    for m in mats:
        model.extract_embedding(m)
    dt = time.time() - t0
    print(json.dumps({"model": CREATION, "where": "reference on CPU, %d torch threads" % torch.get_num_threads(), "batch": [utts, frames, 80],
                      "utts_per_s": round(utts / dt, 2)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precisions", default="bf16,f32m")
    ap.add_argument("--cpu-reference", default=None, metavar="REFERENCE_ROOT")
    a = ap.parse_args()
    if a.cpu_reference:
        return cpu_reference(a.cpu_reference, a.utts, a.frames)
    sys.path[:0] = [os.path.join(REPO, "asv-subtools_amd", "pytorch"), os.path.join(REPO, "tests")]
    import numpy as np
    import torch
    import helpers
    from libs.amd import synth

    model = helpers.build_model("transformer_xvector.py", CREATION)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 73).items()})
    model.cuda()
    max_chunk = type(model).extract_embedding.max_chunk
    feats = torch.from_numpy(np.concatenate([synth.synth_feats(a.frames, 80, 700 + i) for i in range(a.utts)])).cuda()
    offsets = np.arange(a.utts + 1, dtype=np.int32) * a.frames
    for precision in a.precisions.split(","):
        model.amd_precision = precision
        eng = model._amd_engine()
        run = lambda: eng.extract_device(feats, offsets, max_chunk=max_chunk)
        ms = timed(run, a.steps, a.warmup)
        status = eng.status()
        run()
        eng.set_profiling(1)
        eng.get_profile()
        run()
        rows = eng.get_profile()
        eng.set_profiling(0)
        total = sum(r["total_ms"] for r in rows)
        table = [{"kernel": r["name"], "launches": r["launches"], "ms": round(r["total_ms"], 3), "share": round(r["total_ms"] / total, 4),
                  "tflops": round(r["flops"] / r["total_ms"] / 1e9, 1) if r["flops"] else None} for r in sorted(rows, key=lambda r: -r["total_ms"])]
        own = {k: round(sum(r["total_ms"] for r in rows if r["name"] == k) / total, 4) for k in OWN_KERNELS}
        print(json.dumps({"model": CREATION, "precision": precision, "batch": [a.utts, a.frames, 80], "max_chunk": max_chunk,
                          "ms_per_extraction": round(ms, 2), "utts_per_s": round(a.utts / ms * 1e3, 1), "status": status,
                          "device_mib": round(eng.device_bytes() / 2.0 ** 20), "profiled_ms_all_kernels": round(total, 2), "share_of_own_kernels": own,
                          "kernels": table}))


if __name__ == "__main__":
    main()
