#!/usr/bin/env python3
"""A/B of the all-pairs PLDA LLR at VoxCeleb1-O scale against a 10 000-vector cohort (profiles/plda_matrix_ab.txt):
E = 4 708 enrolment vectors x T = 10 000 cohort vectors at dim 150 and dim 256, three routes through the C ABI in ONE process,
hipEvent-timed, interleaved, median and min - max of --reps (>= 10) after a warm-up:

    (a) asv_plda_llr_trials over all E x T index pairs - the only route before asv_plda_llr_matrix existed
    (b) asv_plda_llr_matrix: per-vector preparation + the f64 matrix-core kernel (score_matrix_kernel)
    (c) developer build only (libasv_amd_dev.so, -DASV_WITH_ABLATION): the same prepared operands through the vector-unit
        gemm64_kernel of plda_train.hip + a row add, selected per call with ASV_AMD_SCORE_MATRIX=valu

    python tools/bench_plda_matrix.py [--reps 12] [--out profiles/plda_matrix_ab.txt]
    ASV_AMD_LIB=asv-subtools_amd/libasv_amd_dev.so python tools/bench_plda_matrix.py      # with route (c)

(b) and (c) time the ENTRY POINT: preparation kernels included (O((E + T) dim) against the O(E T dim) product).  The f64 rate of (b) is
2 E T (2 dim) over its time.  The results of (a), (b), (c) are compared with each other before anything is timed.  The script ends itself
after --time-limit seconds (a timer of its own: a hung device call must not outlive it)."""
import argparse
import ctypes as C
import os
import signal
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "asv-subtools_amd", "pytorch"))
sys.path.insert(0, os.path.join(REPO, "tests"))

SHAPES = ((4708, 10000, 150), (4708, 10000, 256))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--time-limit", type=int, default=420)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.reps < 10:
        sys.exit("--reps: at least 10")
    signal.alarm(args.time_limit)                     # SIGALRM's default action ends the process
    import numpy as np
    import torch
    import plda_matrix_cases as PM
    from libs.amd import capi
    lib = capi.lib()
    dev_build = os.path.basename(capi.library_path()) == "libasv_amd_dev.so"
    dev = torch.device("cuda", 0)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    lines = ["# tools/bench_plda_matrix.py --reps %d: %s on %s" % (args.reps, os.path.basename(capi.library_path()), torch.cuda.get_device_name(0)),
             "# ms per call: median (min - max); (b), (c): entry point, preparation kernels included"]
    for E, T, dim in SHAPES:
        enroll, test, psi, n = PM.make_llr_case(E, T, dim, seed=77, mixed_n=True)
        e, t, p, en = (torch.from_numpy(a).to(dev) for a in (enroll, test, psi, n))
        ei = torch.arange(E, dtype=torch.int32, device=dev).repeat_interleave(T).contiguous()
        ti = torch.arange(T, dtype=torch.int32, device=dev).repeat(E).contiguous()
        out_a = torch.empty(E * T, dtype=torch.float32, device=dev)
        out_b, out_c = torch.empty((E, T), dtype=torch.float32, device=dev), torch.empty((E, T), dtype=torch.float32, device=dev)

        def route_a():
            capi.check(lib.asv_plda_llr_trials(ptr(e), ptr(t), dim, ptr(p), ptr(en), ptr(ei), ptr(ti), E * T, ptr(out_a), stream), "asv_plda_llr_trials")

        def route_b():
            os.environ.pop("ASV_AMD_SCORE_MATRIX", None)
            capi.check(lib.asv_plda_llr_matrix(ptr(e), E, ptr(t), T, dim, ptr(p), ptr(en), ptr(out_b), stream), "asv_plda_llr_matrix")

        def route_c():
            os.environ["ASV_AMD_SCORE_MATRIX"] = "valu"
            try:
                capi.check(lib.asv_plda_llr_matrix(ptr(e), E, ptr(t), T, dim, ptr(p), ptr(en), ptr(out_c), stream), "asv_plda_llr_matrix (valu)")
            finally:
                os.environ.pop("ASV_AMD_SCORE_MATRIX", None)
        routes = [("a  asv_plda_llr_trials, all pairs", route_a), ("b  asv_plda_llr_matrix (f64 MFMA)", route_b)]
        if dev_build:
            routes.append(("c  same operands, gemm64_kernel + row add", route_c))
        for _ in range(args.warmup):
            for _, fn in routes:
                fn()
        torch.cuda.synchronize()
        diff_ab = float((out_a.view(E, T) - out_b).abs().max())
        scale = float(out_b.abs().max())
        diff_bc = "%.3g" % float((out_b - out_c).abs().max()) if dev_build else "n/a (developer build only)"
        times = {name: [] for name, _ in routes}
        for _ in range(args.reps):
            for name, fn in routes:                   # interleaved: clock and thermal drift hit every route alike
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                t1.synchronize()
                times[name].append(t0.elapsed_time(t1))
        lines.append("")
        lines.append("E %d x T %d, dim %d (K = %d): max |LLR| %.4g, max |a - b| %.3g, max |b - c| %s" % (E, T, dim, 2 * dim, scale, diff_ab, diff_bc))
        med = {}
        for name, _ in routes:
            v = times[name]
            med[name] = statistics.median(v)
            extra = ""
            if name.startswith("b") or name.startswith("c"):
                extra = "   %.2f f64 TFLOP/s (2 E T 2 dim / time)" % (2.0 * E * T * 2 * dim / (med[name] * 1e-3) / 1e12)
            lines.append("  (%s)%s %10.3f  (%.3f - %.3f)%s" % (name[0], name[1:].ljust(44), med[name], min(v), max(v), extra))
        a, b = med[routes[0][0]], med[routes[1][0]]
        lines.append("  speed-up (a) / (b): %.1f x" % (a / b) + ("   (c) / (b): %.2f x" % (med[routes[2][0]] / b) if dev_build else "   (c): developer build only, not in this library"))
        del e, t, p, en, ei, ti, out_a, out_b, out_c
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
