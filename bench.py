#!/usr/bin/env python3
"""Benchmark of the extraction hot path on MI355X.

One "step" = one pass of the hot path over one batch of synthetic input that is already resident in HBM:
BASELINE.json configs[1] - standard TDNN x-vector, 80-dim fbank, 200-frame utterances, bf16 MFMA (f32 accumulate,
f32 pooled tail) - 256 utterances per GPU per step, exactly as configs[1] states; the same harness at 640 utterances per step
(whole rounds of workgroups, see LABLOG.md) is reported in the same line (`value_at_b640`, `roofline_at_b640`).
Weak scaling: every rank extracts its own shard; with N > 1 the embeddings are collected with one RCCL all-gather per
step (the path's only exchange).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
                                                               (N > 1 without a launcher: bench.py spawns its own ranks)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, settles the clock, runs W warm-up steps, times ONE region of exactly K steps and prints ONE JSON line
on rank 0: `value` = utterances per second of that region, `ms_per_step` = its time / K.  `--dump-outputs DIR` writes
what the last timed step delivered to its caller (the embeddings; gathered over the ranks when N > 1) to DIR/embeddings.npy
(float32); the inputs and weights are seeded, so the same arguments give the same inputs in every run.

`--full` adds everything else, as described below.  With it, `value` comes from the MEDIAN of `repeats` back-to-back
timed regions of exactly K steps each (the regions are repeated until >= --min-seconds have been measured), and the line
adds `roofline` (frame-level GEMM launches, hipEvent-timed inside libasv_amd.so on the extract stream during timed steps),
`parity` (utterances of the timed batch against the CPU port of the reference + the north star's two gates: embeddings
within 1e-4, EER delta < 0.01 % on a 50 000-trial planted-speaker set against the exact-f32 extraction), `cpu_baseline`
(N = 1 only) and, at N = 1, `supplementary` records: the same workload in the f16 / f32x / f32 precision modes (each with
its single-draw gates) and the configs[2] / configs[4] extractors (ECAPA-TDNN C = 1024; ResNet34-SE on fixed 200-frame and on
variable 200..1000-frame utterances) in bf16 / f16 / f32x; `parity_grade` = per model, the fastest mode that passes the 1e-4
embedding gate and the fastest mode that passes the 0.01 % EER gate on EVERY draw of tests/gate_table.py (weight seeds x trial
lists + a 500 000-trial list per seed); `value_parity_grade` = the x-vector's.

`--backend gloo --dry-run` runs the same control flow - self-launch, barriers, MAX over ranks, the double-buffered
asynchronous all-gather, rank 0's JSON line - on CPU ranks with a stand-in extractor (no device, no library): the N > 1
path exercised end to end where no multi-GPU box is available (tests/test_bench_selflaunch_gloo.py).
"""

import argparse
import json
import os
import socket
import subprocess
import sys
import time

# RCCL / device-tensor sharing across the ranks of one node needs dmabuf IPC on these hosts (already exported by the
# launch environment; set here too so a bare `torchrun bench.py` works)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(REPO, "asv-subtools_amd", "pytorch"), REPO, os.path.join(REPO, "tests")]       # tests/: gate_table.py (checker leg)

# dense MFMA peaks, MI355X_MICROARCH.md.  f32x issues 3 bf16 matrix instructions per product: its roofline is the bf16 one / 3.
# f32m: per product one 16-bit matrix instruction (2500) + both corrections in one block-scaled 8-bit instruction of twice the depth at twice
# the rate (~5000 dense, MI355X_MICROARCH.md): 1 / (1 / 2500 + 2 / 5000) = 1250.
PEAK_TFLOPS = {"bf16": 2500.0, "f16": 2500.0, "f32": 157.3, "f32x": 2500.0 / 3.0, "f32m": 1250.0}
GATE_REL, GATE_EER = 1e-4, 0.01          # BASELINE.json north_star: embeddings within 1e-4 relative, EER delta < 0.01 % absolute

MODELS = {
    "xvector": ("xvector.py", "Xvector(%d,10,training=False)", "BASELINE configs[1]: standard TDNN x-vector"),
    "ecapa": ("ecapa_tdnn_xvector.py", "ECAPA_TDNN(%d,10,training=False)", "BASELINE configs[2]: ECAPA-TDNN C=1024"),
    "resnet": ("resnet_xvector.py", "ResNetXvector(%d,10,training=False,resnet_params={'use_se':True,'se_ratio':4,'full_pre_activation':False},"
               "fc2_params={'nonlinearity':'','bn_params':{'momentum':0.5,'affine':False,'track_running_stats':True}})", "BASELINE configs[4] extractor: ResNet34-SE"),
}
KERNEL_NAMES = {"xvector": "frame-level GEMM launches: tdnn_chain_kernel (tdnn3 -> tdnn4 -> tdnn5 -> statistics pooling) + tdnn_gemm_big3 / p8p (tdnn1, tdnn2)",
                "ecapa": "frame-level GEMM launches (tdnn_gemm_p8p_kernel for the wide layers, res2_chain_kernel for the 128-channel ones)",
                "resnet": "frame-level GEMM launches (grid_conv_narrow_pers_kernel / grid_conv_wide_kernel / grid_conv_s2d_kernel / tdnn_gemm_kernel)"}
DOMINANT_NAMES = {"xvector": "tdnn_chain_kernel / tdnn_chainx_kernel:", "ecapa": "tdnn_gemm_p8p / p8x kernel:", "resnet": "grid_conv kernel:"}


LINE_TARGET, LINE_LIMIT = 4096, 8000      # bytes of the final stdout line: the driver parses that line, and a 19 KB one was not held (BENCH_r05)
DUMP_LIMIT = 64 << 20                     # bytes of --dump-outputs at most


def compact_record(res):
    """The ONE line the driver parses: the contract's keys, the dominant kernel's roofline, the CPU baseline and one scalar (+ its
    fraction of the mode's peak) per supplementary model / mode.  Everything else - gate tables, every ark -> ark run, per-launch lists,
    prose - stays in the full record (gpurun_out/bench_full.json and stderr)."""
    def pick(d, keys):
        return {k: d[k] for k in keys if isinstance(d, dict) and k in d and d[k] is not None}

    def num(d, *path):
        for k in path:
            d = d.get(k) if isinstance(d, dict) else None
        return d if isinstance(d, (int, float)) and not isinstance(d, bool) else None

    out = pick(res, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling"))
    out["vs_baseline"] = res.get("vs_baseline")
    out.update(pick(res, ("dtype", "data")))
    cfg = res.get("config", {})
    out["config"] = pick(cfg, ("workload", "global_batch_utts", "frames_per_utt", "parallelism"))
    out["config"]["workload"] = str(cfg.get("workload", ""))[:200]
    if isinstance(cfg.get("streams"), str):
        out["config"]["streams"] = int(cfg["streams"].split()[0])
    rf = res.get("roofline")
    if rf:
        out["roofline"] = pick(rf, ("bound", "kernel", "achieved", "peak", "unit", "frac"))
        out["roofline"]["traffic"] = rf.get("traffic")
        out["roofline"].update(pick(rf, ("dominant_kernel", "dominant_us", "dominant_frac", "dominant_flop_per_launch", "dominant_share_of_gemm_time",
                                         "traffic_algorithmic_bytes", "traffic_over_algorithmic", "all_gemm_launches_tflops", "all_gemm_launches_frac")))
    cb = res.get("cpu_baseline")
    if cb:
        out["cpu_baseline"] = pick(cb, ("value", "unit", "cores", "kind", "value_1_thread"))
        out["cpu_baseline"]["sample"] = str(cb.get("sample", ""))[:160]
    if "value_parity_grade" in res:
        out["value_parity_grade"] = pick(res["value_parity_grade"], ("mode", "value"))
    out.update(pick(res, ("value_single_stream", "value_at_b640", "value_without_event_recording", "dry_run", "gather_verified", "backend")))
    if "collective" in res:
        out["collective"] = pick(res["collective"], ("op", "backend", "world", "verified"))
    par = res.get("parity")
    if par:
        out["parity"] = pick(par, ("max_rel_err", "gate_1e-4", "eer_gate"))
        if num(par, "eer", "eer_delta_percent") is not None:
            out["parity"]["eer_delta_percent"] = par["eer"]["eer_delta_percent"]
    sup = res.get("supplementary") or {}
    flat = {}
    for key, rec in sup.items():
        if key == "ark_to_ark":
            for run, v in (rec.get("runs") or {}).items():                # both clocks: the script's loop and the whole process
                flat["ark_" + run] = pick(v, ("loop_utts_per_s", "end_to_end_utts_per_s")) if "error" not in v else {"error": str(v["error"])[-80:]}
            if "error" in rec:
                flat["ark_to_ark"] = {"error": str(rec["error"])[:80]}
        elif isinstance(rec, dict) and "value" in rec:
            flat[key] = pick(rec, ("value", "frac"))
            if isinstance(rec.get("parity"), dict):
                flat[key]["gates"] = [bool(rec["parity"].get("gate_1e-4")), rec["parity"].get("eer_gate")]
        elif isinstance(rec, dict) and "error" in rec:
            flat[key] = {"error": str(rec["error"])[:80]}
    if flat:
        out["supplementary"] = flat
    pg = res.get("parity_grade")
    if pg:
        out["parity_grade"] = {m: (num(g, "fastest_mode_passing_both", "value") and
                                   {"mode": g["fastest_mode_passing_both"]["mode"], "value": g["fastest_mode_passing_both"]["value"]}) or
                               ({"error": str(g["error"])[:80]} if "error" in g else None) for m, g in pg.items()}
    return out


def emit(res):
    """Rank 0: the full record to gpurun_out/bench_full.json (+ stderr), the compact record as the LAST stdout line."""
    full = json.dumps(res)
    try:
        side = os.path.join(REPO, "gpurun_out")
        os.makedirs(side, exist_ok=True)
        with open(os.path.join(side, "bench_full.json"), "w") as f:
            f.write(full + "\n")
    except OSError as e:
        print("bench.py: full record not written (%s)" % e, file=sys.stderr)
    print("bench.py full record: " + full, file=sys.stderr, flush=True)
    rec = compact_record(res)
    rec["full_record"] = "gpurun_out/bench_full.json (and stderr)"
    line = json.dumps(rec, separators=(",", ":"))
    if len(line) > LINE_TARGET:                                         # first the optional parts, never the contract's keys
        for k in ("parity_grade", "parity", "collective"):
            rec.pop(k, None)
            line = json.dumps(rec, separators=(",", ":"))
            if len(line) <= LINE_TARGET:
                break
    assert len(line) < LINE_LIMIT, "bench line is %d bytes: the driver cannot hold it" % len(line)
    sys.stderr.flush()
    print(line, flush=True)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the embeddings of the last timed step (float32) to DIR/embeddings.npy")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline: repeated timed regions (--min-seconds), hipEvent roofline, "
                         "single-stream pass, HBM traffic, parity and EER gates, supplementary models / modes, parity_grade, cpu_baseline, "
                         "verification of the all-gather")
    ap.add_argument("--precision", default="bf16", help="bf16 (default, BASELINE configs[1]) | f16 | f32x[-bf16|-f16] | f32")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="nccl = RCCL on the GPUs (default); gloo needs --dry-run")
    ap.add_argument("--dry-run", action="store_true",
                    help="CPU ranks, stand-in extractor: exercises self-launch, barriers, the double-buffered all-gather and the JSON line without a device")
    ap.add_argument("--streams", type=int, default=None, choices=[1, 2, 3, 4],
                    help="2 = consecutive steps alternate between two engines (same weights, own activation arenas) on two HIP streams: the small "
                         "launches at the end of step i (pooling merge, pooled affine) overlap the wide GEMMs at the start of step i + 1 "
                         "(default for the x-vector workload: +4.7 %% measured, profiles/r3a_*; the roofline object and `value_single_stream` "
                         "come from a single-stream pass of the same workload)")
    ap.add_argument("--eer-trials", type=int, default=50000, help="trials of the EER gate leg (0 = skip)")
    ap.add_argument("--gate-seeds", type=int, default=3, help="weight seeds of the per-model gate table (parity_grade; 0 = skip)")
    ap.add_argument("--no-traffic", action="store_true", help="skip the two rocprofv3 --pmc passes that measure roofline.traffic (N = 1, default workload)")
    ap.add_argument("--lengths", default=None, help="'lo:hi' = utterance lengths ~ U[lo, hi] (seeded) instead of --frames")
    ap.add_argument("--batch", type=int, default=None,
                    help="utterances per GPU per step (default: 256, what BASELINE configs[1] / [2] / [4] state; the same harness at 640 - whole "
                         "rounds of workgroups - is reported beside it as value_at_b640 / roofline_at_b640)")
    ap.add_argument("--frames", type=int, default=None, help="frames per utterance (default: 200; 300 for --model ecapa, BASELINE configs[2])")
    ap.add_argument("--feat-dim", type=int, default=80)
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="budget of the CPU baseline leg (0 = skip)")
    ap.add_argument("--min-seconds", type=float, default=1.0, help="the K-step timed region is repeated until this much time has been measured")
    ap.add_argument("--no-profile", action="store_true", help="do not record per-kernel hipEvents in the timed region")
    ap.add_argument("--no-supplementary", action="store_true", help="skip the b640 / f32x / f32 / ECAPA / ResNet / ark->ark sub-records")
    ap.add_argument("--ark-utts", type=int, default=50000,
                    help="utterances of the supplementary ark -> ark record (the extraction SCRIPT on a synthetic archive read from the page cache: "
                         "stream and --sharded paths, f32m (the scripts' default) and the headline mode; 0 = skip; tools/bench_pipeline.py runs the same at 50 000)")
    ap.add_argument("--event-stride", type=int, default=8, help="record the per-GEMM hipEvents on every k-th timed step")
    ap.add_argument("--per-op", action="store_true", help="also print a per-op timing table to stderr")
    ap.add_argument("--settle-seconds", type=float, default=0.5,
                    help="untimed steps run for this long before the W warmup steps: the power management needs ~100 ms of sustained load "
                         "to reach the steady clock; the first 100 steps after idle are 30 %% slower than the steady state")
    ap.add_argument("--from-wav", action="store_true",
                    help="start every step from 16-bit PCM in HBM: asv_fbank_pcm16 (log-mel, --feat-dim bins) + asv_cmvn + extraction "
                         "(SURVEY.md 8(f) rank 2; the headline metric starts from feature matrices, this is a supplementary line)")
    ap.add_argument("--model", default="xvector", choices=sorted(MODELS),
                    help="xvector = BASELINE configs[1] (the default, the contract's workload); ecapa = configs[2] (C=1024, 300 frames); "
                         "resnet = the configs[4] extractor (ResNet34-SE)")
    return ap.parse_args()


def measure_traffic(kernel_sub="tdnn_chain_kernel", timeout_s=150):
    """HBM traffic of the dominant kernel, measured in THIS run: two short passes of this same script under rocprofv3, one counter
    each (FETCH_SIZE and WRITE_SIZE do not share a pass on gfx950), collected and corrected as MI355X_MICROARCH.md prescribes - KiB per
    dispatch, the read side doubled (gfx950 reports half the bytes of wide streaming reads), the write side as is - and averaged over
    the kernel's dispatches.  Returns (bytes per launch, detail dict) or (None, {"error": ...}); never raises."""
    import csv
    import glob
    import shutil
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, {"error": "rocprofv3 not found"}
    got = {}
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            d = tempfile.mkdtemp(prefix="asv_pmc_", dir="/tmp")
            cmd = [exe, "--pmc", counter, "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                   "--steps", "4", "--warmup", "2", "--no-profile", "--min-seconds", "0.05", "--settle-seconds", "0.2", "--streams", "1", "--cpu-seconds", "0",
                   "--no-supplementary", "--eer-trials", "0", "--no-traffic"]
            env = dict(os.environ, TMPDIR="/tmp")
            r = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout_s)
            vals = []
            for path in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                with open(path) as f:
                    for row in csv.DictReader(f):
                        if row.get("Counter_Name") == counter and kernel_sub in row.get("Kernel_Name", ""):
                            vals.append(float(row["Counter_Value"]))
            shutil.rmtree(d, ignore_errors=True)
            if not vals:
                return None, {"error": "%s pass: no dispatches of %s in the counter file (rc %d): %s" % (counter, kernel_sub, r.returncode, r.stderr.decode(errors="replace")[-300:])}
            got[counter] = (1024.0 * sum(vals) / len(vals), len(vals))
    except Exception as e:                                        # a counter pass must never take the bench line down
        return None, {"error": "%s: %s" % (type(e).__name__, e)}
    fetch_b, write_b = 2.0 * got["FETCH_SIZE"][0], got["WRITE_SIZE"][0]
    return fetch_b + write_b, {"fetch_bytes_per_launch_corrected": round(fetch_b), "write_bytes_per_launch": round(write_b), "dispatches": got["FETCH_SIZE"][1],
                               "source": "measured in this run: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate passes of this script, 4 steps each), "
                                         "FETCH_SIZE x 2 (gfx950), averaged over the dispatches of " + kernel_sub}


def self_launch(args):
    """`python bench.py --gpus N` with N > 1 and no launcher environment: re-execute under torch.distributed.run, one rank
    per GPU, rendezvous on 127.0.0.1 (the container hostname may not resolve)."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd)


class Workload(object):
    """One model in one precision mode on this rank's device, with a device-resident synthetic batch."""

    def __init__(self, args, kind, precision, batch, frames, rank, dev, lengths=None):
        import numpy as np
        import torch
        import libs.support.utils as utils
        from libs.amd import synth
        self.kind, self.precision, self.B, self.T, self.D = kind, precision, batch, frames, args.feat_dim
        blueprint, creation, self.title = MODELS[kind]
        self.creation = creation % args.feat_dim
        model = utils.create_model_from_py(os.path.join(REPO, "asv-subtools_amd", "pytorch", "model", blueprint), self.creation)
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        self.sd = synth.synth_state_dict(shapes, 0)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in self.sd.items()})
        model.eval()
        model.cuda()
        model.amd_precision = precision
        self.model, self.eng = model, model._amd_engine()
        # fixed length (the BASELINE configs[1..2] shapes) or seeded U[lo, hi] lengths (configs[4]: 200..1000 frames), packed ragged
        self.lengths = np.full(batch, frames, dtype=np.int64) if lengths is None else synth.synth_lengths(batch, lengths[0], lengths[1], 77 + rank)
        self.mats = [synth.synth_feats(int(t), self.D, 10_000 * rank + i) for i, t in enumerate(self.lengths)]
        self.feats = torch.from_numpy(np.concatenate(self.mats, axis=0)).to(dev)
        self.offsets = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int32)
        self.frames_total = int(self.lengths.sum())
        self.dev = dev

    def extract(self, out):
        self.eng.extract_device(self.feats, self.offsets, out=out)


class DryRunEngine(object):
    """Stand-in for libs.amd.engine.Engine in --dry-run: the same call surface on CPU tensors, trivially cheap arithmetic."""
    embed_dim = 32

    def extract_device(self, feats, offsets, out=None, **kw):
        import torch
        idx = torch.repeat_interleave(torch.arange(len(offsets) - 1), torch.as_tensor(offsets[1:] - offsets[:-1]).long())
        acc = torch.zeros((len(offsets) - 1, feats.shape[1]), dtype=torch.float32).index_add_(0, idx, feats)
        res = acc[:, :self.embed_dim]
        if out is not None:
            out.copy_(res)
            return out
        return res

    def set_profiling(self, enable):
        pass

    def get_profile(self):
        return []


class DryRunWorkload(object):
    def __init__(self, args, batch, frames, rank):
        import numpy as np
        import torch
        self.kind, self.precision, self.B, self.T, self.D = "xvector", "dry-run", batch, frames, args.feat_dim
        self.title, self.creation = "dry run (stand-in extractor on CPU ranks, no device)", "none"
        self.eng = DryRunEngine()
        r = np.random.RandomState(1000 + rank)
        self.feats = torch.from_numpy(r.randn(batch * frames, max(self.D, DryRunEngine.embed_dim)).astype(np.float32))
        self.offsets = (np.arange(batch + 1) * frames).astype(np.int32)
        self.lengths = np.full(batch, frames, dtype=np.int64)
        self.frames_total = batch * frames
        self.mats, self.sd = None, None

    def extract(self, out):
        self.eng.extract_device(self.feats, self.offsets, out=out)


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))
    import numpy as np
    import torch
    import torch.distributed as dist
    from libs.amd import synth

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.exit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    dry = args.dry_run
    # Under a launcher (torch.distributed.run sets RANK / WORLD_SIZE / MASTER_PORT) the process group is initialised and the
    # all-gather runs at ANY world size, 1 included: `python -m torch.distributed.run --nproc-per-node 1 bench.py --gpus 1` is the
    # one-GPU proof that RCCL loads and moves the embeddings (tests/test_gpu_rccl.py).  Plain `python bench.py` stays collective-free.
    dist_on = world > 1 or ("RANK" in os.environ and "MASTER_PORT" in os.environ)
    if args.backend == "gloo" and not dry:
        sys.exit("bench.py: --backend gloo is the CPU dry run of the multi-rank control flow: pass --dry-run")
    if dry:
        dev = torch.device("cpu")
        if dist_on:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group(backend="gloo")
    else:
        assert torch.cuda.is_available(), "bench.py needs a ROCm device"
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
        if dist_on:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC for RCCL on these hosts
            dist.init_process_group(backend="nccl", device_id=dev)      # "nccl" is RCCL on ROCm

    def dev_sync():
        if not dry:
            torch.cuda.synchronize(dev)

    if args.frames is None:
        args.frames = 300 if args.model == "ecapa" else 200
    if args.batch is None:
        args.batch = 256                                             # BASELINE configs[1] / [2] / [4]: 256 utterances per step

    SIDE_STREAMS = []

    def measure(wl, steps, warmup, min_seconds, profile, collective, per_op=False, from_wav=False, wl2=None):
        """wl2: None, or a list of further Workloads (same model, own engines): consecutive steps rotate over [wl] + wl2 on one HIP
        stream each."""
        """settle -> warmup -> `repeats` timed regions of exactly `steps` steps (barrier + synchronize on both sides, MAX over
        ranks); returns the record of the median region."""
        eng, B = wl.eng, wl.B
        # two (or one per engine) output / gather buffer pairs: the all-gather of step i runs on RCCL's stream while step i+1 computes
        engines = [wl] + list(wl2 or [])
        nbuf = max(2, len(engines))
        outs = [torch.empty((B, eng.embed_dim), dtype=torch.float32, device=dev) for _ in range(nbuf)]
        gathered = [torch.empty((world * B, eng.embed_dim), dtype=torch.float32, device=dev) for _ in range(nbuf)] if collective else None
        pending, counter = [None] * nbuf, [0]
        if from_wav:
            from libs.amd import frontend
            n_samp = 400 + (wl.T - 1) * 160                             # 25 ms windows, 10 ms shift at 16 kHz: exactly T frames
            wave_dev = torch.from_numpy(np.concatenate([synth.synth_wave(n_samp, 10_000 * rank + i).astype(np.int16) for i in range(B)])).to(dev)
            sample_off = np.arange(B + 1, dtype=np.int64) * n_samp
            fe_kw = dict(num_mel_bins=wl.D, energy_floor=0.0, mean_norm=True)

        def extract_once(out):
            if from_wav:
                f, _ = frontend.fbank_device(wave_dev, sample_off, **fe_kw)
                eng.extract_device(f, wl.offsets, out=out)
            else:
                wl.extract(out)

        # One set of side streams per process, reused by every two-stream measurement.  Measured (profiles/r3q_b256_streams.txt): the
        # first pair of torch pool streams a process uses runs its kernels side by side; a SECOND pair taken later (what every
        # supplementary record did until round 3's last build) does not - 750 k instead of 931 k utt/s for the 256-utterance
        # record, below its own single-stream figure.  BENCH_NEW_STREAMS=1 restores a fresh pair per measurement (A/B aid).
        if wl2:
            while len(SIDE_STREAMS) < len(engines) or os.environ.get("BENCH_NEW_STREAMS"):
                SIDE_STREAMS.append(torch.cuda.Stream(device=dev))
                if len(SIDE_STREAMS) >= 64:
                    break
        side = (SIDE_STREAMS[-len(engines):] if os.environ.get("BENCH_NEW_STREAMS") else SIDE_STREAMS[:len(engines)]) if wl2 else None

        def step():
            k = counter[0] % nbuf
            counter[0] += 1
            if side is not None:
                # one engine per stream: step i + 1 starts while the tail of step i is still running
                with torch.cuda.stream(side[k]):
                    if pending[k] is not None:                          # THIS stream waits until the gather that reads outs[k] has finished
                        pending[k].wait()
                        pending[k] = None
                    engines[k].extract(outs[k])
                    if collective:
                        pending[k] = dist.all_gather_into_tensor(gathered[k], outs[k], async_op=True)
                return
            if pending[k] is not None:                                  # buffer pair k is free once its gather has finished
                pending[k].wait()                                       # (stream-side wait, the host does not block)
                pending[k] = None
            extract_once(outs[k])
            if collective:
                pending[k] = dist.all_gather_into_tensor(gathered[k], outs[k], async_op=True)

        def barrier():
            for k in range(nbuf):
                if pending[k] is not None:
                    pending[k].wait()
                    pending[k] = None
            dev_sync()
            if dist_on:
                dist.barrier()
                dev_sync()

        def timed(n, sample_events=0):
            """sample_events = k > 0: per-GEMM hipEvents are recorded on every k-th step of the timed region
            (each recorded event is a barrier packet between kernels; sampling keeps that perturbation small)."""
            barrier()
            t0 = time.perf_counter()
            for i in range(n):
                if sample_events:
                    eng.set_profiling(4 if i % sample_events == 0 else 0)
                step()
            barrier()
            dt = time.perf_counter() - t0
            if dist_on:
                t = torch.tensor([dt], dtype=torch.float64, device=dev)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                dt = float(t.item())
            return dt

        t_settle = time.perf_counter()
        while time.perf_counter() - t_settle < args.settle_seconds:       # untimed: bring the device to its steady clock
            for _ in range(50):
                extract_once(outs[0])                                    # local work only: the count differs between ranks,
            dev_sync()                                   # so no collective may be issued here
        for _ in range(warmup):
            step()
        barrier()
        if args.full:
            # one probe region decides how many regions make up min_seconds (the same number on every rank)
            probe = timed(steps)
            repeats = max(3, int(min_seconds / max(probe, 1e-6)) + 1)
        else:
            repeats = 1                                                 # a plain run times exactly `steps` steps
        stride = max(1, args.event_stride)
        rows = []
        if profile:
            eng.set_profiling(4)                                        # one hipEvent pair around each run of frame-level GEMM launches
            # create the whole event pool outside the timed regions: one profiled step per step that will be sampled
            # (hipEventCreate inside the timed steps cost 5-30 % of the measured rate, erratically)
            for _ in range((steps + stride - 1) // stride):
                step()
            barrier(); eng.get_profile()
        # every 4th region samples hipEvents; the others run bare.  Both kinds are K-step regions under the contract's timing.
        dts, dts_sampled = [], []
        for r in range(repeats):
            sampled = profile and (r % 4 == 0)
            dt = timed(steps, sample_events=stride if sampled else 0)
            (dts_sampled if sampled else dts).append(dt)
            if sampled:
                rows.extend(eng.get_profile())
        eng.set_profiling(False)
        # what the caller of the last timed step received (later profiled steps reuse the buffers)
        output = (gathered if collective else outs)[(counter[0] - 1) % nbuf].clone()
        gather_ok = None
        if args.full and dry and collective:
            # the dry run also checks WHAT the double-buffered gather delivered: every rank's block of the last two steps
            # against that rank's stand-in result, recomputed here from its seed
            barrier()
            want = torch.cat([DryRunWorkload(args, B, wl.T, r).eng.extract_device(DryRunWorkload(args, B, wl.T, r).feats, wl.offsets) for r in range(world)])
            gather_ok = all(bool(torch.equal(g, want)) for g in gathered)
        elif args.full and collective:
            # on the device: this rank's block of what the last all-gathers delivered equals its own embeddings, bit for bit
            barrier()
            gather_ok = all(bool(torch.equal(gathered[k][rank * B:(rank + 1) * B], outs[k])) for k in range(nbuf) if counter[0] > k)
        allr = sorted(dts + dts_sampled)
        med = allr[len(allr) // 2]
        rec = {"value": round(world * B * steps / med, 1), "ms_per_step": round(1e3 * med / steps, 4), "repeats": len(allr),
               "timed_seconds": round(sum(allr), 3),
               "ms_per_step_min_max": [round(1e3 * allr[0] / steps, 4), round(1e3 * allr[-1] / steps, 4)], "output": output}
        if gather_ok is not None:
            rec["gather_verified"] = gather_ok
        if dts and dts_sampled:
            rec["value_without_event_recording"] = round(world * B * steps / sorted(dts)[len(dts) // 2], 1)
        gemm_ms = sum(r["total_ms"] for r in rows if r["name"] == "tdnn_gemm")
        gemm_fl = sum(r["flops"] for r in rows if r["name"] == "tdnn_gemm")
        gemm_n = sum(r["launches"] for r in rows if r["name"] == "tdnn_gemm")
        if gemm_ms > 0:
            achieved = gemm_fl / (gemm_ms * 1e-3) / 1e12
            peak = PEAK_TFLOPS[wl.precision.split("-")[0]]
            per_frame, per_utt = eng.graph.flops_per_frame()
            sampled_steps = len(dts_sampled) * ((steps + stride - 1) // stride)
            rec["roofline"] = {"bound": "mfma", "kernel": KERNEL_NAMES[wl.kind], "achieved": round(achieved, 2), "peak": round(peak, 1),
                               "unit": "TFLOP/s", "frac": round(achieved / peak, 4), "traffic": None,
                               "launches": gemm_n, "avg_launch_us": round(1e3 * gemm_ms / gemm_n, 2),
                               "algorithmic_gflop_per_utt": round((per_frame * wl.frames_total / wl.B + per_utt) / 1e9, 4), "sampled_steps": sampled_steps,
                               "gemm_ms_per_step": round(gemm_ms / sampled_steps, 4)}
        if profile and rank == 0 and "roofline" in rec:
            # every frame-level GEMM launch on its own (one hipEvent pair per launch: a few untimed steps after the timed regions)
            eng.set_profiling(2)
            for _ in range(8):
                step()
            dev_sync()
            ops = getattr(eng, "ops", eng.graph.ops)
            per = []
            for r in sorted(eng.get_profile(), key=lambda r: r["op_index"]):
                if r["name"] != "tdnn_gemm" or r["total_ms"] <= 0:
                    continue
                i = r["op_index"]
                what = "op %d" % i
                if 0 <= i < len(ops) and ops[i].kind == "tdnn":
                    own = 2.0 * wl.frames_total * ops[i].inp.channels * ops[i].out.channels * len(ops[i].taps)      # this layer alone, per launch
                    chained = wl.kind == "xvector" and r["flops"] / max(r["launches"], 1) > 1.5 * own
                    what = "%d->%d taps=%d%s" % (ops[i].inp.channels, ops[i].out.channels, len(ops[i].taps), " + the layers chained behind it (tdnn_chain_kernel)" if chained else "")
                elif 0 <= i < len(ops) and ops[i].kind == "res2":
                    what = "res2 %d x 128->128" % ops[i].branches
                us = 1e3 * r["total_ms"] / max(r["launches"], 1)
                per.append({"layer": what, "us": round(us, 1), "tflops": round(r["flops"] / (r["total_ms"] * 1e-3) / 1e12, 1)})
            if len(per) <= 12:
                rec["roofline"]["per_launch"] = per
            if per:
                # the dominant kernel as FLAT scalars (a list does not survive the driver's parse of this line - VERDICT r4 item 6):
                # the launch with the most algorithmic FLOPs, its own hipEvent-timed duration and its own fraction of the peak
                dom = max(per, key=lambda q: q["us"] * q["tflops"])
                # `roofline.achieved` / `.frac` ARE the dominant kernel's (algorithmic FLOPs of one launch / its hipEvent-timed duration); the
                # figure over all frame-level GEMM launches of the step stays beside it
                rec["roofline"].update({"all_gemm_launches_tflops": rec["roofline"]["achieved"], "all_gemm_launches_frac": rec["roofline"]["frac"],
                                        "achieved": dom["tflops"], "frac": round(dom["tflops"] / peak, 4), "kernel": DOMINANT_NAMES.get(wl.kind, "") + " " + dom["layer"]})
                rec["roofline"].update({"dominant_kernel": dom["layer"], "dominant_us": dom["us"], "dominant_tflops": dom["tflops"],
                                        "dominant_frac": round(dom["tflops"] / peak, 4),
                                        "dominant_flop_per_launch": round(dom["us"] * 1e-6 * dom["tflops"] * 1e12),
                                        "dominant_share_of_gemm_time": round(dom["us"] / max(sum(q["us"] for q in per), 1e-9), 4)})
            eng.set_profiling(False)
            barrier()
        if per_op and rank == 0:
            eng.set_profiling(2)
            for _ in range(steps):
                step()
            dev_sync()
            ops = getattr(eng, "ops", eng.graph.ops)
            for r in sorted(eng.get_profile(), key=lambda r: r["op_index"]):
                i = r["op_index"]
                desc = ""
                if 0 <= i < len(ops) and ops[i].kind == "tdnn":
                    desc = "%d->%d taps=%s" % (ops[i].inp.channels, ops[i].out.channels, ops[i].taps)
                elif 0 <= i < len(ops) and ops[i].kind == "res2":
                    desc = "res2 %d x 128->128 dilation %d" % (ops[i].branches, ops[i].dilation)
                us = 1e3 * r["total_ms"] / max(r["launches"], 1)
                tf = r["flops"] / (r["total_ms"] * 1e-3) / 1e12 if r["total_ms"] > 0 else 0.0
                print("  op %3d %-14s %-28s %9.1f us  %8.1f TFLOP/s" % (i, r["name"], desc, us, tf), file=sys.stderr)
            eng.set_profiling(False)
            barrier()
        return rec

    def parity_of(wl, n=4):
        """A few utterances of the timed batch against the CPU port of the reference's call sequence (checker leg only;
        x-vector only - the port restates model/xvector.py).  `gate_1e-4`: the north star's embedding gate on that sample."""
        from oracle import torch_cpu_port as P
        ex = P.XvectorCpu(wl.sd, "far")
        pos = sorted({min(q, wl.B - 1) for q in (0, 1, wl.B // 2, wl.B - 1)})[:n]         # (a batch of one or two utterances: fewer positions)
        got = wl.eng.extract_device(wl.feats, wl.offsets).cpu().numpy()[pos]
        want = np.stack([ex.extract_embedding(wl.mats[i]).numpy() for i in pos])
        rel = float(np.abs(got - want).max() / np.abs(want).max())
        cos = float(((got * want).sum(1) / np.linalg.norm(got, axis=1) / np.linalg.norm(want, axis=1)).min())
        return {"max_rel_err": float("%.3g" % rel), "min_cosine": round(cos, 6), "n": len(pos), "gate_1e-4": bool(rel < GATE_REL),
                "against": "oracle/torch_cpu_port.py (the reference's torch CPU call "
                "sequence, pinned to the reference's own outputs by tests/test_oracle_golden.py)", "metric": "max|a-b| / max|b| over the sampled embeddings"}

    eer_state = {}

    def eer_gate_of(wl):
        """The north star's second gate for this workload's precision mode: |EER(mode) - EER(exact-f32 extraction)| on the
        planted-speaker set of tests/test_gpu_eer_gate.py (4 708 utterances of 200..500 frames, args.eer_trials trials, cosine
        scoring: sub-mean, length-norm, dot products).  The f32 extraction is the reference-equivalent one (tied to the oracle
        by the -m gpu tests).  Checker leg: not timed."""
        from libs.amd import scoring
        if "mats" not in eer_state:
            mats, labels = synth.synth_planted_utts(1177, 4, wl.D, 200, 500, 0.8)
            eer_state["mats"] = mats
            eer_state["trials"] = synth.synth_trials(labels, args.eer_trials, seed=41)
            order = np.argsort([-m.shape[0] for m in mats], kind="stable")
            batches, i = [], 0
            while i < len(order):
                j, frames = i, 0
                while j < len(order) and (j == i or frames + mats[order[j]].shape[0] <= 130_000):
                    frames += mats[order[j]].shape[0]
                    j += 1
                idx = order[i:j]
                offs = np.concatenate([[0], np.cumsum([mats[k].shape[0] for k in idx])]).astype(np.int32)
                batches.append((idx, torch.from_numpy(np.concatenate([mats[k] for k in idx], axis=0)).to(dev), offs))
                i = j
            eer_state["batches"] = batches

        def extract_all(eng):
            out = torch.empty((len(eer_state["mats"]), eng.embed_dim), dtype=torch.float32, device=dev)
            for idx, feats, offs in eer_state["batches"]:
                out[torch.as_tensor(idx, device=dev)] = eng.extract_device(feats, offs)
            return out

        def eer_of(emb):
            ei, ti, tgt = eer_state["trials"]
            e = scoring.length_normalize(emb, scoring.mean_vector(emb))
            sc = scoring.score_trials(e, e, ei, ti)
            return scoring.eer(sc, tgt)[0], sc

        if "ref" not in eer_state:
            wl.model.amd_precision = "f32"
            eer_state["ref"] = eer_of(extract_all(wl.model._amd_engine()))
            wl.model.amd_precision = wl.precision
        eer_ref, sc_ref = eer_state["ref"]
        eer_new, sc_new = eer_of(extract_all(wl.eng))
        delta = float(eer_new - eer_ref)
        return {"eer_percent": round(float(eer_new), 4), "eer_f32_percent": round(float(eer_ref), 4), "eer_delta_percent": round(delta, 4),
                "max_abs_score_delta": float("%.3g" % float((sc_new - sc_ref).abs().max().item())), "trials": int(args.eer_trials),
                "utterances": len(eer_state["mats"]), "gate_0.01": bool(abs(delta) < GATE_EER)}

    def gates_of(wl):
        rec = parity_of(wl)
        if args.eer_trials > 0:
            rec["eer"] = eer_gate_of(wl)
            rec["eer_gate"] = rec["eer"]["gate_0.01"]
        return rec

    # ---- the headline workload ------------------------------------------------------------------
    if dry:
        wl = DryRunWorkload(args, args.batch, args.frames, rank)
    else:
        lengths = tuple(int(v) for v in args.lengths.split(":")) if args.lengths else None
        wl = Workload(args, args.model, args.precision, args.batch, args.frames, rank, dev, lengths=lengths)
    if args.streams is None:
        # two engines on two streams fill the CUs a partly filled last round of tiles leaves idle: +12 % for the f32x mode at 256
        # utterances per step too (288 k -> 321 k, profiles/r4e_f32x_streams.txt); at 640 (whole rounds) it costs that mode 3 %
        one_only = ("f32",) if args.batch <= 320 else ("f32x", "f32m", "f32")
        args.streams = 2 if (not dry and not args.from_wav and not args.per_op and args.precision.split("-")[0] not in one_only) else 1
    wl2 = [Workload(args, args.model, args.precision, args.batch, args.frames, rank, dev, lengths=lengths) for _ in range(args.streams - 1)] if (args.streams >= 2 and not dry) else None
    head = measure(wl, args.steps, args.warmup, args.min_seconds, args.full and not args.no_profile and not dry and wl2 is None, dist_on, per_op=args.per_op,
                   from_wav=args.from_wav, wl2=wl2)
    if args.dump_outputs and rank == 0:
        emb = head["output"].cpu().numpy().astype(np.float32)
        if emb.nbytes > DUMP_LIMIT:                                      # a fixed subset of rows: the same in every run
            emb = emb[np.linspace(0, len(emb) - 1, DUMP_LIMIT // emb[0].nbytes).astype(np.int64)]
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "embeddings.npy"), emb)
    single = None
    if wl2 is not None and args.full:
        # the kernel-level figures (roofline: hipEvents around the GEMM launches of ONE stream) come from a single-stream pass
        single = measure(wl, args.steps, 2, min(args.min_seconds, 0.6), not args.no_profile, dist_on)
        if "roofline" in single:
            head["roofline"] = single["roofline"]
    res = {
        "metric": "utterances/sec (200-frame) embedding extraction + EER, 1/2/4/8 MI355X",
        "value": head["value"], "unit": "utterances/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": head["ms_per_step"],
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": args.precision, "data": "synthetic",
        "config": {"workload": "%s: %s, %d-dim fbank, %d utterances x %s frames per GPU per step, "
                               "%s resident in HBM, f32 embeddings out%s" % (wl.title, wl.creation, wl.D, wl.B, ("%d" % wl.T) if not args.lengths else "U[%s]" % args.lengths,
                                                                             "16-bit PCM (fbank + CMN computed on the device in every step)" if args.from_wav else "features",
                                                                             ", + RCCL all-gather of embeddings" if dist_on else ""),
                   "global_batch_utts": world * wl.B, "frames_per_utt": wl.T if not args.lengths else round(wl.frames_total / wl.B, 1),
                   "parallelism": "utterance shards x%d" % world},
        "timing": {"regions": head["repeats"], "steps_per_region": args.steps, "timed_seconds": head["timed_seconds"], "value_from": "median region",
                   "ms_per_step_min_max": head["ms_per_step_min_max"]},
        "settle_seconds": args.settle_seconds,
    }
    if single is not None:
        res["value_single_stream"] = single["value"]
        res["ms_per_step_single_stream"] = single["ms_per_step"]
    if wl2 is not None:
        res["config"]["streams"] = "%d engines on %d HIP streams, consecutive steps rotate over them (software pipelining across batches; every step is a full pass)" % (args.streams, args.streams)
    if dist_on and not dry:
        res["collective"] = {"op": "all_gather_into_tensor", "backend": dist.get_backend(), "world": world, "verified": head.get("gather_verified")}
    if dry:
        res["dry_run"] = True
        if "gather_verified" in head:
            res["gather_verified"] = head["gather_verified"]
        res["dtype"] = "none"
        res["backend"] = args.backend
        res["config"]["workload"] = "DRY RUN of the control flow on %d CPU rank(s), backend %s: stand-in extractor, %d x %d rows per step%s - not a measurement" % (
            world, args.backend if world > 1 else "none", wl.B, wl.T, ", + all-gather of embeddings" if world > 1 else "")
    if "value_without_event_recording" in head:
        res["value_without_event_recording"] = head["value_without_event_recording"]
    if "roofline" in head:
        res["roofline"] = head["roofline"]
        res["gemm_ms_per_step"] = head["roofline"].pop("gemm_ms_per_step")
        if args.model == "xvector" and args.precision == "bf16":
            # strictly algorithmic bytes of one chain-kernel launch: the 512-channel 16-bit input rows once, the three layers' weights
            # once, the pooled statistics out
            rows = wl.B * (wl.T + 4) + 4
            alg = rows * 512 * 2 + (3 * 512 * 512 + 512 * 512 + 512 * 1536) * 2 + wl.B * 2 * 1500 * 4
            res["roofline"]["traffic_algorithmic_bytes"] = alg
            traffic, detail = (None, {"error": "skipped (--no-traffic)"})
            if world == 1 and not args.no_traffic and not args.lengths and not args.from_wav:
                traffic, detail = measure_traffic()
            if traffic is not None:
                res["roofline"]["traffic"] = round(traffic)
                res["roofline"]["traffic_over_algorithmic"] = round(traffic / alg, 3)
                res["roofline"]["traffic_source"] = detail
            else:
                # fall back to the committed passes of the same command (tools/collect_profiles.sh -> tools/pmc_summary.py)
                pmc = os.path.join(REPO, "profiles", "pmc_summary.json")
                if os.path.exists(pmc):
                    with open(pmc) as f:
                        info = json.load(f)
                    res["roofline"]["traffic"] = info.get("traffic_bytes_per_launch")
                    res["roofline"]["traffic_source"] = {"static": "profiles/pmc_summary.json (" + str(info.get("source")) + "; library build " + str(info.get("library_sha256_16")) +
                                                         ", batch of that collection: " + str(info.get("batch", 640)) + ")", "live_pass": detail}

    modes = {}
    if args.full and rank == 0 and args.model == "xvector" and not dry and not args.lengths:
        res["parity"] = gates_of(wl) if (world == 1 and not args.from_wav) else parity_of(wl)
        modes[args.precision] = {"value": head["value"], "gate_1e-4": res["parity"]["gate_1e-4"], "eer_gate": res["parity"].get("eer_gate")}
    if args.full and rank == 0 and world == 1 and not args.no_supplementary and args.model == "xvector" and not args.from_wav and not dry and not args.lengths:
        # ---- supplementary records, same harness (shorter: 0.4 s of timed regions each) --------------
        sup = {}
        two = args.streams >= 2

        def record(kind, prec, batch, frames, lens=None, steps=None, min_s=0.4, f32x_single=True):
            """One sub-record: `value` as the headline is measured (two engines on two streams unless --streams 1; the f32x / f32
            modes gain nothing from it - their steps are one long matrix-bound launch sequence - and run on one), the kernel
            figures from a single-stream pass."""
            steps = steps or args.steps
            use_two = two and not (f32x_single and prec.split("-")[0] in (("f32",) if (kind == "xvector" and batch <= 320) else ("f32x", "f32m", "f32")))
            w = Workload(args, kind, prec, batch, frames, rank, dev, lengths=lens)
            w2 = [Workload(args, kind, prec, batch, frames, rank, dev, lengths=lens)] if use_two else None
            r1 = measure(w, steps, 2, min_s, not args.no_profile, False)
            r = measure(w, steps, 2, min_s, False, False, wl2=w2) if use_two else r1
            rec = {"value": r["value"], "unit": "utterances/s", "ms_per_step": r["ms_per_step"], "streams": 2 if use_two else 1}
            if use_two:
                rec["value_single_stream"] = r1["value"]
            if "roofline" in r1:
                rec["gemm_tflops"] = r1["roofline"]["achieved"]
                rec["frac"] = r1["roofline"]["frac"]
                rec["mode_peak_tflops"] = r1["roofline"]["peak"]
                rec["avg_launch_us"] = r1["roofline"]["avg_launch_us"]
                rec["algorithmic_gflop_per_utt"] = r1["roofline"]["algorithmic_gflop_per_utt"]
                rec["whole_step_tflops"] = round(rec["algorithmic_gflop_per_utt"] * r["value"] / 1e3, 1)
                for k in ("dominant_kernel", "dominant_us", "dominant_tflops", "dominant_frac", "dominant_flop_per_launch", "dominant_share_of_gemm_time"):
                    if k in r1["roofline"]:
                        rec[k] = r1["roofline"][k]
            return rec, w

        if wl.B != 640:
            rec, w640 = record("xvector", args.precision, 640, args.frames)
            res["value_at_b640"] = rec["value"]
            if "value_single_stream" in rec:
                res["value_at_b640_single_stream"] = rec["value_single_stream"]
            if "frac" in rec:
                res["roofline_at_b640"] = {"achieved": rec["gemm_tflops"], "peak": rec["mode_peak_tflops"], "unit": "TFLOP/s", "frac": rec["frac"], "avg_launch_us": rec["avg_launch_us"],
                                           "whole_step_frac": round(rec["whole_step_tflops"] / rec["mode_peak_tflops"], 4)}
            res["config"]["batch_note"] = ("`value` is BASELINE configs[1] as stated: 256 utterances per step (408 row tiles of 128 frames on 256 CUs: 1.6 rounds of workgroups "
                                           "per launch); value_at_b640 / roofline_at_b640: the same harness at 640 utterances per step (whole rounds)")
            del w640
        for prec in ("f16", "f32m", "f32x", "f32"):
            if prec == args.precision:
                continue
            rec, w = record("xvector", prec, args.batch, args.frames)
            rec["parity"] = gates_of(w)
            rec["frac_of_mode_peak"] = rec.get("frac")
            sup["xvector_" + prec] = rec
            modes[prec] = {"value": rec["value"], "gate_1e-4": rec["parity"]["gate_1e-4"], "eer_gate": rec["parity"].get("eer_gate")}
            del w
        for kind, key, frames, prec, lens in (("ecapa", "ecapa_c3", 300, args.precision, None), ("ecapa", "ecapa_c3_f16", 300, "f16", None), ("ecapa", "ecapa_c3_f32x", 300, "f32x", None), ("ecapa", "ecapa_c3_f32m", 300, "f32m", None),
                                              ("resnet", "resnet_c5_t200", 200, args.precision, None), ("resnet", "resnet_c5", 600, args.precision, (200, 1000)),
                                              ("resnet", "resnet_c5_f16", 600, "f16", (200, 1000)), ("resnet", "resnet_c5_f32x", 600, "f32x", (200, 1000))):
            try:
                rec, w = record(kind, prec, 256, frames, lens, steps=max(4, args.steps // 4), f32x_single=(kind == "resnet"))
                shape = "%d frames" % frames if lens is None else "U[%d, %d] frames (packed ragged, %d frames in all)" % (lens[0], lens[1], w.frames_total)
                rec["frames_per_s"] = round(rec["value"] * w.frames_total / w.B, 0)
                rec["workload"] = "%s: %s, 256 utterances x %s, %s" % (w.title, w.creation, shape, prec)
                sup[key] = rec
                del w
            except Exception as e:                                        # a supplementary record must never take the headline down
                sup[key] = {"error": "%s: %s" % (type(e).__name__, e)}
        if args.ark_utts > 0:
            # SURVEY 8(d) "then also ark->ark": the drop-in script itself (subprocesses of its own: reader thread / native loaders,
            # page-locked buffers, H2D, two engines, D2H, ark writer), not timed inside the headline region
            try:
                sys.path.insert(0, os.path.join(REPO, "tools"))
                import bench_pipeline
                sup["ark_to_ark"] = bench_pipeline.measure(args.ark_utts, 200, tuple(dict.fromkeys(("f32m", args.precision))), ("stream", "sharded"),
                                                           directory=os.path.join("/tmp", "asv_pipe_%d" % os.getpid()))
            except Exception as e:                                        # a supplementary record must never take the headline down
                sup["ark_to_ark"] = {"error": "%s: %s" % (type(e).__name__, e)}
        res["supplementary"] = sup
    if modes and args.gate_seeds > 0 and "supplementary" in res:
        # The gates as statistics (tests/gate_table.py: checker leg, not timed): per model, every mode on `gate_seeds` weight seeds x 3
        # trial lists + one 500 000-trial list per seed against the exact-f32 extraction of the same engine family.  A mode is
        # "EER grade" only if it is inside 0.01 % on EVERY draw.
        import gate_table
        sup = res["supplementary"]
        rate = {"xvector": {args.precision: res["value"]}, "ecapa": {}, "resnet": {}}
        for prec in ("f16", "f32m", "f32x", "f32"):
            if "xvector_" + prec in sup and "value" in sup["xvector_" + prec]:
                rate["xvector"][prec] = sup["xvector_" + prec]["value"]
        for model, stem in (("ecapa", "ecapa_c3"), ("resnet", "resnet_c5")):
            for prec, key in ((args.precision, stem), ("f16", stem + "_f16"), ("f32x", stem + "_f32x"), ("f32m", stem + "_f32m")):
                if key in sup and "value" in sup[key]:
                    rate[model][prec] = sup[key]["value"]
        grade = {}
        for model in ("xvector", "ecapa", "resnet"):
            try:
                t0 = time.perf_counter()
                g = gate_table.Gates(model, feat_dim=args.feat_dim, device=dev)
                tab = g.table([p for p in ("f32x", "f32m", "f16", "bf16") if p in rate[model]], weight_seeds=tuple(range(args.gate_seeds)))
                del g
                torch.cuda.empty_cache()
                m = tab["modes"]
                ok_emb = [p for p in m if m[p]["gate_1e-4"]]
                ok_eer = [p for p in m if m[p]["eer_gate_every_draw"]]
                ok_both = [p for p in ok_emb if p in ok_eer]
                pick = lambda c: (lambda b: {"mode": b, "value": rate[model][b], "unit": "utterances/s"} if b else {"mode": None, "value": None})(max(c, key=lambda p: rate[model][p]) if c else None)
                grade[model] = {"config": {"xvector": "configs[1]", "ecapa": "configs[2] / [3]", "resnet": "configs[4]"}[model],
                                "fastest_mode_passing_1e-4": pick(ok_emb), "fastest_mode_passing_eer_gate_on_every_draw": pick(ok_eer),
                                "fastest_mode_passing_both": pick(ok_both), "rates": rate[model],
                                "draws": "%d weight seeds x %d trial lists of %d trials + one list of %d trials per seed; scoring: %s; reference-equivalent = the exact-f32 extraction" % (
                                    len(tab["weight_seeds"]), len(tab["trial_lists"]), tab["trials_per_list"], tab["big_list_trials"], tab["scoring"]),
                                "eer_f32_percent": tab["eer_f32_percent"], "planted_set": tab["planted_set"], "modes": m, "seconds": round(time.perf_counter() - t0, 1)}
            except Exception as e:                                        # a checker leg must never take the headline down
                grade[model] = {"error": "%s: %s" % (type(e).__name__, e)}
        res["parity_grade"] = grade
        xv = grade.get("xvector", {})
        if "fastest_mode_passing_both" in xv:
            res["value_parity_grade"] = dict(xv["fastest_mode_passing_both"], rule="the fastest precision mode of the headline workload that passes BOTH north-star gates - embeddings within "
                                             "1e-4 and EER delta < 0.01 % on every draw of parity_grade.xvector")
            res["value_eer_grade"] = dict(xv["fastest_mode_passing_eer_gate_on_every_draw"], rule="the fastest mode inside the EER gate on every draw, whatever its embedding error")

    if args.full and rank == 0 and world == 1 and args.cpu_seconds > 0 and not dry and not args.lengths:
        from oracle import torch_cpu_port as P                        # cpu_baseline leg only
        # torch's default (one thread per core) collapses on many-core hosts for these small
        # convolutions: probe a few thread counts briefly and time the sample with the best one
        if args.model != "xvector":
            raise SystemExit("cpu_baseline is implemented for the default workload only; pass --cpu-seconds 0 with --model %s" % args.model)
        ex = P.XvectorCpu(wl.sd, "far")
        host = os.cpu_count() or 1
        best, cores, one_thread = 0.0, 1, None
        for th in sorted({1, min(8, host), min(16, host), min(32, host)}):
            torch.set_num_threads(th)
            ups, _, _ = P.time_cpu_baseline(ex, wl.mats[:8], budget_s=min(1.5, args.cpu_seconds / 6.0), min_utts=2)
            if th == 1:
                one_thread = ups
            if ups > best:
                best, cores = ups, th
        torch.set_num_threads(cores)
        ups, n, secs = P.time_cpu_baseline(ex, wl.mats[:64], budget_s=args.cpu_seconds)
        res["cpu_baseline"] = {"value": round(ups, 2), "unit": "utterances/s", "cores": cores, "kind": "port",
                               "value_1_thread": round(one_thread, 2) if one_thread else None,      # the README's RTF protocol is single-threaded
                               "sample": "%d utterances of the same %dx%d workload, batch=1 loop as pipeline/onestep/extract_embeddings.py:73-83, "
                                         "torch %s CPU with the best of {1,8,16,32} threads on a %d-core host, %.1f s" % (n, wl.T, wl.D, torch.__version__, host, secs),
                               "why_port": "the reference tree cannot travel to the GPU box; oracle/torch_cpu_port.py issues the reference's exact torch "
                                           "calls (dense masked conv1d, in-place ReLU, eval batch_norm, two-pass pooling) and is pinned to the reference's outputs"}
    if rank == 0:
        emit(res)
    if dist_on:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
