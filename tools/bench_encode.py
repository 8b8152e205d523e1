#!/usr/bin/env python3
"""The device compressor of Kaldi feature matrices (asv_encode_compressed, csrc/kernels_encode.hip; profiles/encode_ab.txt):

    python tools/bench_encode.py [--reps 15] [--calls 4] [--wavs 2000] [--out profiles/encode_ab.txt]

(a) The kernel sequence alone, through the C ABI: 50 000 x 200 x 80 and a ragged table of 200 - 1000 frames x 80 ('CM '; fbank-like
    values - the select's work depends a little on how the keys spread).  Event-timed windows of --calls back-to-back calls, median /
    min / max over --reps windows after 3 warm-up windows, same offsets in every call (the staged upload is reused).  Bytes are counted
    from the shapes: the algorithmic 4 B in + 1 B out per value, and what the sequence really reads - the input SIX times (1 min / max
    pass, 4 radix-select passes, 1 quantising pass; the later passes of a short utterance hit the L2) - so GB/s is given both ways.  A
    few utterances are compared byte for byte with the NumPy restatement (tests/compress_cases.py) before anything is timed.
(b) wav -> ark through makeFeatures.py's make_features on files in a tmpfs (/dev/shm when there, else the temp dir; page cache either
    way), --wavs files of 2 - 6 s, 80-bin fbank + energy, three ways in the same process, in both orders:
        compress      --compress true (the device compressor)
        float         --compress false ('FM ' matrices, 4 B per value)
        float+numpy   --compress false, then the NumPy restatement on the host over that archive into a compressed one - what a user
                      without the kernel would do
    Wall-clock seconds of each whole call, and the archive sizes.
One MI355X, one process; numbers from different boxes or sessions are not comparable to a few per cent.
"""
import argparse
import ctypes as C
import os
import shutil
import statistics
import sys
import tempfile
import time
import wave

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "asv-subtools_amd", "pytorch"))
sys.path.insert(0, os.path.join(REPO, "tests"))

HBM_PEAK_TBS = 8.0


def fbank_like(rng, rows, dim):
    import numpy as np
    t = np.arange(rows, dtype=np.float32)[:, None]
    return (8.0 + 4.0 * np.sin(t / 17.0 + np.arange(dim, dtype=np.float32)[None] / 5.0) + rng.standard_normal((rows, dim), dtype=np.float32)).astype(np.float32)


def kernel_sequence(lines, reps, calls):
    import numpy as np
    import torch
    import compress_cases as cc
    from libs.amd import capi, frontend
    lib = capi.lib()
    dev = torch.device("cuda", 0)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p64 = lambda x: x.ctypes.data_as(C.POINTER(C.c_longlong))
    rng = np.random.default_rng(0)
    tables = (("50000 x 200 x 80", np.full(50000, 200, dtype=np.int64)), ("16384 x (200 - 1000) x 80", rng.integers(200, 1001, size=16384).astype(np.int64)))
    for name, rows in tables:
        dim = 80
        frame_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
        total = int(frame_off[-1])
        # one block of fbank-like rows, tiled: the values of an utterance are what matters to the select, not their uniqueness across the table
        block = torch.from_numpy(fbank_like(rng, 1 << 16, dim)).to(dev)
        feats = block.repeat((total + block.shape[0] - 1) // block.shape[0], 1)[:total].contiguous()
        formats = np.ones(len(rows), dtype=np.uint8)
        sizes = (frontend.compressed_body_bytes(formats, rows, dim) + 15) // 16 * 16
        byte_off = np.concatenate([[0], np.cumsum(sizes[:-1])]).astype(np.int64)
        out = torch.empty(int(byte_off[-1] + sizes[-1]), dtype=torch.uint8, device=dev)
        status = torch.empty(len(rows), dtype=torch.int32, device=dev)

        def call():
            capi.check(lib.asv_encode_compressed(feats.data_ptr(), p64(frame_off), p64(byte_off), formats.ctypes.data_as(C.POINTER(C.c_ubyte)), len(rows), dim,
                                                 out.data_ptr(), status.data_ptr(), stream), "asv_encode_compressed")

        call()
        torch.cuda.synchronize(dev)
        same = int(status.sum().item()) == 0
        for u in (0, 1, len(rows) // 2, len(rows) - 1):
            a, b = int(frame_off[u]), int(frame_off[u + 1])
            fmt, body = cc.kaldi_compress(feats[a:b].cpu().numpy())
            same = same and fmt == 1 and out[int(byte_off[u]):int(byte_off[u]) + len(body)].cpu().numpy().tobytes() == body
        times = []
        for rep in range(reps + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            e0.record()
            for _ in range(calls):
                call()
            e1.record()
            e1.synchronize()
            if rep >= 3:
                times.append(e0.elapsed_time(e1) * 1e3 / calls)
        times.sort()
        med = statistics.median(times)
        values = total * dim
        algorithmic, read6 = values * 5, values * (6 * 4 + 1)
        lines.append("%-28s %10.0f us/call (min %.0f, max %.0f; %d windows of %d calls)  %6.2f G values/s   algorithmic 5 B/value: %6.0f GB/s (%4.1f %% of %g TB/s)   "
                     "6 reads + 1 B out = 25 B/value: %6.0f GB/s   bytes = NumPy restatement: %s" %
                     (name, med, times[0], times[-1], reps, calls, values / med / 1e3, algorithmic / med / 1e3, algorithmic / med / 1e6 / HBM_PEAK_TBS * 100, HBM_PEAK_TBS,
                      read6 / med / 1e3, same))
        assert same
        del feats, out, block
        torch.cuda.empty_cache()


def write_wavs(root, n):
    import numpy as np
    rng = np.random.default_rng(1)
    d = os.path.join(root, "data", "bench")
    os.makedirs(d)
    seconds = 0.0
    with open(os.path.join(d, "wav.scp"), "w") as scp:
        for i in range(n):
            s = int(rng.integers(2 * 16000, 6 * 16000))
            x = (2000.0 * rng.standard_normal(s, dtype=np.float32)).astype("<i2")
            path = os.path.join(root, "w%05d.wav" % i)
            with wave.open(path, "wb") as f:
                f.setnchannels(1)
                f.setsampwidth(2)
                f.setframerate(16000)
                f.writeframes(x.tobytes())
            scp.write("utt%05d %s\n" % (i, path))
            seconds += s / 16000.0
    return d, seconds


def script_paths(lines, n_wavs):
    import numpy as np
    import torch
    import compress_cases as cc
    from libs.amd import featprep
    from libs.support import kaldi_io
    root = tempfile.mkdtemp(prefix="asv_bench_encode_", dir="/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None)
    try:
        d, audio_s = write_wavs(root, n_wavs)
        conf = os.path.join(root, "fbank.conf")
        with open(conf, "w") as f:
            f.write("--num-mel-bins=80\n--use-energy=true\n--dither=0\n")
        exp = os.path.join(root, "exp")
        name = featprep.data_name(d)
        ark = os.path.join(exp, "fbank", name, "raw_fbank_%s.1.ark" % name)

        def run(way):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            featprep.make_features(d, "fbank", conf, exp=exp, compress=(way == "compress"))
            if way == "float+numpy":
                items = ((k,) + cc.kaldi_compress(np.ascontiguousarray(m, dtype=np.float32)) for k, m in kaldi_io.read_mat_scp(os.path.join(d, "feats.scp")))
                kaldi_io.write_compressed_ark_scp(os.path.join(root, "host.ark"), os.path.join(root, "host.scp"), items)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            size = os.path.getsize(os.path.join(root, "host.ark") if way == "float+numpy" else ark)
            return dt, size

        run("compress")                                                         # warm-up: library load, tables, page cache
        ways = ("compress", "float", "float+numpy")
        got = {w: [] for w in ways}
        sizes = {}
        for order in (ways, ways[::-1], ways, ways[::-1]):
            for w in order:
                dt, sizes[w] = run(w)
                got[w].append(dt)
        lines.append("%d wavs, %.0f s of audio, 81 columns; wall seconds of the whole call, 4 runs each (orders: forward, backward, forward, backward)" % (n_wavs, audio_s))
        for w in ways:
            t = got[w]
            lines.append("  %-12s median %7.3f s  (%s)   archive %8.1f MB   %7.0f x real time" %
                         (w, statistics.median(t), " ".join("%.3f" % v for v in t), sizes[w] / 1e6, audio_s / statistics.median(t)))
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--wavs", type=int, default=2000)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    lines = ["Device compressor of Kaldi feature matrices (asv_encode_compressed, kernels_encode.hip; DESIGN 4.3.5) - one MI355X, one session", "",
             "(a) the kernel sequence alone (memset + min/max + select + encode), through the C ABI"]
    kernel_sequence(lines, a.reps, a.calls)
    if a.wavs > 0:                                                            # (--wavs 0: part (a) alone, e.g. under a kernel trace)
        lines += ["", "(b) wav -> ark through makeFeatures.py (make_features), files in a tmpfs"]
        script_paths(lines, a.wavs)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
