#!/usr/bin/env python3
"""The device decode of Kaldi compressed matrices alone (asv_decode_compressed, csrc/kernels_decode.hip; profiles/decode_ab.txt):

    python tools/bench_decode.py [--reps 25] [--calls 200]

One batch of 256 x 200 x 80 and one of 321 x 200 x 80 'CM ' matrices (random percentiles and bytes: the kernel's work does not depend on
the values), decoded through the C ABI.  Event-timed: a window of --calls back-to-back calls between two events (one call is a few
microseconds - a window of one would measure the event pair), per-call time = window / calls, median / min / max over --reps windows
after 5 warm-up windows.  The offsets are the same in every call (the staged upload is reused: no copy) and, in a second series,
alternate between two batches (one asynchronous 5 KB upload per call, as in the extraction loop).  Bytes are counted from the shapes:
1 B read and 4 B written per value, plus the column headers; GB/s next to the HBM figures DESIGN normalises by (8 TB/s peak, ~6.3
achievable).  The first batch is compared bit for bit with the host reader before anything is timed.  Kernel time alone: run this
under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import struct
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "asv-subtools_amd", "pytorch"))

HBM_PEAK_TBS, HBM_ACHIEVABLE_TBS = 8.0, 6.3


def cm_batch(rng, utts, frames, dim):
    """(uint8 array of the bodies, each at a 16-byte boundary; byte offsets; frame offsets; formats)"""
    import numpy as np
    size = 16 + 8 * dim + frames * dim
    step = (size + 15) // 16 * 16
    buf = np.zeros(utts * step, dtype=np.uint8)
    for u in range(utts):
        pct = np.sort(rng.randint(0, 65536, size=(dim, 4)), axis=1).astype("<u2")
        body = struct.pack("<ffii", -12.5, 31.0, frames, dim) + pct.tobytes() + rng.randint(0, 256, size=dim * frames).astype(np.uint8).tobytes()
        buf[u * step:u * step + size] = np.frombuffer(body, dtype=np.uint8)
    return buf, np.arange(utts, dtype=np.int64) * step, np.arange(utts + 1, dtype=np.int64) * frames, np.ones(utts, dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    import numpy as np
    import torch
    from libs.amd import capi
    from libs.support import kaldi_io
    lib = capi.lib()
    dev = torch.device("cuda", 0)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p64 = lambda x: x.ctypes.data_as(C.POINTER(C.c_longlong))
    pu8 = lambda x: x.ctypes.data_as(C.POINTER(C.c_ubyte))
    for utts, frames, dim in ((256, 200, 80), (321, 200, 80)):
        rng = np.random.RandomState(utts)
        batches = []
        for _ in range(2):
            host, byte_off, frame_off, formats = cm_batch(rng, utts, frames, dim)
            batches.append((host, torch.from_numpy(host).to(dev), byte_off, frame_off, formats))
        out = torch.empty((utts * frames, dim), dtype=torch.float32, device=dev)

        def call(k):
            _, d, byte_off, frame_off, formats = batches[k]
            capi.check(lib.asv_decode_compressed(d.data_ptr(), p64(byte_off), p64(frame_off), pu8(formats), utts, dim, out.data_ptr(), stream), "asv_decode_compressed")

        call(0)
        torch.cuda.synchronize(dev)
        got = out.cpu().numpy()
        host, _, byte_off, _, _ = batches[0]
        size = 16 + 8 * dim + frames * dim
        same = True
        for u in range(0, utts, 17):
            want = kaldi_io.read_mat(io.BytesIO(b"\0BCM " + host[int(byte_off[u]):int(byte_off[u]) + size].tobytes()))
            same = same and bool(np.array_equal(np.ascontiguousarray(want, dtype=np.float32).view(np.uint32), got[u * frames:(u + 1) * frames].view(np.uint32)))
        times = {"same offsets": [], "offsets changed": []}
        for rep in range(a.reps + 5):
            for name in times:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                e0.record()
                for i in range(a.calls):
                    call(i & 1 if name == "offsets changed" else 0)
                e1.record()
                e1.synchronize()
                if rep >= 5:
                    times[name].append(e0.elapsed_time(e1) * 1e3 / a.calls)
        values = utts * frames * dim
        moved = values * 5 + utts * (16 + 8 * dim)
        rec = {"batch": [utts, frames, dim], "format": "CM ", "bit_equal_to_host_reader": same, "reps": a.reps, "calls_per_window": a.calls,
               "bytes_by_shape": moved, "hbm_peak_tb_s": HBM_PEAK_TBS, "hbm_achievable_tb_s": HBM_ACHIEVABLE_TBS}
        for name, t in times.items():
            t = sorted(t)
            med = statistics.median(t)
            rec[name] = {"median_us_per_call": round(med, 2), "min_us": round(t[0], 2), "max_us": round(t[-1], 2), "gb_s": round(moved / med / 1e3, 1),
                         "share_of_hbm_peak": round(moved / med / 1e6 / HBM_PEAK_TBS, 3)}
        print(json.dumps(rec))
        assert same


if __name__ == "__main__":
    main()
