"""Writes tests/golden/de_silence.npz: what the reference's own de_silence (pytorch/libs/egs/signal_processing.py:13-55) returns for
constructed 16-bit utterances, with the keep-whole fallback of its caller (pytorch/libs/egs/processor.py:170-171: `if force_output and
cache_len==0: cache_wave=waveform`; the retry of lines 166-169 drops its length in line 168, so it never changes what an utterance
yields) applied here.  tests/test_de_silence_host.py checks libs.amd.frontend.de_silence_host against it, tests/test_gpu_desilence.py the
device entry.

Needs the reference tree (build container only).  signal_processing.py is loaded on its own by file path: processor.py pulls in
torchaudio, which this check does not need.  The waveform handed over is what torchaudio.load(normalize=True) gives for 16-bit PCM:
float32 int16 / 32768, shape [1, L].  The fixture holds data only: the int16 inputs, (sample rate, min_eng) per case, and the reference's
output converted back to int16.

The cases are constructed, not drawn.  A block of m samples with a chosen S = sum |s_i| sits at floor(min_eng * m) - 1 / + 0 / + 1
around the threshold S > min_eng * m; every case has at least one kept and one dropped block, except the ones named for it: a single
block can only be one or the other (b), wholly silent (e: kept whole), wholly loud (f: nothing dropped)."""

import importlib.util
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
SOURCE = os.path.join(REF, "pytorch", "libs", "egs", "signal_processing.py")


def block(m, total, seed):
    """m int16 samples with sum |s| == total exactly: magnitudes total // m and one more for the first total % m, moved between
    neighbours by a fixed pattern, signs from the same pattern."""
    base, rem = divmod(int(total), m)
    assert base < 32767
    mag = np.full(m, base, dtype=np.int64)
    mag[:rem] += 1
    k = np.arange(m)
    pat = (k * 2654435761 + seed * 40503) >> 7
    shift = np.minimum(mag[0::2][:m // 2], mag[1::2][:m // 2])
    shift = np.minimum(shift, 32767 - np.maximum(mag[0::2][:m // 2], mag[1::2][:m // 2])) * (pat[:m // 2] % 3) // 3      # pairs: +d / -d keeps the sum
    mag[0:2 * (m // 2):2] += shift
    mag[1:2 * (m // 2):2] -= shift
    assert mag.min() >= 0 and mag.max() <= 32767 and int(mag.sum()) == int(total)
    mag = np.roll(mag, seed % m)
    return np.where(pat % 2 == 0, mag, -mag).astype(np.int16)


def around(min_eng, m, delta, seed):
    return block(m, int(np.floor(min_eng * m)) + delta, seed)


def cases():
    out = []

    def add(name, sr, min_eng, parts):
        out.append((name, sr, float(min_eng), np.concatenate(parts).astype(np.int16)))

    n = 1600
    loud, quiet, zero = (lambda m, s: block(m, 3000 * m, s)), (lambda m, s: block(m, 2 * m, s)), (lambda m: np.zeros(m, dtype=np.int16))
    # (a) blocks one count below, at and above the threshold, full blocks and a 777-sample tail, at three thresholds
    for eng in (12.5, 50, 100):
        for tail_delta in (-1, 0, 1):
            add("a_eng%g_tail%+d" % (eng, tail_delta), 16000, eng,
                [around(eng, n, -1, 1), around(eng, n, 1, 2), around(eng, n, 0, 3), loud(n, 4), zero(n), around(eng, n, 1, 5), around(eng, 777, tail_delta, 6)])
    # (b) shorter than one block: the tail block alone
    add("b_short_loud", 16000, 50, [loud(500, 7)])
    add("b_short_quiet_kept_whole", 16000, 50, [quiet(500, 8)])
    add("b_short_at_threshold_kept_whole", 16000, 50, [around(50, 999, 0, 9)])
    # (c) a whole number of blocks: no tail
    add("c_exact_blocks", 16000, 50, [loud(n, 10), zero(n), quiet(n, 11), loud(n, 12)])
    # (d) a tail of one sample: 51 > 50 is kept, 50 > 50 is not
    add("d_tail_one_kept", 16000, 50, [quiet(n, 13), loud(n, 14), zero(n), np.array([-51])])
    add("d_tail_one_dropped", 16000, 50, [loud(n, 15), quiet(n, 16), loud(n, 17), np.array([50])])
    # (e) wholly silent: kept whole; (f) wholly loud: nothing dropped
    add("e_silent_zeros_kept_whole", 16000, 50, [zero(2 * n + 300)])
    add("e_silent_two_counts_kept_whole", 16000, 50, [quiet(n, 18), quiet(n, 19), quiet(41, 20)])
    add("f_loud", 16000, 50, [loud(n, 21), loud(n, 22), loud(123, 23)])
    # (g) a block of -32768 throughout: |s| does not fit 16 bits
    add("g_min_int16", 16000, 100, [zero(n), np.full(n, -32768), quiet(n, 24), np.full(37, -32768)])
    # (h) other sample rates: n = 4410 is no multiple of 8, n = 800
    add("h_44100", 44100, 50, [around(50, 4410, 1, 25), around(50, 4410, 0, 26), loud(4410, 27), zero(4410), around(50, 1001, -1, 28)])
    add("h_44100_eng12.5", 44100, 12.5, [around(12.5, 4410, -1, 29), around(12.5, 4410, 1, 30), around(12.5, 3, 1, 31)])
    add("h_8000", 8000, 100, [around(100, 800, 0, 32), around(100, 800, 1, 33), zero(800), loud(800, 34), around(100, 800, -1, 35), around(100, 799, 1, 36)])
    return out


def main():
    if not os.path.isfile(SOURCE):
        sys.exit("gen_de_silence_golden.py needs the reference tree at %s (build container only)" % REF)
    import torch
    spec = importlib.util.spec_from_file_location("ref_signal_processing", SOURCE)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {"names": [], "sample_rate": [], "min_eng": []}
    for i, (name, sr, eng, x) in enumerate(cases()):
        sig = torch.from_numpy(x.astype(np.float32) / np.float32(32768.0))[None, :]
        kept, lens = ref.de_silence(sig, sr=sr, win_len=0.1, min_eng=eng)
        if lens == 0:                                     # processor.py:170-171
            kept = sig
        y = np.round(kept[0].numpy().astype(np.float64) * 32768.0).astype(np.int16)
        n = int(0.1 * sr)
        blocks = -(-len(x) // n)
        print("%-36s sr %5d min_eng %5g: %6d samples, %d blocks -> %6d samples%s" % (name, sr, eng, len(x), blocks, len(y), "  (kept whole)" if lens == 0 else ""))
        out["names"].append(name)
        out["sample_rate"].append(sr)
        out["min_eng"].append(eng)
        out["x_%d" % i], out["y_%d" % i] = x, y
    out["names"] = np.array(out["names"])
    out["sample_rate"] = np.array(out["sample_rate"], dtype=np.int64)
    out["min_eng"] = np.array(out["min_eng"], dtype=np.float64)
    dst = os.path.join(REPO, "tests", "golden", "de_silence.npz")
    np.savez_compressed(dst, **out)
    print("wrote %s (%d bytes)" % (dst, os.path.getsize(dst)))


if __name__ == "__main__":
    main()
