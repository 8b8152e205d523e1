"""Shared by tests/test_de_silence_host.py and tests/test_gpu_desilence.py: the golden cases of tests/golden/de_silence.npz, the rule as
a plain block-by-block loop, the synthetic batches of the device tests, and the calls asv_desilence_pcm16 has to refuse."""

import collections
import ctypes as C
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "de_silence.npz")
Case = collections.namedtuple("Case", "name sample_rate min_eng x y")


@functools.lru_cache(maxsize=None)
def golden_cases():
    """(name, sample rate, min_eng, int16 input, the reference's int16 output) per case; read once, shared, never written."""
    with np.load(GOLDEN) as z:
        cases = tuple(Case(str(name), int(sr), float(eng), z["x_%d" % i], z["y_%d" % i])
                      for i, (name, sr, eng) in enumerate(zip(z["names"], z["sample_rate"], z["min_eng"])))
    for c in cases:
        c.x.setflags(write=False)
        c.y.setflags(write=False)
    return cases


def plain_rule(x, win, min_eng):
    """signal_processing.py:13-55 + processor.py:170-171 in integers, one block at a time."""
    kept = []
    for a in range(0, len(x), win):
        blk = x[a:a + win]
        if int(np.abs(blk.astype(np.int64)).sum()) > min_eng * len(blk):
            kept.append(blk)
    return np.concatenate(kept) if kept else np.asarray(x)


def utterance(rng, length, win, silent=False):
    """`length` int16 samples in blocks of `win`: loud, zero, +-2 counts, or a mean of exactly 50 / just above it, at random (silent: only
    the kinds a threshold of 50 drops)."""
    x = np.zeros(length, dtype=np.int16)
    for a in range(0, length, win):
        m = min(win, length - a)
        kind = rng.randint(5) if not silent else 1 + rng.randint(3)
        if kind == 0:
            x[a:a + m] = rng.randint(-3000, 3001, size=m)
            if np.abs(x[a:a + m].astype(np.int64)).sum() <= 50 * m:
                x[a] = 20000
        elif kind == 2:
            x[a:a + m] = rng.randint(-2, 3, size=m)
        elif kind == 3:
            x[a:a + m] = 50 * (1 - 2 * rng.randint(2, size=m))                 # S = 50 m: not above the threshold
        elif kind == 4:
            x[a:a + m] = 50 * (1 - 2 * rng.randint(2, size=m))
            x[a + rng.randint(m)] = 51                                         # S = 50 m + 1
    return x


def odd_batch(win, seed=5):
    """Odd lengths (so that later utterances start on odd samples), a zero-length utterance first, in the middle and last, one that falls back."""
    rng = np.random.RandomState(seed + win)
    lengths = [0, (3 * win + 1) | 1, 2 * win, (5 * win + win // 2) | 1, 0, win, (4 * win) | 1, (2 * win + 1) | 1, 3 * win, 0]
    return [utterance(rng, n, win, silent=(i == 6)) for i, n in enumerate(lengths)]


@functools.lru_cache(maxsize=None)
def long_utterance():
    """700 blocks of 7 samples: the scan over one utterance's blocks crosses a 256-thread workgroup twice."""
    x = utterance(np.random.RandomState(77), 699 * 7 + 3, 7)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def many_utterances():
    """600 utterances of 1 - 3 blocks of 64 samples (the last one partial for most), every seventh silent throughout: the scan over the
    utterances crosses a 256-thread workgroup twice, and fall-backs sit next to trimmed utterances.  Returns (utterances, silent flags)."""
    rng = np.random.RandomState(78)
    silent = [(i % 7 == 3) or i in (0, 599) for i in range(600)]
    utts = [utterance(rng, int(rng.randint(1, 193)), 64, silent=s) for s in silent]
    for u in utts:
        u.setflags(write=False)
    return tuple(utts), tuple(silent)


def offsets(utts):
    off = np.zeros(len(utts) + 1, dtype=np.int64)
    np.cumsum([len(u) for u in utts], out=off[1:])
    return off


def bad_calls(lib, wave, out, samples=64):
    """name -> call(out_offsets int64 [3]) for every argument set the entry point refuses; wave / out: addresses of `samples` int16 each."""
    p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_longlong))
    good = np.array([0, samples // 2, samples], dtype=np.int64)
    keep = []                                              # (the arrays outlive the lambdas)

    def call(wave=wave, off=good, n=2, win=8, eng=50.0, out=out, null_out_off=False):
        off = None if off is None else np.ascontiguousarray(off, dtype=np.int64)
        keep.append(off)
        return lambda out_off: lib.asv_desilence_pcm16(wave, None if off is None else p64(off), n, win, eng, out, None if null_out_off else p64(out_off), None)

    return {
        "wave is null": call(wave=None),
        "sample_offsets is null": call(off=None),
        "out is null": call(out=None),
        "out_offsets is null": call(null_out_off=True),
        "no utterance": call(n=0),
        "negative n_utts": call(n=-1),
        "win_samples 0": call(win=0),
        "win_samples negative": call(win=-3),
        "min_eng negative": call(eng=-1.0),
        "min_eng nan": call(eng=float("nan")),
        "min_eng inf": call(eng=float("inf")),
        "offsets decrease": call(off=[0, samples, samples // 2]),
        "offsets start behind 0": call(off=[1, samples // 2, samples]),
        "out is wave": call(out=wave),
        "out overlaps the end of wave": call(out=wave + 2 * (samples - 1)),
        "out overlaps the start of wave": call(out=wave - 2 * (samples - 1)),
    }
