"""asv_ingest_windows (csrc/kernels_ingest.hip) through the C ABI: a batch of windows of rows that lie on the device, each normalised as
an utterance of its own - overlapping, repeated, in any order, from two parents.  The yardstick is asv_ingest_frames(voiced = NULL) on a
host-packed copy of the same windows, bit for bit (that kernel is pinned to the float64 restatement of Kaldi's rule by
tests/test_gpu_ingest.py, and to asv_cmvn_sliding bit for bit)."""

import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PARENTS = [700, 40]                                      # packed one behind the other: rows 0..699 and 700..739
ROWS = sum(PARENTS)
DIMS = [1, 30, 64, 65]                                   # one column, a partial block, exactly one block of 64 columns, one column more
LENGTHS = [1, 31, 32, 33, 64, 100, 299, 300, 301, 333]   # around the 32-frame segment and around cmn_window = 300
ZERO = 22                                                # index of the zero-length window below
WINDOWS = (
    [(0, n) for n in LENGTHS]                            # from row 0
    + [(700 - n, n) for n in (1, 33, 300, 333)]          # to the first parent's last row
    + [(100 + 50 * i, 100) for i in range(6)]            # a half-overlapping run
    + [(200, 150), (200, 150)]                           # one window twice
    + [(350, 0)]                                         # an empty one between its neighbours
    + [(600, 64), (700, 40), (10, 31), (705, 32), (400, 299), (739, 1), (700, 1), (367, 333)]      # any order, alternating between the parents
    + [(708, 32), (700, 33), (1, 300), (2, 301), (399, 301), (50, 64), (333, 333), (699, 1), (668, 32)]
)
START = np.array([w[0] for w in WINDOWS], dtype=np.int64)
LEN = np.array([w[1] for w in WINDOWS], dtype=np.int64)
OFF = np.concatenate([[0], np.cumsum(LEN)]).astype(np.int64)
TOTAL = int(OFF[-1])
OPTS = [(300, 100, 1, 0), (300, 100, 0, 0), (300, 100, 1, 1), (300, 100, 0, 1), (0, 100, 1, 0)]      # (cmn_window, min_window, center, norm_vars)
CANARY = 3                                               # rows behind the last one written
MARK = np.float32(-12345.678)


def test_the_window_list_covers_what_it_should():
    assert len(WINDOWS) == 40 and WINDOWS[ZERO] == (350, 0) and (LEN[np.arange(len(LEN)) != ZERO] > 0).all()
    assert (START + LEN <= ROWS).all() and set(LENGTHS) <= set(LEN.tolist())
    assert (np.diff(START) < 0).any() and WINDOWS.count((200, 150)) == 2
    # no window crosses from one parent into the other
    assert all(a + n <= 700 or a >= 700 for a, n in WINDOWS)


@functools.lru_cache(maxsize=None)
def host(dim):
    from libs.amd import synth
    return np.concatenate([synth.synth_feats(T, dim, 70 + i) * 3.0 + 1.5 for i, T in enumerate(PARENTS)], axis=0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def packed_copy(dim):
    return np.concatenate([host(dim)[a:a + n] for a, n in WINDOWS], axis=0)


def p64(a):
    return a.ctypes.data_as(C.POINTER(C.c_longlong))


def call(x, start, length, dim, opts, out, n_rows=None):
    from libs.amd import capi
    start, length = np.ascontiguousarray(start, dtype=np.int64), np.ascontiguousarray(length, dtype=np.int64)
    return capi.lib().asv_ingest_windows(x.data_ptr() if x is not None else None, x.shape[0] if n_rows is None else n_rows,
                                         p64(start) if start is not None else None, p64(length), len(start), dim, opts[0], opts[1], opts[2], opts[3],
                                         out.data_ptr() if out is not None else None, None)


@functools.lru_cache(maxsize=None)
def reference(dim, k):
    """asv_ingest_frames without flags on the host-packed copy of the windows: computed once per (dim, option set), kept on the host."""
    import torch
    from libs.amd import capi
    x = torch.from_numpy(packed_copy(dim)).cuda()
    out = torch.empty_like(x)
    o = OPTS[k]
    capi.check(capi.lib().asv_ingest_frames(x.data_ptr(), None, p64(OFF), p64(OFF), len(WINDOWS), dim, o[0], o[1], o[2], o[3], out.data_ptr(), None), "asv_ingest_frames")
    return out.cpu().numpy()


def marked(rows, dim):
    import torch
    return torch.full((rows, dim), float(MARK), dtype=torch.float32, device="cuda")


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("k", range(len(OPTS)))
def test_equals_ingest_frames_on_the_packed_copy_bit_for_bit(dim, k):
    import torch
    from libs.amd import capi
    x = torch.from_numpy(host(dim)).cuda()
    before = x.clone()
    out = marked(TOTAL + CANARY, dim)
    capi.check(call(x, START, LEN, dim, OPTS[k], out), "asv_ingest_windows")
    got = out.cpu().numpy()
    assert torch.equal(x, before)                                              # the input is read only
    want = reference(dim, k)
    assert np.array_equal(got[:TOTAL].view(np.uint32), want.view(np.uint32)), (dim, OPTS[k])
    if OPTS[k][0] == 0:                                                         # a pure gather: the rows as they are
        assert np.array_equal(got[:TOTAL].view(np.uint32), packed_copy(dim).view(np.uint32))
    assert (got[TOTAL:] == MARK).all()                                          # nothing behind the last row


@pytest.mark.parametrize("dim", [30, 65])
@pytest.mark.parametrize("k", [0, 3])
def test_a_window_does_not_depend_on_the_other_windows(dim, k):
    import torch
    from libs.amd import capi
    x = torch.from_numpy(host(dim)).cuda()
    want = reference(dim, k)
    out = marked(int(LEN.max()) + CANARY, dim)
    for w, (a, n) in enumerate(WINDOWS):
        if n == 0:
            continue
        out.fill_(float(MARK))
        capi.check(call(x, [a], [n], dim, OPTS[k], out), "asv_ingest_windows")
        got = out.cpu().numpy()
        assert np.array_equal(got[:n].view(np.uint32), want[OFF[w]:OFF[w + 1]].view(np.uint32)), (dim, w, a, n)
        assert (got[n:] == MARK).all(), (dim, w)


def test_an_empty_window_writes_nothing():
    """Alone: no launch, `out` untouched.  Between two neighbours: they lie one behind the other, and nothing behind them is written."""
    import torch
    from libs.amd import capi, frontend
    dim = 30
    x = torch.from_numpy(host(dim)).cuda()
    out = marked(16, dim)
    capi.check(call(x, [350], [0], dim, OPTS[0], out), "asv_ingest_windows")
    assert bool((out == float(MARK)).all())
    capi.check(call(x, [10, 350, 20], [5, 0, 5], dim, OPTS[4], out), "asv_ingest_windows")
    got = out.cpu().numpy()
    assert np.array_equal(got[:5], host(dim)[10:15]) and np.array_equal(got[5:10], host(dim)[20:25]) and (got[10:] == MARK).all()
    # the Python front end: the offsets of the windows in the result, `out=` taken as it is
    rows, off = frontend.ingest_windows(x, START, LEN, cmn_window=300, out=marked(TOTAL + CANARY, dim))
    assert np.array_equal(off, OFF) and rows.shape == (TOTAL, dim)
    assert np.array_equal(rows.cpu().numpy().view(np.uint32), reference(dim, 0).view(np.uint32))
    none, off0 = frontend.ingest_windows(x, [350], [0], cmn_window=300)
    assert none.shape == (0, dim) and not off0.any()


def test_bad_arguments_return_negative_with_a_text_and_write_nothing():
    import torch
    from libs.amd import capi
    lib = capi.lib()
    dim = 30
    x = torch.from_numpy(host(dim)).cuda()
    out = marked(TOTAL + CANARY, dim)
    good = OPTS[0]
    neg_start, neg_len, beyond = START.copy(), LEN.copy(), START.copy()
    neg_start[5], neg_len[7], beyond[13] = -1, -1, ROWS - LEN[13] + 1
    inside = x[100:]                                                            # `out` inside `feats`: rows other windows still read
    cases = {
        "feats is null": lambda: lib.asv_ingest_windows(None, ROWS, p64(START), p64(LEN), len(WINDOWS), dim, 300, 100, 1, 0, out.data_ptr(), None),
        "win_start is null": lambda: lib.asv_ingest_windows(x.data_ptr(), ROWS, None, p64(LEN), len(WINDOWS), dim, 300, 100, 1, 0, out.data_ptr(), None),
        "win_len is null": lambda: lib.asv_ingest_windows(x.data_ptr(), ROWS, p64(START), None, len(WINDOWS), dim, 300, 100, 1, 0, out.data_ptr(), None),
        "out is null": lambda: lib.asv_ingest_windows(x.data_ptr(), ROWS, p64(START), p64(LEN), len(WINDOWS), dim, 300, 100, 1, 0, None, None),
        "no window": lambda: lib.asv_ingest_windows(x.data_ptr(), ROWS, p64(START), p64(LEN), 0, dim, 300, 100, 1, 0, out.data_ptr(), None),
        "dim 0": lambda: lib.asv_ingest_windows(x.data_ptr(), ROWS, p64(START), p64(LEN), len(WINDOWS), 0, 300, 100, 1, 0, out.data_ptr(), None),
        "negative start": lambda: call(x, neg_start, LEN, dim, good, out),
        "negative length": lambda: call(x, START, neg_len, dim, good, out),
        "beyond n_rows": lambda: call(x, beyond, LEN, dim, good, out),
        "beyond a smaller n_rows": lambda: call(x, START, LEN, dim, good, out, n_rows=ROWS - 1),
        "out is feats": lambda: call(x, START, LEN, dim, good, x),
        "out inside feats": lambda: call(x, START[:3], LEN[:3], dim, good, inside),
        "causal, min_window 0": lambda: call(x, START, LEN, dim, (300, 0, 0, 0), out),
        "causal, min_window > cmn_window": lambda: call(x, START, LEN, dim, (300, 301, 0, 0), out),
    }
    before = x.clone()
    for name, bad in cases.items():
        rc = bad()
        assert rc < 0, name
        text = lib.asv_last_error()
        assert text and b"asv_ingest_windows" in text, name
    torch.cuda.synchronize()
    assert bool((out == float(MARK)).all()) and torch.equal(x, before)          # no launch: nothing was written anywhere
    # the library still works after the refusals
    capi.check(call(x, START, LEN, dim, good, out), "asv_ingest_windows")
    assert np.array_equal(out.cpu().numpy()[:TOTAL].view(np.uint32), reference(dim, 0).view(np.uint32))
