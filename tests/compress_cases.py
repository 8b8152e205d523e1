"""The quantiser of Kaldi's compressed matrices (compressed-matrix.cc, the automatic method of copy-feats --compress=true) restated in
NumPy float32, written independently of csrc/kernels_encode.hip, and the matrices both test files of the device encode use -
tests/test_make_features_host.py, tests/test_gpu_encode_compressed.py, tests/gen_compress_golden.py.  Not collected by pytest.

The rule: sequential float32, each operation rounded on its own; float -> int conversions truncate.
    min, max over the matrix; max == min -> max = min + (1 + |min|); range = max - min
    u16(v) = (int)(clamp((v - min) / range, 0, 1) * 65535 + 0.499f)
    f(q)   = ((float)q * range) * 1.52590218966964e-05f + min                      (what every reader computes)
    'CM ' column, s = the column sorted, n rows: order statistics s[0], s[n/4], s[3 (n/4)], s[n-1] (n < 5: s[0..3], missing ones "+ 1")
        p0 = min(u16(.), 65532), p25 = min(max(u16(.), p0 + 1), 65533), p75 = min(max(u16(.), p25 + 1), 65534), p100 = max(u16(.), p75 + 1)
        value v: v < f(p25): clamp((int)((v - P0) / (P25 - P0) * 64 + 0.5f), 0, 64); v < f(p75): 64 + clamp(... * 128 ..., 0, 128);
                 else 192 + clamp(... * 63 ..., 0, 63)
    'CM2': u16(v), row-major.          more than 8 rows -> 'CM ', otherwise 'CM2'
"""

import struct

import numpy as np

F = np.float32
INT_MIN = -2147483648


def _to_int(x):
    """(int)x of C on x86 (cvttss2si): truncates; INT_MIN for a NaN and for anything outside int32."""
    x = np.asarray(x, dtype=F)
    ok = np.isfinite(x) & (x >= F(-2147483648.0)) & (x < F(2147483648.0))
    return np.where(ok, np.trunc(np.where(ok, x, F(0))).astype(np.int64), INT_MIN)


def _min_max(mat):
    """Min and max with -0.0 in front of +0.0 (np.min / np.max leave the sign of a zero extreme open)."""
    mn, mx = F(mat.min()), F(mat.max())
    if mn == 0:
        mn = F(-0.0) if np.signbit(mat[mat == 0]).any() else F(0.0)
    if mx == 0:
        mx = F(0.0) if (~np.signbit(mat[mat == 0])).any() else F(-0.0)
    return mn, mx


def global_header(mat):
    mn, mx = _min_max(mat)
    if mx == mn:
        mx = F(mn + F(F(1.0) + abs(mn)))
    return mn, F(mx - mn)


def _u16(v, mn, rng):
    f = (np.asarray(v, dtype=F) - mn) / rng
    f = np.where(f > F(1.0), F(1.0), f)
    f = np.where(f < F(0.0), F(0.0), f).astype(F)
    return _to_int(f * F(65535.0) + F(0.499))


def percentile_value(q, mn, rng):
    return (np.asarray(q).astype(F) * rng) * F(1.52590218966964e-05) + mn


def column_percentiles(mat, mn, rng):
    """uint16 [cols, 4]"""
    n = mat.shape[0]
    s = np.sort(mat, axis=0)
    idx = [0, n // 4, 3 * (n // 4), n - 1] if n >= 5 else [0, 1, 2, 3]
    p0 = np.minimum(_u16(s[idx[0]], mn, rng), 65532)
    p25 = np.minimum(np.maximum(_u16(s[idx[1]], mn, rng), p0 + 1), 65533) if idx[1] < n else p0 + 1
    p75 = np.minimum(np.maximum(_u16(s[idx[2]], mn, rng), p25 + 1), 65534) if idx[2] < n else p25 + 1
    p100 = np.maximum(_u16(s[idx[3]], mn, rng), p75 + 1) if idx[3] < n else p75 + 1
    return np.clip(np.stack([p0, p25, p75, p100], axis=1), 0, 65535).astype("<u2")


def auto_format(rows):
    return 1 if rows > 8 else 2


def kaldi_compress(mat, fmt=None):
    """(format 1 = 'CM ' / 2 = 'CM2', the body: what lies behind the token on disk).  fmt=None: Kaldi's automatic choice."""
    mat = np.ascontiguousarray(mat, dtype=F)
    rows, cols = mat.shape
    assert rows >= 1 and cols >= 1
    fmt = auto_format(rows) if fmt is None else fmt
    with np.errstate(all="ignore"):
        mn, rng = global_header(mat)
        head = struct.pack("<ffii", mn, rng, rows, cols)
        if fmt == 2:
            return 2, head + np.clip(_u16(mat, mn, rng), 0, 65535).astype("<u2").tobytes()
        assert fmt == 1
        pct = column_percentiles(mat, mn, rng)
        P = percentile_value(pct, mn, rng)                                     # [cols, 4] float32
        P0, P25, P75, P100 = (P[:, i:i + 1] for i in range(4))
        v = mat.T
        lo = np.clip(_to_int((v - P0) / (P25 - P0) * F(64.0) + F(0.5)), 0, 64)
        mid = 64 + np.clip(_to_int((v - P25) / (P75 - P25) * F(128.0) + F(0.5)), 0, 128)
        hi = 192 + np.clip(_to_int((v - P75) / (P100 - P75) * F(63.0) + F(0.5)), 0, 63)
        data = np.where(v < P25, lo, np.where(v < P75, mid, hi)).astype(np.uint8)
    return 1, head + pct.tobytes() + np.ascontiguousarray(data).tobytes()


def error_bound(mat, fmt, body):
    """Per value: step / 2 + range / 65535, step = the width of the value's segment / its 64, 128 or 63 codes ('CM2': step 0) - nearest-code
    rounding plus at most 0.501 of a uint16 quantum from the header rounding and the end clamps.  float64 [rows, cols]."""
    mat = np.ascontiguousarray(mat, dtype=F)
    rows, cols = mat.shape
    mn, rng = struct.unpack("<ff", body[:8])
    quantum = float(rng) / 65535.0
    if fmt == 2:
        return np.full(mat.shape, quantum)
    pct = np.frombuffer(body[16:16 + 8 * cols], dtype="<u2").reshape(cols, 4)
    P = percentile_value(pct, F(mn), F(rng)).astype(np.float64)
    v = mat.T
    step = np.where(v < P[:, 1:2].astype(F), (P[:, 1:2] - P[:, 0:1]) / 64.0, np.where(v < P[:, 2:3].astype(F), (P[:, 2:3] - P[:, 1:2]) / 128.0, (P[:, 3:4] - P[:, 2:3]) / 63.0))
    return (step / 2.0 + quantum).T


# ---------------------------------------------------------------------------------------------------------------------------------
KINDS = ("normal", "ties", "constant", "const_col", "max_col", "signs", "fbank")


def make_matrix(kind, rows, cols, seed=0):
    rng = np.random.RandomState(seed * 7919 + rows * 131 + cols)
    if kind == "normal":
        m = 1.0 + 3.0 * rng.randn(rows, cols)
    elif kind == "ties":                                      # integer values: many ties at the quartile ranks
        m = np.round(1.0 + 3.0 * rng.randn(rows, cols))
    elif kind == "constant":                                  # max == min
        m = np.full((rows, cols), -7.25)
    elif kind == "const_col":                                 # the forced + 1 chain
        m = 1.0 + 3.0 * rng.randn(rows, cols)
        m[:, cols // 2] = 0.5
    elif kind == "max_col":                                   # one column at the global maximum throughout: the 65532 / 65533 / 65534 clamps
        m = 1.0 + 3.0 * rng.randn(rows, cols)
        m[:, cols - 1] = m.max()
    elif kind == "signs":                                     # both signs and both zeros
        m = rng.randn(rows, cols)
        flat = m.reshape(-1)
        flat[::5] = 0.0
        flat[2::7] = -0.0
        m[0, 0], m[rows - 1, cols - 1] = -2.5, 3.5
    elif kind == "fbank":                                     # log-mel-like: an energy column in front, smooth in time
        t = np.arange(rows)[:, None]
        m = 8.0 + 4.0 * np.sin(t / 17.0 + np.arange(cols)[None] / 5.0) + rng.randn(rows, cols)
        m[:, 0] = 14.0 + 3.0 * rng.rand(rows)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(m, dtype=F)


# the golden entries (tests/gen_compress_golden.py): (kind, rows, cols), all kinds, both formats, every branch of the percentile chain
GOLDEN_CASES = [("normal", 1, 23), ("normal", 4, 1), ("ties", 8, 23), ("normal", 9, 23), ("ties", 65, 23), ("constant", 9, 5), ("const_col", 64, 23),
                ("max_col", 63, 23), ("signs", 257, 7), ("fbank", 257, 80), ("constant", 2, 3), ("normal", 5, 1)]

# the single-matrix cases of the GPU test: every row count x a few widths, then the kinds at 257 x 80 and 9 x 23
ROWS = (1, 2, 4, 5, 8, 9, 63, 64, 65, 257)
DIMS = (1, 23, 64, 65, 80)
SHAPE_CASES = [("normal", r, d) for i, r in enumerate(ROWS) for d in (DIMS[i % len(DIMS)], DIMS[(i + 2) % len(DIMS)])]
KIND_CASES = [(k, r, d) for k in ("normal", "ties", "constant", "const_col", "max_col", "signs") for r, d in ((257, 80), (9, 23))]
BATCH_ROWS = (9, 1, 300, 8, 65, 5, 1000)
