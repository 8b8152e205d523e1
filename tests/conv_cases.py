"""Short layer programs around ONE 16-bit grid convolution, their inputs, their float64 reference and the error measures (TEST
INFRASTRUCTURE, shared by tests/test_conv_reference_host.py and tests/test_gpu_grid_conv_h16.py).

A case is  grid_input -> [head layer] -> the ONE layer under test -> pool(per_bin, mean and std)  built with libs.amd.ir.Graph.
The head layer (one input channel, 9 taps, ReLU) produces the channel count the kernel under test needs; grid_conv_c1_kernel reads
the one-channel grid itself and has no head.  The per-bin pooling is the read-out (pinned to 1e-5 by tests/test_gpu_pool_kernels.py).
The reference restates the 3x3 / backward-tap / 1x1 convolution over a [T, F] map with zero padding (no row layout, no gap rows)
in float64 and rounds every layer's output to the element type, ties to even, before the next layer and before the pooling.

Exact family (forms relu, none, affine, res): features are integers in [-4, 4]; the weights of the head are drawn from {-1, 0, 1},
those of the layer under test from {-1, -1/2, 0, 1/2, 1}, independently per (tap, input channel, output channel); biases and shifts
are integers, scales powers of two; the residual is the head's output.  The head's outputs are integers in [0, 38] (exact in 8
significant bits); every partial sum of the layer under test is a multiple of 1/2 below 9 * 256 * 38 * 2 < 2^24 halves: no f32
operation on the device can round, in whatever order the matrix instruction adds.  The one rounding on the way out is the
reference's.  Bound: TOL_EXACT = 1e-5, the statistics kernels' own, mean block and std block separately.

Rounded family (forms tanh, sigmoid - stored as 2 sigmoid(z) - 1 through scale and shift -, se = ReLU times a per-utterance scale
sigmoid(W mean(head) + b)): Gaussian features and weights rounded to the element type.  Between device and reference lie the f32
summation order, the f32 tanh / exp, and output roundings that fall on the other side of a boundary: one unit in the last place of
one element, which the mean of a one-frame utterance reads out undiluted.  Such a rounding costs spacing(v) / block maximum, so the
family rides on each kernel's small map (few one-frame elements; an epilogue form does not depend on the map) with pre-activations
small enough that the outputs spread like a Gaussian and few of them lie near the block maximum.
Calibration (tests/test_conv_reference_host.py): a float32 numpy restatement with another summation order and float32 tanh / exp
against the float64 reference on the same cases; its largest error per element type is HOST_ROUNDED, the device bound TOL_ROUNDED
four times that, capped at one unit in the last place relative to the block maximum (2^-8 bf16, 2^-11 f16):
  float32 restatement   bf16 mean 9.70e-04 std 6.76e-04        f16 mean 2.62e-04 std 3.81e-04      (before the rounding: ~1e-6)
  bound                 bf16 4 x 9.75e-04 = 3.90e-03           f16 2^-11 = 4.88e-04 (the cap binds: 4 x 3.85e-04 = 1.54e-03)
Every one of the restatement's maxima IS a rounding on the other side (0.25 units bf16, 0.78 units f16 - f32 noise meets the eight
times finer f16 grid eight times as often).  Hence for f16 the restatement cannot lie within a quarter of the capped bound, and no
correctly rounded implementation could; the host test asks the quarter of the arithmetic in front of the rounding there and holds
the rounded read-out to the cap itself.  Measured on the MI355X: bf16 <= 1.50e-03, f16 <= 3.09e-04 (std block, 0.63 of the cap).

Batches: a dozen or so ragged utterances, 1-, 2- and 3-frame ones between utterances of 20 - 40 frames.  A grid segment of T
frames owns T * pitch rows (pitch = F + 1) and pitch + 2 gap rows lie around it (Domain::gap() in batch_plan.h); row_layout()
restates that rule and LENS holds, per (F, tile), lengths for which tile seams fall inside short utterances, on the first row of
an utterance and inside a gap (seam_report(); asserted on the host).
"""

import functools
import zlib

import numpy as np

from helpers import rel_err
from pool_cases import ELEM_TYPES, round_to

POS9 = [(dt, df) for dt in (-1, 0, 1) for df in (-1, 0, 1)]
POS4 = [(-1, -1), (-1, 0), (0, -1), (0, 0)]                # the backward taps of the space-to-depth form
POS1 = [(0, 0)]
POS = {9: POS9, 4: POS4, 1: POS1}

TOL_EXACT = 1e-5
ULP = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}               # one unit in the last place relative to a block maximum
HOST_ROUNDED = {"bf16": 9.75e-4, "f16": 3.85e-4}           # float32 restatement vs float64, the larger of the two blocks (module docstring)
TOL_ROUNDED = {et: min(4.0 * HOST_ROUNDED[et], ULP[et]) for et in ULP}
EPS = 1e-10

EXACT_FORMS = ("relu", "none", "affine", "res")
ROUNDED_FORMS = ("tanh", "sigmoid", "se")
C1_CHUNK_ROWS = 8                                           # C1_ROWS of kernels_conv2d.hip


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


class Case(object):
    """kernel in {'c1', 'narrow', 'wide', 's2d', 'fallback'}; cin / cout: channels of the layer under test; F bins; taps 9 / 4 / 1;
    form: the epilogue (EXACT_FORMS + ROUNDED_FORMS)."""

    def __init__(self, kernel, cin, cout, F, taps, form):
        self.kernel, self.cin, self.cout, self.F, self.taps, self.form = kernel, cin, cout, F, taps, form
        self.key = (kernel, cin, cout, F, taps, form)

    @property
    def exact(self):
        return self.form in EXACT_FORMS

    @property
    def generic(self):
        """the GENERIC epilogue instantiation (anything but bias -> [ReLU] -> scale, shift)"""
        return self.form not in ("relu", "none")

    @property
    def tile(self):
        """rows per workgroup step of the kernel under test: where its tile seams lie"""
        if self.kernel == "c1":
            return (256 // (self.cout // 8)) * C1_CHUNK_ROWS
        return 128 if self.cin == 256 else 256              # (the C = 64 persistent form: 128, every second of them a 256-row seam)

    @property
    def name(self):
        return "%s[c%d->%d F=%d taps=%d %s]" % self.key

    __repr__ = name.fget

    def tol(self, et):
        return TOL_EXACT if self.exact else TOL_ROUNDED[et]

    def elem_types(self):
        return ELEM_TYPES if self.kernel == "c1" else ("bf16", "f16")


# ------------------------------------------------------------------------------------------ case lists

def c1_cases():
    out = [Case("c1", 1, c, 82, 9, "relu") for c in (32, 40, 48, 56, 64)]          # 4 - 8 channel chunks; F = 82: halo 84 = C1_HALO
    out += [Case("c1", 1, 40, 82, 4, "none"), Case("c1", 1, 56, 82, 1, "relu"), Case("c1", 1, 64, 82, 4, "relu")]
    out += [Case("c1", 1, 56, 3, 9, "relu"), Case("c1", 1, 64, 3, 9, "none")]
    out += [Case("c1", 1, 48, 82, 9, "affine"), Case("c1", 1, 56, 3, 4, "affine")]
    return out


# the rounded family rides on the small maps: an epilogue form does not depend on the map, and fewer one-frame elements mean fewer
# roundings on the other side (module docstring)
NARROW_FORMS = {82: EXACT_FORMS, 61: ("relu", "affine", "res"), 8: ("none", "res") + ROUNDED_FORMS}


def narrow_cases(C, F=None):
    return [Case("narrow", C, C, f, 9, form) for f in ((F,) if F else (82, 61, 8)) for form in NARROW_FORMS[f]]


def ring_cases():
    """what the capped persistent launches walk: both epilogues, the widest map (most rows: the ring wraps most often)"""
    return [Case("narrow", C, C, 82, 9, form) for C in (32, 64) for form in ("relu", "res")]


WIDE_MAPS = {128: (22, 10), 256: (14, 5)}                   # the largest map the 24- / 16-row halo admits, and a small one


def wide_cases(C):
    big, small = WIDE_MAPS[C]
    return ([Case("wide", C, C, big, 9, form) for form in EXACT_FORMS] +
            [Case("wide", C, C, small, 9, form) for form in ("relu", "res") + ROUNDED_FORMS])


def s2d_cases():
    return ([Case("s2d", 128, 64, 46, 4, form) for form in EXACT_FORMS] +                                # reach 48 = S2D_HLO
            [Case("s2d", 128, 64, 20, 4, form) for form in ("relu", "res") + ROUNDED_FORMS])


def fallback_cases():
    """one bin too wide for the wide kernel's halo (the generic tile takes taps beyond +-4 rows with the plain epilogue only: asking
    it for a residual is an error, not a result)"""
    return [Case("fallback", C, C, F, 9, form) for C, F in ((128, 23), (256, 15)) for form in ("relu", "none")]


def independence_cases():
    return [Case("c1", 1, 40, 82, 9, "relu"), Case("narrow", 32, 32, 61, 9, "relu"), Case("narrow", 64, 64, 8, 9, "res"),
            Case("wide", 128, 128, 22, 9, "relu"), Case("wide", 256, 256, 14, 9, "res"), Case("s2d", 128, 64, 46, 4, "relu")]


def all_cases():
    return c1_cases() + narrow_cases(32) + narrow_cases(64) + wide_cases(128) + wide_cases(256) + s2d_cases() + fallback_cases()


# ------------------------------------------------------------------------------------------ batches and the row layout

# (F, tile) -> utterance lengths (found by a search over lengths in 1 .. 3 and 20 .. 40; seam_report() states what they achieve)
LENS = {
    (3, 256): (34, 23, 3, 24, 1, 23, 2, 3, 1, 25, 1, 29, 2, 1),
    (3, 288): (1, 21, 1, 2, 30, 3, 2, 34, 36, 30, 31, 3, 3, 24, 1, 2),
    (5, 128): (34, 2, 3, 2, 1, 34, 32, 3, 1, 2, 3, 39, 37, 2, 2),
    (8, 256): (26, 27, 1, 21, 2, 3, 34, 1, 1, 3, 36, 1, 2, 31, 29),
    (10, 256): (35, 1, 2, 22, 3, 3, 40, 1, 1, 27, 37, 35, 27, 1, 2, 2),
    (14, 128): (1, 1, 2, 1, 28, 1, 40, 3, 39, 3, 1, 2, 25, 2, 32),
    (15, 128): (34, 26, 1, 2, 3, 30, 39, 30, 3, 1, 33, 3, 2, 3, 31, 1),
    (20, 256): (23, 2, 1, 28, 3, 3, 36, 3, 21, 22, 36, 2, 3, 20, 1, 1),
    (22, 256): (1, 34, 37, 2, 2, 32, 40, 1, 3, 3, 3, 34, 25, 2),
    (23, 256): (3, 3, 3, 1, 2, 3, 20, 2, 20, 23, 3, 1, 26, 2, 40),
    (46, 256): (28, 1, 1, 3, 37, 35, 32, 37, 2, 3, 40, 1, 2, 3, 3),
    (61, 256): (2, 3, 25, 2, 2, 39, 2, 3, 2, 1, 1, 21, 1, 34),
    (82, 256): (3, 31, 2, 21, 1, 38, 3, 2, 37, 23, 1, 33),
    (82, 288): (2, 3, 1, 1, 2, 22, 1, 3, 2, 29, 3, 29, 30, 3),
    (82, 336): (2, 1, 32, 1, 3, 3, 1, 31, 26, 1, 1, 2, 2, 2, 2),
    (82, 408): (31, 31, 3, 35, 2, 37, 3, 30, 23, 1, 2, 2, 1, 3),
    (82, 512): (22, 2, 1, 3, 40, 3, 1, 3, 2, 2, 28, 2, 37, 24, 3, 1),
}


def row_layout(lens, F):
    """(first row of every utterance, rows of every utterance, padded row count): segments of T * pitch rows with pitch + 2 gap rows
    before, between and behind them; the total padded to 256 rows."""
    pitch, gap = F + 1, F + 3
    row0, row = [], gap
    for T in lens:
        row0.append(row)
        row += T * pitch + gap
    return row0, [T * pitch for T in lens], -(-row // 256) * 256


def seam_report(lens, F, tile):
    """{'inside_short': n, 'first_row': n, 'gap': n}: tile seams (multiples of `tile` rows) strictly inside an utterance of at most 3
    frames, on the first row of an utterance, strictly inside a gap between two utterances."""
    row0, rows, total = row_layout(lens, F)
    out = dict(inside_short=0, first_row=0, gap=0)
    for s in range(tile, total, tile):
        for i, (a, n) in enumerate(zip(row0, rows)):
            if s == a:
                out["first_row"] += 1
            elif a < s < a + n and lens[i] <= 3:
                out["inside_short"] += 1
            elif i > 0 and row0[i - 1] + rows[i - 1] <= s < a:
                out["gap"] += 1
    return out


def lengths(case):
    return LENS[(case.F, case.tile)]


# ------------------------------------------------------------------------------------------ plans (inputs and weights) and graphs

DYADIC = np.array([-1.0, -0.5, 0.0, 0.5, 1.0])


def _layer(w, pos, bias, scale=None, shift=None, affine_first=False, act=None, res=False, se=None):
    return dict(w=np.ascontiguousarray(w, dtype=np.float32), pos=pos, bias=np.asarray(bias, dtype=np.float32),
                scale=None if scale is None else np.asarray(scale, dtype=np.float32), shift=None if shift is None else np.asarray(shift, dtype=np.float32),
                affine_first=affine_first, act=act, res=res, se=se)


@functools.lru_cache(maxsize=None)
def _plan_cached(key, et):
    case = _BY_KEY[key]
    r = _rng(*key)
    lens = lengths(case)
    pos = POS[case.taps]
    layers = []
    if case.exact:
        feats = [r.randint(-4, 5, (T, case.F)).astype(np.float32) for T in lens]
        if case.kernel != "c1":
            layers.append(_layer(r.randint(-1, 2, (case.cin, 1, 9)), POS9, r.randint(-2, 3, case.cin), act="relu"))
        w = DYADIC[r.randint(0, 5, (case.cout, case.cin, len(pos)))]
        bias = r.randint(-2, 3, case.cout)
        scale, shift = 2.0 ** r.randint(-1, 2, case.cout), r.randint(-1, 2, case.cout)
        act = None if case.form == "none" else "relu"
        layers.append(_layer(w, pos, bias, scale, shift, affine_first=case.form == "affine", act=act, res=case.form == "res"))
    else:
        feats = [round_to(r.randn(T, case.F), et) for T in lens]
        layers.append(_layer(round_to(r.randn(case.cin, 1, 9) / 3.0, et), POS9, 0.2 * r.randn(case.cin), act="relu"))
        # E[head^2] ~ 0.5: pre-activations of standard deviation ~0.2 (tanh), ~0.4 (sigmoid, stored as 2 sigmoid(z) - 1 through
        # scale and shift), ~1 (se): outputs spread like a Gaussian around 0, few of them near the block maximum
        std = {"tanh": 0.2, "sigmoid": 0.4, "se": 1.0}[case.form]
        w = round_to(std * r.randn(case.cout, case.cin, len(pos)) / np.sqrt(0.5 * case.cin * len(pos)), et)
        bias = 0.1 * std * r.randn(case.cout)
        if case.form == "se":
            se = (r.randn(case.cout, case.cin).astype(np.float32) / np.float32(np.sqrt(case.cin)) * np.float32(4.0), (0.5 * r.randn(case.cout)).astype(np.float32))
            layers.append(_layer(w, pos, bias, act="relu", se=se))
        elif case.form == "sigmoid":
            layers.append(_layer(w, pos, bias, np.full(case.cout, 2.0), np.full(case.cout, -1.0), act="sigmoid"))
        else:
            layers.append(_layer(w, pos, bias, act=case.form))
    for m in feats:
        m.setflags(write=False)
    return tuple(feats), tuple(layers)


_BY_KEY = {}


def plan(case, et):
    """(feats, layers) of the case, built once; leave both unchanged."""
    _BY_KEY.setdefault(case.key, case)
    return _plan_cached(case.key, et)


def _dense(w, pos, pitch):
    """[Cout, Cin, len(pos)] -> (taps, left, dense [Cout, Cin, span]) in row offsets dt * pitch + df"""
    offs = [dt * pitch + df for dt, df in pos]
    order = np.argsort(offs)
    taps = [offs[i] for i in order]
    left = taps[0]
    dense = np.zeros((w.shape[0], w.shape[1], taps[-1] - left + 1), dtype=np.float32)
    for i in order:
        dense[:, :, offs[i] - left] = w[:, :, i]
    return taps, left, dense


def build(case, et):
    """(graph, feats) for the engine; a fresh Graph per call (an Engine keeps pointers into its arrays)."""
    from libs.amd import ir
    feats, layers = plan(case, et)
    g = ir.Graph(case.F)
    v = g.grid_input()
    pitch = g.grid_spec(v.tid)[3]
    head = None
    for L in layers:
        taps, left, dense = _dense(L["w"], L["pos"], pitch)
        kw = {}
        if L["se"] is not None:
            m = g.pool(head, stddev=False)
            kw["seg_scale"] = g.tdnn(m, L["se"][0][:, :, None], L["se"][1], [0], 0, act1="sigmoid")
        if L["res"]:
            kw["res"] = ir.View(head.tid, 0, L["w"].shape[0])
        v = g.tdnn(v, dense, L["bias"], taps, left, act1=L["act"], scale=L["scale"], shift=L["shift"], affine_first=L["affine_first"], **kw)
        if head is None:
            head = v
    g.output = g.pool(v, stddev=True, per_bin=True, eps=EPS)
    return g, list(feats)


# ------------------------------------------------------------------------------------------ reference

def _act(z, name):
    if name == "relu":
        return np.maximum(z, 0)
    if name == "tanh":
        return np.tanh(z)
    if name == "sigmoid":
        return 1 / (1 + np.exp(-z))
    assert name is None, name
    return z


def _shifted(x, dt, df):
    """x [T, F, C] -> x[t + dt, f + df] with zeros outside the map"""
    T, F, _ = x.shape
    src = np.zeros_like(x)
    t0, t1 = max(0, -dt), min(T, T - dt)
    f0, f1 = max(0, -df), min(F, F - df)
    if t0 < t1 and f0 < f1:
        src[t0:t1, f0:f1] = x[t0 + dt:t1 + dt, f0 + df:f1 + df]
    return src


def conv_map(x, w, pos, order=0, fault=None):
    """x [T, F, Cin], w [Cout, Cin, len(pos)] (both of the working dtype) -> [T, F, Cout] in that dtype.
    order 0: taps ascending, one product per tap.  order 1: taps descending, every tap in 16-channel groups from the last to the
    first, added one by one (another f32 summation order).
    fault (self-test of the cases): 'drop_tap' leaves out the tap (0, -1) - (0, 0) for a 1-tap layer - at the first frame;
    'swap_groups' swaps the first two 16-channel groups of the input channels (with one input channel: the first two 8-channel
    chunks of the output channels)."""
    dtype = x.dtype
    if fault == "swap_groups":
        w = w.copy()
        if w.shape[1] >= 32:
            w[:, 0:16], w[:, 16:32] = w[:, 16:32].copy(), w[:, 0:16].copy()
        else:
            w[0:8], w[8:16] = w[8:16].copy(), w[0:8].copy()
    y = np.zeros(x.shape[:2] + (w.shape[0],), dtype=dtype)
    taps = list(range(len(pos)))
    dropped = pos.index((0, -1)) if (0, -1) in pos else 0
    for k in (taps if order == 0 else taps[::-1]):
        src = _shifted(x, *pos[k])
        if fault == "drop_tap" and k == dropped:
            src[0] = 0
        wk = np.ascontiguousarray(w[:, :, k].T)
        src2, y2 = src.reshape(-1, src.shape[2]), y.reshape(-1, y.shape[2])
        if order == 0 or wk.shape[0] < 32:
            y2 += src2 @ wk
        else:
            for c0 in range(wk.shape[0] - 16, -1, -16):
                y2 += np.ascontiguousarray(src2[:, c0:c0 + 16]) @ wk[c0:c0 + 16]
    return y


def evaluate(case, et, dtype=np.float64, order=0, fault=None, raw=None):
    """The case's program on every utterance alone -> [B, F * 2 * cout] in the engine's column order (bin f: [mean | std]).
    Every layer's output is rounded to `et` (ties to even).  `raw`: a list that receives the UNROUNDED outputs of the layer under
    test, one [T, F, cout] array of `dtype` per utterance."""
    feats, layers = plan(case, et)
    out = []
    for m in feats:
        x = np.asarray(m, dtype=dtype)[:, :, None]
        head = None
        for li, L in enumerate(layers):
            last = li == len(layers) - 1
            z = conv_map(x, L["w"].astype(dtype), L["pos"], order, fault if last else None) + L["bias"].astype(dtype)
            s = dtype(1) if L["scale"] is None else L["scale"].astype(dtype)
            t = dtype(0) if L["shift"] is None else L["shift"].astype(dtype)
            z = _act(z * s + t, L["act"]) if L["affine_first"] else _act(z, L["act"]) * s + t
            if L["se"] is not None:
                # the device's squeeze: the sum over the map divided by frames * pitch (the zero row of every frame counts)
                sq = head.sum(axis=(0, 1), dtype=dtype) / dtype(head.shape[0] * (case.F + 1))
                z = z * _act(L["se"][0].astype(dtype) @ sq + L["se"][1].astype(dtype), "sigmoid")
            if L["res"]:
                z = z + head[:, :, :z.shape[2]]
            if last and raw is not None:
                raw.append(z)
            x = round_to(z, et).astype(dtype)
            if head is None:
                head = x
        mean = x.mean(axis=0, dtype=dtype)                                       # [F, C]
        var = ((x - mean) ** 2).sum(axis=0, dtype=dtype) / dtype(x.shape[0])
        out.append(np.concatenate([mean, np.sqrt(np.maximum(var, dtype(EPS)))], axis=1).reshape(-1))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def _reference_cached(key, et):
    ref = evaluate(_BY_KEY[key], et)
    ref.setflags(write=False)
    return ref


def reference64(case, et):
    """float64 reference of the case, computed once and shared (read-only)."""
    plan(case, et)
    return _reference_cached(case.key, et)


# ------------------------------------------------------------------------------------------ error measures

def errors(case, got, ref):
    """{'mean': error, 'std': error}: helpers.rel_err on each block of [B, F, (mean | std), C]."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    g4, r4 = got.reshape(got.shape[0], case.F, 2, case.cout), ref.reshape(ref.shape[0], case.F, 2, case.cout)
    return {"mean": rel_err(g4[:, :, 0], r4[:, :, 0]), "std": rel_err(g4[:, :, 1], r4[:, :, 1])}


def report(case, et, errs, note=""):
    """The line the pull request's error table is read from."""
    print("[conv] case %s et %s err mean %.2e std %.2e tol %.2e%s" % (case.name, et, errs["mean"], errs["std"], case.tol(et), note))
