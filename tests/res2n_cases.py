"""One-op programs around the 64-wide Res2 chain kernel (res2n_chain_kernel, kernels_res2n.hip), their inputs, their float64 reference
and the error measures (TEST INFRASTRUCTURE, shared by tests/test_ecapa_bench_host.py and tests/test_gpu_res2n_kernel.py).

A case is  features[in_off : in_off + (n + 1) * 64] -> res2n -> statistics pooling (mean and std)  built with libs.amd.ir.Graph;
`unfused_graph` is the same arithmetic as n dependent TDNN ops and the pass-through copy (the per-branch path).  Columns of the
features outside the input view hold FILL, the output view starts at `out_off` of its buffer.  The read-out is the statistics
pooling, pinned to 1e-5 by tests/test_gpu_pool_kernels.py.

The reference restates the chain per utterance in float64 (zero padding at the utterance ends, no row layout) and rounds where the
kernel's contract rounds: every y to the element type where it is stored, the next input as round(round(y) + x).

Exact family: features are integers in [-2, 2].  Every output channel of a branch has ONE or TWO nonzero weights, each -1 or +1, at
random (tap, input channel) positions; bias (if present) and shift are integers in [-1, 1], scale is 1.  So every value is an integer,
and with B_u the bound of a branch's input (2 for the first), |y| <= nnz * B_u + 2 and the next input is bounded by |y| + 2: a branch
takes two nonzeros per channel while that keeps |y| <= 254 and one otherwise (n = 7: two in the first five branches - bounds 6, 18, 42,
90, 186 -, then 190, 194).  Integers below 256 are exact in bf16 and in IEEE half and their f32 sums are exact in any order: no
operation and no store on the device can round, and device and float64 agree to the pooling's arithmetic alone (TOL_EXACT = 1e-5,
mean and std blocks separately).

Random family: Gaussian features and weights (standard deviation 1 / sqrt(3 * 64)) rounded to the element type, scale in [0.5, 1.5],
shift and bias Gaussian.  Device and reference share every rounding point and differ by the f32 summation order: a sum that falls on
the other side of a rounding boundary is one unit in the last place of one element.  The bound is not a constant: the test measures
the per-branch path's error on the same case and allows the fused kernel twice that.

Batches: `RAGGED` (lengths 1, 2, 3, 27, 28, 29, M - 1, M, M + 1, 2 M + 5 with M = 192, the kernel's output rows per workgroup, and one
of 150 frames: with 4 gap rows in front, lengths next to multiples of M alone put every segment end BEHIND a tile edge; the order was
found by search: first and last frames of utterances inside the 32 recomputed rows before and behind a tile edge, a tile edge inside
a 3-frame utterance - seam_report(), asserted on the host) and `SMALL` (less than one tile).  An utterance of T frames owns T rows with 4 zero rows before, between and behind
(asv_internal.h kHalo); the total is padded to 256.
"""

import functools
import zlib

import numpy as np

from helpers import rel_err
from pool_cases import round_to

W = 64
M = 192                    # capi.RES2N_TILE_ROWS (asserted on the host)
MARGIN = 32
HALO = 4
FILL = 3.0                 # what the feature columns outside the input view hold
EPS = 1e-10
TOL_EXACT = 1e-5
RAGGED = (3, M, M - 1, 1, 2 * M + 5, 150, M + 1, 2, 28, 27, 29)
SMALL = (3, 40, 1)
OFFSETS = ((0, 0), (64, 64), (0, 64), (64, 0))


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


class Case(object):
    """d: dilation; first: group 0 passes through (otherwise the last); n: convolved groups; bias: present; in_off / out_off: channel
    offsets of the views; exact: the family."""

    def __init__(self, d, first, n, bias, in_off, out_off, exact):
        self.d, self.first, self.n, self.bias, self.in_off, self.out_off, self.exact = d, first, n, bias, in_off, out_off, exact
        self.key = (d, first, n, bias, in_off, out_off, exact)

    @property
    def pass_group(self):
        return 0 if self.first else self.n

    @property
    def channels(self):
        return (self.n + 1) * W

    @property
    def feat_dim(self):
        return self.in_off + self.channels + 16

    @property
    def name(self):
        return "res2n[d=%d pass=%s n=%d bias=%d in+%d out+%d %s]" % (self.d, "first" if self.first else "last", self.n, self.bias, self.in_off,
                                                                     self.out_off, "exact" if self.exact else "random")

    __repr__ = name.fget

    def groups(self):
        """the convolved groups in chain order"""
        return [g for g in range(self.n + 1) if g != self.pass_group]


def all_cases(exact):
    out = []
    for d in (2, 3, 4):
        for first in (True, False):
            for n in (1, 7):
                for bias in (True, False):
                    in_off, out_off = OFFSETS[len(out) % len(OFFSETS)]
                    out.append(Case(d, first, n, bias, in_off, out_off, exact))
    return out


# ------------------------------------------------------------------------------------------ the row layout

def row_layout(lens):
    """(first row of every utterance, padded row count)"""
    row0, row = [], HALO
    for T in lens:
        row0.append(row)
        row += T + HALO
    return row0, -(-row // 256) * 256


def seam_report(lens):
    """Counts over the tile edges (multiples of M rows): last / first frames of utterances inside the MARGIN rows before / behind an
    edge (last_before, last_behind, first_before, first_behind) and edges inside an utterance of at most 3 frames (inside_short)."""
    row0, total = row_layout(lens)
    out = dict(last_before=0, last_behind=0, first_before=0, first_behind=0, inside_short=0)
    for s in range(M, total, M):
        for a, T in zip(row0, lens):
            last = a + T - 1
            out["last_before"] += s - MARGIN <= last < s
            out["last_behind"] += s <= last < s + MARGIN
            out["first_before"] += s - MARGIN <= a < s
            out["first_behind"] += s <= a < s + MARGIN
            out["inside_short"] += T <= 3 and a <= s < a + T
    return out


# ------------------------------------------------------------------------------------------ plans (inputs and constants)

@functools.lru_cache(maxsize=None)
def _plan_cached(key, et, lens):
    case = _BY_KEY[key]
    r = _rng(key, lens)
    n, d = case.n, case.d
    weight = np.zeros((n, W, W, 2 * d + 1), dtype=np.float32)
    if case.exact:
        x = [r.randint(-2, 3, (T, case.channels)).astype(np.float32) for T in lens]
        bound = 2
        for b in range(n):
            nnz = 2 if 2 * bound + 2 <= 254 else 1
            for co in range(W):
                for _ in range(nnz):                                    # (two draws may hit one position: then one nonzero)
                    weight[b, co, r.randint(W), d * r.randint(3)] = r.choice([-1.0, 1.0])
            bound = nnz * bound + 2 + 2
        bias = r.randint(-1, 2, (n, W)).astype(np.float32)
        scale, shift = np.ones((n, W), dtype=np.float32), r.randint(-1, 2, (n, W)).astype(np.float32)
    else:
        x = [round_to(r.randn(T, case.channels), et) for T in lens]
        weight[:, :, :, ::d] = round_to(r.randn(n, W, W, 3) / np.sqrt(3.0 * W), et)
        bias = (0.1 * r.randn(n, W)).astype(np.float32)
        scale, shift = r.uniform(0.5, 1.5, (n, W)).astype(np.float32), (0.2 * r.randn(n, W)).astype(np.float32)
    feats = []
    for m in x:
        f = np.full((m.shape[0], case.feat_dim), FILL, dtype=np.float32)
        f[:, case.in_off:case.in_off + case.channels] = m
        f.setflags(write=False)
        feats.append(f)
    consts = dict(weight=weight, bias=bias if case.bias else None, scale=scale, shift=shift)
    for a in consts.values():
        if a is not None:
            a.setflags(write=False)
    return tuple(feats), consts


_BY_KEY = {}


def plan(case, et, lens=RAGGED):
    """(feats, constants) of the case, built once; leave both unchanged."""
    _BY_KEY.setdefault(case.key, case)
    return _plan_cached(case.key, et, tuple(lens))


def fused_graph(case, et, lens=RAGGED):
    """(graph, feats): the ONE res2n op and the pooling; a fresh Graph per call (an Engine keeps pointers into its arrays)."""
    from libs.amd import ir
    feats, c = plan(case, et, lens)
    g = ir.Graph(case.feat_dim)
    out = ir.View(g.new_tensor(ir.DOMAIN_FRAMES, case.out_off + case.channels), case.out_off, case.channels)
    g.ops.append(ir.Op("res2n", out, inp=ir.View(0, case.in_off, case.channels), width=W, groups=case.n + 1, pass_group=case.pass_group,
                       dilation=case.d, weight=np.array(c["weight"]), bias=None if c["bias"] is None else np.array(c["bias"]),
                       scale=np.array(c["scale"]), shift=np.array(c["shift"])))
    g.output = g.pool(out, stddev=True, eps=EPS)
    return g, list(feats)


def unfused_graph(case, et, lens=RAGGED):
    """(graph, feats): the same chain as n dependent TDNN ops writing slices of the output buffer, and the pass-through copy."""
    from libs.amd import ir
    feats, c = plan(case, et, lens)
    g = ir.Graph(case.feat_dim)
    O = g.new_tensor(ir.DOMAIN_FRAMES, case.out_off + case.channels)
    taps, prev = [-case.d, 0, case.d], None
    for b, grp in enumerate(case.groups()):
        xin = ir.View(0, case.in_off + grp * W, W)
        y = g.tdnn(xin if prev is None else prev, np.array(c["weight"][b]), None if c["bias"] is None else np.array(c["bias"][b]), taps, -case.d,
                   act1="relu", scale=np.array(c["scale"][b]), shift=np.array(c["shift"][b]), inp2=None if prev is None else xin)
        g.ops[-1].out = prev = ir.View(O, case.out_off + grp * W, W)           # what cat elision does: write the slice
        del y
    p = case.pass_group
    g.ops.append(ir.Op("eltwise", ir.View(O, case.out_off + p * W, W), a=ir.View(0, case.in_off + p * W, W), b=None, c=None, seg_scale=None, scale=None,
                       shift=None, act=None, seg_norm=None, seg_norm_mode=0))
    g.output = g.pool(ir.View(O, case.out_off, case.channels), stddev=True, eps=EPS)
    return g, list(feats)


# ------------------------------------------------------------------------------------------ reference

def chain(case, x, c, et, dtype=np.float64, order=0):
    """x [T, (n + 1) * 64] -> cat(y_0 .. y_n) [T, (n + 1) * 64] of `dtype`; et None: no rounding.  order 1: taps descending, input
    channels in 16-channel groups from the last to the first (another summation order)."""
    rnd = (lambda a: a) if et is None else (lambda a: round_to(a, et).astype(dtype))
    x = np.asarray(x, dtype=dtype)
    T, d = x.shape[0], case.d
    y = np.zeros_like(x)
    p = case.pass_group
    y[:, p * W:(p + 1) * W] = x[:, p * W:(p + 1) * W]
    u = None
    for b, grp in enumerate(case.groups()):
        xg = x[:, grp * W:(grp + 1) * W]
        u = xg if u is None else rnd(u + xg)
        z = np.zeros((T, W), dtype=dtype)
        for k in ((0, 1, 2) if order == 0 else (2, 1, 0)):
            off = (k - 1) * d
            lo, hi = max(0, -off), min(T, T - off)
            if hi <= lo:
                continue
            wk = c["weight"][b][:, :, k * d].T.astype(dtype)               # [in, out]
            if order == 0:
                z[lo:hi] += u[lo + off:hi + off] @ wk
            else:
                for c0 in range(W - 16, -1, -16):
                    z[lo:hi] += np.ascontiguousarray(u[lo + off:hi + off, c0:c0 + 16]) @ wk[c0:c0 + 16]
        if c["bias"] is not None:
            z = z + c["bias"][b].astype(dtype)
        u = rnd(np.maximum(z, 0) * c["scale"][b].astype(dtype) + c["shift"][b].astype(dtype))
        y[:, grp * W:(grp + 1) * W] = u
    return y


def evaluate(case, et, lens=RAGGED, dtype=np.float64, rounding=True, order=0):
    """The case's program on every utterance alone -> [B, 2 * channels] = [mean | std]."""
    feats, c = plan(case, et, lens)
    out = []
    for f in feats:
        y = chain(case, f[:, case.in_off:case.in_off + case.channels], c, et if rounding else None, dtype, order)
        mean = y.mean(axis=0, dtype=dtype)
        var = ((y - mean) ** 2).sum(axis=0, dtype=dtype) / dtype(y.shape[0])
        out.append(np.concatenate([mean, np.sqrt(np.maximum(var, dtype(EPS)))]))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def _reference_cached(key, et, lens):
    ref = evaluate(_BY_KEY[key], et, lens)
    ref.setflags(write=False)
    return ref


def reference64(case, et, lens=RAGGED):
    """float64 reference (rounding where the contract rounds), computed once and shared (read-only)."""
    plan(case, et, lens)
    return _reference_cached(case.key, et, tuple(lens))


# ------------------------------------------------------------------------------------------ error measures

def errors(case, got, ref):
    """{'mean': error, 'std': error}: helpers.rel_err on each block of [B, (mean | std), channels]."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape == (got.shape[0], 2 * case.channels), (got.shape, ref.shape)
    C = case.channels
    return {"mean": rel_err(got[:, :C], ref[:, :C]), "std": rel_err(got[:, C:], ref[:, C:])}


def report(case, et, tag, fused, per_branch=None):
    """The line the measured values are read from."""
    extra = "" if per_branch is None else " | per-branch mean %.2e std %.2e" % (per_branch["mean"], per_branch["std"])
    print("[res2n] case %s et %s %s fused mean %.2e std %.2e%s" % (case.name, et, tag, fused["mean"], fused["std"], extra))
