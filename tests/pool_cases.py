"""One-op pooling programs, their inputs, their float64 reference and the error measures (TEST INFRASTRUCTURE, shared by
tests/test_pool_reference_host.py and tests/test_gpu_pool_kernels.py).

A program of one op runs exactly one pooling kernel of kernels_pool.hip: the op reads channel views of IR tensor 0, the feature
matrix, which the engine converts to the mode's element type with pack_input_kernel.  Every input value is rounded to that type
on the host first, so the conversion on the device is exact and the numpy reference (tests/ir_interp.py) sees the numbers the
kernel sees - no GEMM, no rounding of activations between the input and the kernel under test.

Inputs
  rows       per-channel std in [0.3, 2], |mean| <= 1 std (the one-pass variance stays well conditioned in f32)
  logits     4 * randn clipped to [-16, 16]: the spread within an utterance is at most 32 (softplus2 forms: stored values in
             [-12, 12], logits 2 log softplus in [-24, 5])
  filler     every column of tensor 0 outside the views holds FILL (finite in IEEE half): a read outside a view shows
Views start at multiples of 16 channels with 16 filler columns between and behind them.

Error measures (never one rel_err over [mean | std]: large means would hide the std half)
  rel_err    helpers.rel_err on one block: means, LDE outputs, the std of the plain statistics
  std2_err   attentive std, compared squared per channel: |got^2 - ref^2| / max over the channels of E_a[x^2], per utterance
             (kernel and reference form E[x^2] - mean^2 in f32 and the square root magnifies the cancellation when one frame
             dominates).  E_a[x^2] is taken as mean^2 + std^2 of the float64 reference (exact where the reference does not clamp,
             eps = 1e-5 off where it does; with a prior frame it includes the prior, one more frame of the utterance).  Clamped
             channels enter after the clamp on both sides.
Tolerances: TOL_STATS for the statistics kernels (the bound of test_stats_pool_vs_oracle), TOL_ATT for the attentive kernels
and LDE (the f32 kernel-level bound MODE_TOL["f32"] of tests/test_gpu_kernels.py), for all three element types.
"""

import functools
import zlib

import numpy as np

import ir_interp
from helpers import rel_err

ELEM_TYPES = ("f32", "bf16", "f16")
LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 1000)
LDE_LENGTHS = LENGTHS + (7, 8, 9)                    # lde_weights_kernel takes 8 rows per workgroup
GRID_FRAMES = (63, 64, 65, 129, 3)                   # x pitch 32: 2016, 2048, 2080, 4128 rows (kPoolChunkRows = 2048) and 96
COMBINE_LENGTHS = (257, 100, 101, 1)
COMBINE_CHUNK = 100
FILL = 3e4
TOL_STATS = 1e-5
TOL_ATT = 2e-5
ATT_EPS = 1e-5


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def round_to(a, et):
    """float32 array whose values are representable in the element type `et` (round to nearest even, like pack_input_kernel)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if et == "f32":
        return a
    import torch
    return torch.from_numpy(a).to({"bf16": torch.bfloat16, "f16": torch.float16}[et]).float().numpy()


def layout(ch_off, widths):
    """Column offsets of views of the given widths (first at ch_off, each at a multiple of 16, 16 filler columns between and
    behind them) and the width of tensor 0."""
    offs, off = [], ch_off
    for w in widths:
        offs.append(off)
        off = -(-(off + w) // 16) * 16 + 16
    return offs, off


def assemble(lens, feat_dim, blocks, et):
    """[(offset, [sum lens, w] array)] -> per-utterance feature matrices [T, feat_dim], rounded to `et`, FILL elsewhere."""
    m = np.full((int(sum(lens)), feat_dim), FILL, dtype=np.float32)
    for off, a in blocks:
        m[:, off:off + a.shape[1]] = a
    m = round_to(m, et)
    ends = np.cumsum(lens)
    return [m[e - n:e] for n, e in zip(lens, ends)]


def channel_stats(rng, channels, positive=False):
    std = rng.uniform(0.3, 2.0, channels)
    u = rng.uniform(-1.0, 1.0, channels)
    return (np.abs(u) if positive else u) * std, std


def channel_rows(rng, rows, mean, std):
    return rng.randn(rows, len(std)) * std + mean


def random_logits(rng, rows, n, lim=16.0):
    return np.clip(4.0 * rng.randn(rows, n), -lim, lim)


class Case(object):
    """family in {'stats', 'grid', 'att', 'mq', 'lde', 'combine'}; `p`: the family's parameters."""

    def __init__(self, family, **p):
        self.family, self.p = family, p
        self.key = (family,) + tuple(sorted(p.items()))

    @property
    def name(self):
        return self.family + "[" + " ".join("%s=%s" % kv for kv in sorted(self.p.items())) + "]"

    __repr__ = name.fget


# ------------------------------------------------------------------------------------------ case lists

STATS_CHANNELS = (16, 24, 32, 48, 64, 80, 200)       # <= 32: NARROW in the 16-bit modes (24: padded lanes); the others leave a partly filled last 64-channel tile
STATS_OPTIONS = [dict(stddev=False, unbiased=0, var_mode=0)] + [dict(stddev=True, unbiased=u, var_mode=v) for u in (0, 1, 2) for v in (0, 1)]
ATT_CHANNELS = (16, 48, 64, 200)
ATT_FORMS = ("chan", "shared", "group16", "sp2", "sp2prior")       # + "group50" with 200 channels
ATT_PATTERNS = ("inc", "dec", "last")                # the running maximum of the one-pass path moves every trip / never / at the last row (33 frames: second frame of a trip; 65, 129, 257: one lane of the tail loop)
MQ_HEADS = ((16, 3), (48, 2))                        # (head channels, heads): a workgroup's 64 channels span two or three heads
LDE_CENTRES = (1, 8, 9, 16, 17, 32, 33, 64)          # both sides of every KMAX instantiation
LDE_CHANNELS = (16, 80, 200)


def stats_cases(channels, ch_off):
    return [Case("stats", channels=channels, ch_off=ch_off, eps=1e-10, const=False, **o) for o in STATS_OPTIONS]


def stats_eps_cases():
    """eps = 1e-2 and a constant channel: max(var, eps) and var + eps differ in every channel."""
    return [Case("stats", channels=48, ch_off=16, eps=1e-2, const=True, stddev=True, unbiased=0, var_mode=v) for v in (0, 1)]


def grid_cases():
    return [Case("grid", per_bin=False, unbiased=0), Case("grid", per_bin=True, unbiased=0), Case("grid", per_bin=True, unbiased=1)]


def att_cases(channels, ch_off):
    forms = ATT_FORMS + (("group50",) if channels == 200 else ())
    return [Case("att", channels=channels, ch_off=ch_off, form=f, pattern="rand") for f in forms]


def att_pattern_cases():
    return [Case("att", channels=48, ch_off=16, form=f, pattern=pt) for f in ("chan", "shared") for pt in ATT_PATTERNS]


def mq_cases():
    return [Case("mq", head_ch=hc, heads=h, queries=q, shared=s) for hc, h in MQ_HEADS for q in (1, 2, 3, 4) for s in (False, True)]


def lde_cases(channels):
    return [Case("lde", channels=channels, centres=k, ch_off=0 if channels == 80 else 16) for k in LDE_CENTRES]


def combine_cases():
    return [Case("combine", channels=48, ch_off=16)]


def independence_cases():
    """One graph of each family for the neighbour-independence test (no NaN in their outputs)."""
    return [Case("stats", channels=48, ch_off=16, eps=1e-10, const=False, stddev=True, unbiased=1, var_mode=0),
            Case("stats", channels=24, ch_off=16, eps=1e-10, const=False, stddev=True, unbiased=0, var_mode=1),
            Case("grid", per_bin=False, unbiased=0),
            Case("att", channels=48, ch_off=16, form="chan", pattern="rand"),
            Case("mq", head_ch=48, heads=2, queries=2, shared=False),
            Case("lde", channels=80, centres=9, ch_off=0)]


def all_cases():
    out = []
    for c in STATS_CHANNELS:
        for off in (0, 16):
            out += stats_cases(c, off)
    out += stats_eps_cases() + grid_cases()
    for c in ATT_CHANNELS:
        for off in (0, 16):
            out += att_cases(c, off)
    out += att_pattern_cases() + mq_cases()
    for c in LDE_CHANNELS:
        out += lde_cases(c)
    return out + combine_cases()


# ------------------------------------------------------------------------------------------ graph builders

@functools.lru_cache(maxsize=None)
def _stats_feats(channels, ch_off, const, lens, et):
    rng = _rng("stats", channels, ch_off, const)
    (xo,), feat_dim = layout(ch_off, [channels])
    mean, std = channel_stats(rng, channels)
    x = channel_rows(rng, sum(lens), mean, std)
    if const:
        x[:, 5] = 0.71875                           # (representable in all three types)
    return xo, feat_dim, assemble(lens, feat_dim, [(xo, x)], et)


def _build_stats(p, et, lens=LENGTHS):
    from libs.amd import ir
    xo, feat_dim, feats = _stats_feats(p["channels"], p["ch_off"], p.get("const", False), lens, et)
    g = ir.Graph(feat_dim)
    g.output = g.pool(ir.View(0, xo, p["channels"]), stddev=p.get("stddev", True), unbiased=p.get("unbiased", 0), var_mode=p.get("var_mode", 0),
                      eps=p.get("eps", 1e-10))
    return g, feats


@functools.lru_cache(maxsize=None)
def _grid_feats(et):
    rng = _rng("grid")
    mean, std = channel_stats(rng, 31, positive=True)          # positive bin means: the mean over the whole map does not cancel
    return assemble(GRID_FRAMES, 31, [(0, channel_rows(rng, sum(GRID_FRAMES), mean, std))], et)


def _build_grid(p, et):
    from libs.amd import ir
    g = ir.Graph(31)                                            # pitch 32: the chunked mean's pitch condition holds
    g.output = g.pool(g.grid_input(), stddev=p["per_bin"], unbiased=p["unbiased"], per_bin=p["per_bin"])
    return g, _grid_feats(et)


def _pattern_logits(rng, pattern, lens, n):
    parts = []
    for T in lens:
        if pattern == "last":                                   # one dominant frame at the utterance's last row
            e = rng.uniform(-16.0, -8.0, (T, n))
            e[-1] = 14.0
        else:
            # 30 / T per row: more than one bf16 step over the 32 rows between two frames of a lane, so every lane's own
            # sequence is strictly monotone after rounding (the utterance's is monotone)
            ramp = np.linspace(-15.0, 15.0, T) if T > 1 else np.zeros(1)
            e = (ramp if pattern == "inc" else ramp[::-1])[:, None] + rng.uniform(-1.0, 1.0, n)[None, :]
        parts.append(e)
    return np.concatenate(parts)


def _build_att(p, et, lens=LENGTHS):
    from libs.amd import ir
    C, form = p["channels"], p["form"]
    rng = _rng("att", C, p["ch_off"], form, p["pattern"])
    group = {"group16": 16, "group50": 50}.get(form, 0)
    n = 1 if form == "shared" else (-(-C // group) if group else C)
    (xo, lo), feat_dim = layout(p["ch_off"], [C, n])
    mean, std = channel_stats(rng, C)
    x = channel_rows(rng, sum(lens), mean, std)
    sp2 = form in ("sp2", "sp2prior")
    e = _pattern_logits(rng, p["pattern"], lens, n) if p["pattern"] != "rand" else random_logits(rng, sum(lens), n, 12.0 if sp2 else 16.0)
    kw = {}
    if form == "sp2prior":
        # prior logits 2 .. 3 in the even channels, -20 .. -18 in the odd ones; utterance 3 stores values <= -3 (logits <= -6: the
        # prior is the maximum of its even channels), utterance 9 values >= 8 (logits >= 4.1: the prior of its odd channels is far below)
        ends = np.cumsum(lens)
        a, b = ends[3] - lens[3], ends[9] - lens[9]
        e[a:ends[3]] = np.clip(-3.0 - np.abs(e[a:ends[3]]), -12.0, -3.0)
        e[b:ends[9]] = np.clip(8.0 + np.abs(e[b:ends[9]]), 8.0, 12.0)
        kw["prior_logit"] = np.where(np.arange(C) % 2 == 0, rng.uniform(2.0, 3.0, C), rng.uniform(-20.0, -18.0, C)).astype(np.float32)
        kw["prior_value"] = (mean + std * rng.randn(C)).astype(np.float32)
    g = ir.Graph(feat_dim)
    g.output = g.attpool(ir.View(0, xo, C), ir.View(0, lo, n), eps=ATT_EPS, shared=form == "shared", group=group, softplus2=sp2, **kw)
    return g, assemble(lens, feat_dim, [(xo, x), (lo, e)], et)


def _build_mq(p, et, lens=LENGTHS):
    """The heads x queries attpool ops as the ECAPA blueprint's MQMHASP leaves them after concat elision: pair p = head * Q + query
    reads head's channel view and logit columns [p n, (p + 1) n), writes [mean | std] to columns [p 2 Ch, (p + 1) 2 Ch) of one tensor."""
    from libs.amd import ir
    Ch, H, Q, shared = p["head_ch"], p["heads"], p["queries"], p["shared"]
    rng = _rng("mq", Ch, H, Q, shared)
    n = 1 if shared else Ch
    (xo, lo), feat_dim = layout(16, [H * Ch, H * Q * n])
    mean, std = channel_stats(rng, H * Ch)
    x = channel_rows(rng, sum(lens), mean, std)
    e = random_logits(rng, sum(lens), H * Q * n)
    g = ir.Graph(feat_dim)
    outs = [g.attpool(ir.View(0, xo + h * Ch, Ch), ir.View(0, lo + (h * Q + q) * n, n), eps=ATT_EPS, shared=shared, mq=(h, q, H, Q))
            for h in range(H) for q in range(Q)]
    g.output = g.cat(outs)
    g.optimize()
    return g, assemble(lens, feat_dim, [(xo, x), (lo, e)], et)


def _build_lde(p, et):
    from libs.amd import ir
    C, K = p["channels"], p["centres"]
    rng = _rng("lde", C, K)
    (xo,), feat_dim = layout(p["ch_off"], [C])
    mean, std = channel_stats(rng, C)
    x = channel_rows(rng, sum(LDE_LENGTHS), mean, std)
    # centres within 0.3 std of the channel means: soft weights, and the sums of x - mu over 1000 frames stay small enough that
    # the float32 reference's sequential sum (numpy, one centre) keeps its quarter of the tolerance
    mu = mean[:, None] + 0.3 * std[:, None] * rng.randn(C, K)
    beta = rng.uniform(0.01, 0.1, K)
    if K > 1:
        beta[K - 1] = 50.0                                      # its logit is hundreds below the others': the weight underflows to 0
    g = ir.Graph(feat_dim)
    g.output = g.lde(ir.View(0, xo, C), mu, beta)
    return g, assemble(LDE_LENGTHS, feat_dim, [(xo, x)], et)


@functools.lru_cache(maxsize=None)
def _build_cached(case_key, et):
    case = _BY_KEY[case_key]
    p = case.p
    if case.family == "stats":
        return _build_stats(p, et)
    if case.family == "combine":
        return _build_stats(dict(p, stddev=True), et, COMBINE_LENGTHS)
    if case.family == "grid":
        return _build_grid(p, et)
    if case.family == "att":
        return _build_att(p, et)
    if case.family == "mq":
        return _build_mq(p, et)
    if case.family == "lde":
        return _build_lde(p, et)
    raise AssertionError(case.family)


_BY_KEY = {}


def build(case, et):
    """(graph, feats_list) of the case for inputs rounded to element type `et` (built once; leave both unchanged)."""
    _BY_KEY.setdefault(case.key, case)
    return _build_cached(case.key, et)


# ------------------------------------------------------------------------------------------ reference

def reference(graph, feats, dtype=np.float64, max_chunk=None, ops=None):
    """The numpy interpreter on every utterance alone -> [B, E]."""
    if max_chunk is not None:
        return np.stack([ir_interp.extract(graph, m, max_chunk=max_chunk, dtype=dtype, ops=ops) for m in feats])
    return np.stack([ir_interp.run_graph(graph, m, dtype, ops) for m in feats])


@functools.lru_cache(maxsize=None)
def _reference_cached(case_key, et):
    case = _BY_KEY[case_key]
    graph, feats = build(case, et)
    ref = reference(graph, feats, np.float64, COMBINE_CHUNK if case.family == "combine" else None)
    ref.setflags(write=False)
    return ref


def reference64(case, et):
    """float64 reference of the case, computed once and shared (read-only)."""
    build(case, et)
    return _reference_cached(case.key, et)


def expand_mqattpool(op):
    """The heads x queries attpool ops a fused 'mqattpool' op stands for, from the fused op's own fields (ir_interp evaluates
    attpool ops only): what the one-launch kernel is asked to compute."""
    from libs.amd import ir
    H, Q = op.heads, op.queries
    Ch = op.x.channels // H
    n = 1 if op.shared else Ch
    out = []
    for pair in range(H * Q):
        h = pair // Q
        o = ir.Op("attpool", ir.View(op.out.tid, op.out.ch_off + pair * op.pair_stride, 2 * Ch), x=ir.View(op.x.tid, op.x.ch_off + h * Ch, Ch),
                  logits=ir.View(op.logits.tid, op.logits.ch_off + pair * n, n), eps=op.eps, shared=op.shared, group=0, softplus2=False,
                  prior_logit=None, prior_value=None, mq=None)
        assert op.std_off == Ch                                  # [mean | std] per pair, the layout ir_interp's attpool writes
        out.append(o)
    return out


# ------------------------------------------------------------------------------------------ error measures

def std2_err(got_std, ref_mean, ref_std):
    """max over utterances and channels of |got^2 - ref^2| / max_c (ref_mean^2 + ref_std^2); [B, C] blocks."""
    got_std, ref_mean, ref_std = (np.asarray(a, dtype=np.float64) for a in (got_std, ref_mean, ref_std))
    scale = (ref_mean ** 2 + ref_std ** 2).max(axis=1, keepdims=True)
    return float((np.abs(got_std ** 2 - ref_std ** 2) / scale).max())


def _nan_rel_err(got, ref):
    """rel_err where the reference is finite; NaN exactly where the reference is NaN."""
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), "NaN in %d places, the reference in %d" % (int(np.isnan(got).sum()), int(nan.sum()))
    return rel_err(np.where(nan, 0.0, got), np.where(nan, 0.0, ref))


def errors(case, got, ref):
    """{block: (error, tolerance)} of a result [B, E] against the float64 reference, in the measure of each block."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    p, fam = case.p, case.family
    if fam in ("stats", "combine"):
        C = p["channels"]
        out = {"mean": (_nan_rel_err(got[:, :C], ref[:, :C]), TOL_STATS)}
        if p.get("stddev", True):
            out["std"] = (_nan_rel_err(got[:, C:], ref[:, C:]), TOL_STATS)
        return out
    if fam == "grid":
        if not p["per_bin"]:
            return {"mean": (rel_err(got, ref), TOL_STATS)}
        return {"mean": (rel_err(got[:, 0::2], ref[:, 0::2]), TOL_STATS), "std": (rel_err(got[:, 1::2], ref[:, 1::2]), TOL_STATS)}
    if fam == "att":
        C = p["channels"]
        return {"mean": (rel_err(got[:, :C], ref[:, :C]), TOL_ATT), "std": (std2_err(got[:, C:], ref[:, :C], ref[:, C:]), TOL_ATT)}
    if fam == "mq":
        Ch, pairs = p["head_ch"], p["heads"] * p["queries"]
        g4, r4 = got.reshape(-1, pairs, 2, Ch), ref.reshape(-1, pairs, 2, Ch)
        std = max(std2_err(g4[:, k, 1], r4[:, k, 0], r4[:, k, 1]) for k in range(pairs))
        return {"mean": (rel_err(g4[:, :, 0], r4[:, :, 0]), TOL_ATT), "std": (std, TOL_ATT)}
    if fam == "lde":
        return {"mean": (rel_err(got, ref), TOL_ATT)}
    raise AssertionError(fam)


def report(case, et, errs):
    """The line the pull request's error table is read from."""
    print("[pool] case %s %s mean %.2e std %.2e" % (et, case.name, errs["mean"][0], errs.get("std", (float("nan"),))[0]))
