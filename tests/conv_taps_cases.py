"""Short layer programs around ONE tap-table grid convolution (asv_net_add_grid_conv, kernels_conv_taps.hip), their inputs and their
float64 reference (TEST INFRASTRUCTURE for tests/test_gpu_conv_taps_kernel.py, on the model of tests/conv_cases.py whose
reference convolution, error measures and exact input family this file uses).

A case is  grid_input (reach-2 grid, pitch = F + 2) -> head layer (1 -> cin channels, 9 taps, ReLU: an existing kernel) -> the ONE
grid convolution under test (cin -> cout, a tap table, bias, ReLU) -> pool(per_bin, mean and std).

Exact family (conv_cases.py): features are integers in [-4, 4], the head's weights come from {-1, 0, 1} and its bias is an integer:
its outputs are integers in [0, 38], exact in 8 significant bits.  The weights of the layer under test come from {-1, -1/2, 0, 1/2, 1},
its bias is an integer: every partial sum is a multiple of 1/2 below 25 * 128 * 38 * 2 < 2^24 halves, so no f32 operation on the
device can round, in whatever order the kernel adds.  The one rounding on the way out (to the element type) is the reference's too.
Bound: conv_cases.TOL_EXACT = 1e-5, the pooling kernels' own, mean block and std block separately.

Tap tables: the 17 live taps of a folded RepSPK block, all 25, and a lone corner tap (+2, +2) / (-2, -2): with every feature
non-zero, a corner tap that wrapped into the neighbouring frame (pitch too small) or reached into the neighbouring utterance
(gap too small) reads values where the reference reads its zero padding.

Batch: utterances of 3, 40, 1, 7 and 2 frames.  At F = 80 (pitch 82, the largest window: halo 166) the 40-frame utterance covers
25 row tiles of 128 and the short ones lie within one tile of its edges.
"""

import functools

import numpy as np

import conv_cases as CC
from pool_cases import round_to

ELEM_TYPES = ("bf16", "f16", "f32")
WIDTHS = (1, 2, 3, 5, 20, 80)
CHANNELS = ((32, 32), (64, 64), (128, 128), (32, 96))           # 128: several input-channel chunks; 96: a partial output tile
LENS = (3, 40, 1, 7, 2)

SPK17 = sorted({(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)} | {(2 * a, 2 * b) for a in (-1, 0, 1) for b in (-1, 0, 1)})
TAP_TABLES = {
    "spk17": SPK17,
    "full25": [(a, b) for a in range(-2, 3) for b in range(-2, 3)],
    "corner_pp": [(2, 2)],
    "corner_mm": [(-2, -2)],
}
assert len(SPK17) == 17


class Case(object):
    def __init__(self, F, cin, cout, table):
        self.F, self.cin, self.cout, self.table = F, cin, cout, table
        self.key = (F, cin, cout, table)
        self.pos = TAP_TABLES[table]

    @property
    def name(self):
        return "taps[c%d->%d F=%d %s]" % (self.cin, self.cout, self.F, self.table)

    __repr__ = name.fget


def cases(F):
    return [Case(F, cin, cout, table) for cin, cout in CHANNELS for table in TAP_TABLES]


@functools.lru_cache(maxsize=None)
def _plan_cached(key):
    F, cin, cout, table = key
    r = CC._rng("conv_taps", *key)
    feats = []
    for T in LENS:
        m = r.randint(1, 5, (T, F)).astype(np.float32) * r.choice([-1.0, 1.0], (T, F)).astype(np.float32)       # integers in [-4, 4], never 0
        m.setflags(write=False)
        feats.append(m)
    head = dict(w=r.randint(-1, 2, (cin, 1, 9)).astype(np.float32), pos=CC.POS9, bias=r.randint(-2, 3, cin).astype(np.float32))
    pos = TAP_TABLES[table]
    layer = dict(w=CC.DYADIC[r.randint(0, 5, (cout, cin, len(pos)))].astype(np.float32), pos=pos, bias=r.randint(-2, 3, cout).astype(np.float32))
    if len(pos) == 1:
        # a lone tap: all-positive weights of 1/2 or 1, so that no output of the ReLU'd head can cancel what a stray read adds
        layer["w"] = np.abs(layer["w"]) + np.float32(0.5) * (layer["w"] == 0)
    return tuple(feats), head, layer


def plan(case):
    """(feats, head layer, layer under test), built once; leave them unchanged."""
    return _plan_cached(case.key)


def build(case, feats=None):
    """(graph, feats) for the engine; a fresh Graph per call (an Engine keeps pointers into its arrays)."""
    from libs.amd import ir
    base, head, layer = plan(case)
    g = ir.Graph(case.F)
    v = g.grid_input(reach=2)
    pitch = g.grid_spec(v.tid)[3]
    assert pitch == case.F + 2 and g.grid_reach(v.tid) == 2
    taps, left, dense = CC._dense(head["w"], head["pos"], pitch)
    v = g.tdnn(v, dense, head["bias"], taps, left, act1="relu")
    v = g.grid_conv(v, layer["w"], layer["bias"], layer["pos"], act="relu")
    g.output = g.pool(v, stddev=True, per_bin=True, eps=CC.EPS)
    return g, list(base if feats is None else feats)


def evaluate(case, et, feats=None, dtype=np.float64):
    """The case's program on every utterance alone -> [B, F * 2 * cout] in the engine's column order (bin f: [mean | std]); every
    layer's output rounded to `et`, ties to even."""
    base, head, layer = plan(case)
    out = []
    for m in (base if feats is None else feats):
        x = np.asarray(m, dtype=dtype)[:, :, None]
        for L in (head, layer):
            z = CC.conv_map(x, L["w"].astype(dtype), L["pos"]) + L["bias"].astype(dtype)
            x = round_to(np.maximum(z, 0), et).astype(dtype)
        mean = x.mean(axis=0, dtype=dtype)
        var = ((x - mean) ** 2).sum(axis=0, dtype=dtype) / dtype(x.shape[0])
        out.append(np.concatenate([mean, np.sqrt(np.maximum(var, dtype(CC.EPS)))], axis=1).reshape(-1))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def _reference_cached(key, et):
    ref = evaluate(_BY_KEY[key], et)
    ref.setflags(write=False)
    return ref


_BY_KEY = {}


def reference64(case, et):
    """float64 reference of the case, computed once and shared (read-only)."""
    _BY_KEY.setdefault(case.key, case)
    return _reference_cached(case.key, et)


def errors(case, got, ref):
    return CC.errors(case, got, ref)


def row_layout(F):
    """(first row of every utterance, padded rows) on the reach-2 grid: pitch F + 2, 2 pitch + 3 gap rows around every utterance."""
    pitch = F + 2
    gap = 2 * pitch + 3
    row0, row = [], gap
    for T in LENS:
        row0.append(row)
        row += T * pitch + gap
    return row0, -(-row // 256) * 256
