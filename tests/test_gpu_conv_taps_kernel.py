"""The tap-table grid convolution kernel (kernels_conv_taps.hip, asv_net_add_grid_conv) alone, per element type, against float64.

A case (tests/conv_taps_cases.py) is  grid_input (reach-2 grid) -> head -> ONE grid convolution -> per-bin pooling, on the exact input
family: no f32 operation on the device can round, so device and reference differ by the pooling's arithmetic alone - 1e-5, mean
block and std block separately (the bound of tests/test_gpu_grid_conv_h16.py).  bf16, f16 and f32 instantiations; widths 1, 2, 3, 5,
20 and 80 (the largest window); 32 -> 32, 64 -> 64, 128 -> 128 (several channel chunks) and 32 -> 96 (a partial output tile) channels;
the 17-tap RepSPK table, all 25 taps, and the lone corner taps (+2, +2) and (-2, -2).  Every case prints its measured error.

Which kernel ran: asv_kernel_launch_count(KERNEL_CONV_TAPS) moves by exactly one per extraction; of the other grid convolution
kernels only the head's may move (grid_conv_c1_kernel, at most once).
"""

import numpy as np
import pytest

import conv_cases as CC
import conv_taps_cases as TC

pytestmark = pytest.mark.gpu

OTHERS = ("CONV_NARROW", "CONV_NARROW_PERS", "CONV_WIDE", "CONV_S2D")


def _counts():
    from libs.amd import capi
    L = capi.lib()
    return {n: int(L.asv_kernel_launch_count(getattr(capi, "KERNEL_" + n))) for n in ("CONV_TAPS", "CONV_C1") + OTHERS}


def _extract(case, et, batches=None):
    """One Engine for the case; its batch (or every batch of `batches`) extracted; status 0; the launch counters moved as the module
    docstring says, per extraction; closed."""
    from libs.amd import engine
    graph, feats = TC.build(case)
    eng = engine.Engine(graph, precision=et)
    try:
        assert [op.kind for op in eng.ops] == ["grid_input", "tdnn", "grid_conv", "pool"]
        outs = []
        for f in ([feats] if batches is None else batches):
            before = _counts()
            outs.append(eng.extract_batch(f).numpy())
            after = _counts()
            moved = {n: after[n] - before[n] for n in after}
            assert moved["CONV_TAPS"] == 1 and moved["CONV_C1"] in (0, 1) and all(moved[n] == 0 for n in OTHERS), (case.name, et, moved)
        assert eng.status() == 0
    finally:
        eng.close()
    return outs[0] if batches is None else outs


def _check(case, et, got):
    assert not np.isnan(got).any(), (case.name, et)
    errs = TC.errors(case, got, TC.reference64(case, et))
    print("[conv_taps] case %s et %s err mean %.2e std %.2e tol %.2e" % (case.name, et, errs["mean"], errs["std"], CC.TOL_EXACT))
    for block, err in errs.items():
        assert err < CC.TOL_EXACT, (case.name, et, block, err)


@pytest.mark.parametrize("et", TC.ELEM_TYPES)
@pytest.mark.parametrize("F", TC.WIDTHS)
def test_conv_taps_kernel_vs_float64(F, et):
    """every channel shape x every tap table at this width"""
    for case in TC.cases(F):
        _check(case, et, _extract(case, et))


def test_row_tiles_at_the_widest_map():
    """F = 80: the 40-frame utterance alone covers 25 tiles of 128 rows; the batch more than 30"""
    row0, rows = TC.row_layout(80)
    assert rows // 128 > 30 and 40 * 82 // 128 == 25


@pytest.mark.parametrize("et", TC.ELEM_TYPES)
@pytest.mark.parametrize("case", [TC.Case(80, 32, 32, "spk17"), TC.Case(20, 128, 128, "full25"), TC.Case(3, 32, 96, "full25"), TC.Case(80, 64, 64, "corner_mm")],
                         ids=lambda c: "F%d-c%d-%s" % (c.F, c.cin, c.table))
def test_neighbours_do_not_change_the_bits(case, et):
    """Every utterance alone gives the bits it has in the batch - and in the batch whose OTHER utterances are scaled by 1e4: a tap
    that reached into a neighbour would carry 1e4 times the neighbour's values."""
    feats, _, _ = TC.plan(case)
    feats = list(feats)
    batches = [feats] + [[m] for m in feats]
    for i in range(len(feats)):
        batches.append([m if j == i else (m * np.float32(1e4)) for j, m in enumerate(feats)])
    outs = _extract(case, et, batches=batches)
    whole = outs[0]
    _check(case, et, whole)
    n = len(feats)
    for i in range(n):
        alone, loud = outs[1 + i], outs[1 + n + i]
        assert np.array_equal(alone[0], whole[i]), (case.name, et, i)
        assert np.array_equal(loud[i], whole[i]), (case.name, et, i, "next to neighbours scaled by 1e4")
