"""The reference side of tests/test_gpu_grid_conv_h16.py, on the host: the exact family is exact in float32 whatever the summation
order, the float32 restatement of the rounded family lies where tests/conv_cases.py says it does, the batches put tile seams where
the kernels can trip over them, the cases see the faults they are aimed at, and the launch-counter ids agree with the header."""

import os
import re

import numpy as np
import pytest

import conv_cases as CC
from helpers import REPO

KERNELS = ("c1", "narrow", "wide", "s2d", "fallback")


def _cases(kernel, exact):
    return [c for c in CC.all_cases() if c.kernel == kernel and c.exact == exact]


@pytest.mark.parametrize("kernel", KERNELS)
def test_exact_family_is_exact_in_float32_in_two_summation_orders(kernel):
    """Before the rounding, float32 in both orders equals float64 bit for bit (so no f32 operation rounded), the values are what the
    module docstring promises (multiples of 1/4 below 2^22); the same rounding then gives the reference's bits, and the float32 pooling of them is all that is left."""
    cases = _cases(kernel, True)
    assert cases
    for case in cases:
        for et in case.elem_types():
            raw64 = []
            ref = CC.evaluate(case, et, np.float64, raw=raw64)
            feats, layers = CC.plan(case, et)
            for L in layers:
                assert np.array_equal(L["w"] * 2, np.round(L["w"] * 2)) and np.abs(L["w"]).max() <= 1
            for order in (0, 1):
                raw32 = []
                got = CC.evaluate(case, et, np.float32, order, raw=raw32)
                for a, b in zip(raw32, raw64):
                    assert a.dtype == np.float32 and np.array_equal(a.astype(np.float64), b), (case.name, et, order)
                    if order == 0:
                        assert np.array_equal(b * 4, np.round(b * 4)) and np.abs(b).max() < 2 ** 22
                errs = CC.errors(case, got, ref)                 # what is left: the float32 pooling
                assert max(errs.values()) <= CC.TOL_EXACT / 4, (case.name, et, errs)


def test_head_outputs_of_the_exact_family_are_integers_of_8_bits():
    for case in (CC.narrow_cases(64)[0], CC.wide_cases(256)[0], CC.s2d_cases()[0]):
        feats, layers = CC.plan(case, "bf16")
        for m in feats:
            h = np.maximum(CC.conv_map(np.asarray(m, dtype=np.float64)[:, :, None], layers[0]["w"].astype(np.float64), layers[0]["pos"]) + layers[0]["bias"], 0)
            assert np.array_equal(h, np.round(h)) and h.max() <= 38 and np.array_equal(CC.round_to(h, "bf16"), h.astype(np.float32))


@pytest.mark.parametrize("et", ("bf16", "f16"))
def test_rounded_family_calibration(et):
    """The float32 restatement (order 1: taps descending, 16-channel groups added one by one; float32 tanh / exp) against float64.
    Its largest error is the HOST_ROUNDED the device bound is derived from (four times it, capped at one unit in the last place).
    Where the cap does not bind (bf16) the restatement is within a quarter of the bound.  Where it binds (f16) no correctly rounded
    restatement can be: an output rounding on the other side of a boundary, read out by a one-frame utterance, is by itself up to a
    whole unit.  There the quarter is asked of the arithmetic in front of the rounding - the summation order and the float32 tanh /
    exp, what the calibration is about - and the rounded read-out is held to the cap."""
    cases = [c for c in CC.all_cases() if not c.exact]
    assert {c.form for c in cases} == set(CC.ROUNDED_FORMS) and {c.kernel for c in cases} == {"narrow", "wide", "s2d"}
    worst = {"mean": 0.0, "std": 0.0, "raw": 0.0}
    for case in cases:
        raw32, raw64 = [], []
        got = CC.evaluate(case, et, np.float32, 1, raw=raw32)
        ref = CC.evaluate(case, et, np.float64, raw=raw64)
        errs = CC.errors(case, got, ref)
        scale = max(np.abs(b).max() for b in raw64)
        errs["raw"] = max(np.abs(a.astype(np.float64) - b).max() for a, b in zip(raw32, raw64)) / scale
        for k, v in errs.items():
            worst[k] = max(worst[k], v)
    print("[conv-host] rounded family %s: float32 restatement vs float64: mean %.2e std %.2e, before the rounding %.2e; bound %.2e" %
          (et, worst["mean"], worst["std"], worst["raw"], CC.TOL_ROUNDED[et]))
    host = max(worst["mean"], worst["std"])
    assert 0.9 * CC.HOST_ROUNDED[et] <= host <= CC.HOST_ROUNDED[et], (et, host)       # the recorded calibration value is the measured one
    assert CC.TOL_ROUNDED[et] == min(4 * CC.HOST_ROUNDED[et], CC.ULP[et])
    assert worst["raw"] <= CC.TOL_ROUNDED[et] / 4
    if 4 * CC.HOST_ROUNDED[et] <= CC.ULP[et]:
        assert host <= CC.TOL_ROUNDED[et] / 4
    else:
        assert host <= CC.TOL_ROUNDED[et]


def test_tile_seams_fall_where_the_kernels_can_trip():
    """Per case: the batch has 1-, 2- and 3-frame utterances and some of 20 - 40 frames, a few tens of thousands of rows at most,
    and tile seams of the kernel under test strictly inside a short utterance, on the first row of an utterance and inside a gap."""
    for case in CC.all_cases():
        lens = CC.lengths(case)
        assert 12 <= len(lens) <= 16 and all(1 <= t <= 3 or 20 <= t <= 40 for t in lens)
        assert all(lens.count(k) >= 2 for k in (1, 2, 3)) and sum(t >= 20 for t in lens) >= 3
        row0, rows, total = CC.row_layout(lens, case.F)
        assert row0[0] == case.F + 3 and total % 256 == 0 and total <= 30000
        assert all(b - (a + n) == case.F + 3 for a, n, b in zip(row0, rows, row0[1:]))
        tiles = [case.tile] + ([128] if case.kernel == "narrow" and case.cin == 64 else [])       # (C = 64: the persistent form's tiles too)
        for tile in tiles:
            rep = CC.seam_report(lens, case.F, tile)
            assert rep["inside_short"] >= 1 and rep["first_row"] >= 1 and rep["gap"] >= 1, (case.name, tile, rep)
        if case.kernel != "c1":
            assert total // case.tile >= 4                       # more than one workgroup, and a run of tiles for the capped launches


def test_halo_limits_are_the_kernels():
    """F + 2 against C1_HALO = 84, CHALO = 88, the wide kernel's 24 / 16, S2D_HLO = 48 (kernels_conv2d.hip)."""
    src = open(os.path.join(REPO, "asv-subtools_amd", "csrc", "kernels_conv2d.hip")).read()
    const = lambda pat: int(re.search(pat, src).group(1))
    assert const(r"constexpr int C1_HALO = (\d+);") == 84 == max(c.F for c in CC.c1_cases()) + 2
    assert const(r"constexpr int CHALO = (\d+);") >= 84 == max(c.F for c in CC.narrow_cases(32)) + 2
    assert (const(r"HALO = CIN == 128 \? (\d+) : \d+;"), const(r"HALO = CIN == 128 \? \d+ : (\d+);")) == (24, 16)
    assert [CC.WIDE_MAPS[C][0] + 2 for C in (128, 256)] == [24, 16]
    assert sorted((c.cin, c.F + 2) for c in CC.fallback_cases())[::2] == [(128, 25), (256, 17)]
    assert const(r"S2D_HLO = (\d+),") == 48 == max(c.F for c in CC.s2d_cases()) + 2


@pytest.mark.parametrize("et", ("bf16", "f16"))
def test_cases_see_a_dropped_tap_and_swapped_weight_groups(et):
    """Self-test of the cases: the float32 restatement with one tap left out at the first frame, and with two 16-channel groups of
    the weights swapped, is off by at least ten times the bound - in every kernel's cases, both families."""
    picks = [CC.c1_cases()[1], CC.c1_cases()[6], CC.narrow_cases(32, 8)[0], CC.narrow_cases(64, 8)[2], CC.narrow_cases(64, 8)[3], CC.narrow_cases(32, 8)[4],
             CC.wide_cases(128)[0], CC.wide_cases(256)[8], CC.s2d_cases()[0], CC.s2d_cases()[6], CC.fallback_cases()[0]]
    assert {c.form for c in picks} >= set(CC.ROUNDED_FORMS)
    for case in picks:
        ref = CC.reference64(case, et)
        for fault in ("drop_tap", "swap_groups"):
            errs = CC.errors(case, CC.evaluate(case, et, np.float32, 1, fault=fault), ref)
            print("[conv-host] %s %s %s: mean %.2e std %.2e (bound %.2e)" % (case.name, et, fault, errs["mean"], errs["std"], case.tol(et)))
            assert errs["mean"] >= 10 * case.tol(et), (case.name, et, fault, errs)


def test_graph_asks_for_what_the_reference_computes():
    """The program handed to the engine, run by the numpy interpreter of the IR (row layout, dense tap offsets, no rounding: element
    type f32), equals the map-shaped reference - every form, every tap set."""
    import ir_interp
    picks = [CC.c1_cases()[5], CC.c1_cases()[6], CC.c1_cases()[11], CC.s2d_cases()[1], CC.s2d_cases()[8]] + CC.narrow_cases(32, 8) + CC.wide_cases(128)[4:6]
    for case in picks:
        graph, feats = CC.build(case, "f32")
        assert [op.kind for op in graph.ops].count("tdnn") == (1 if case.kernel == "c1" else 2) + (case.form == "se")
        ref = CC.evaluate(case, "f32", np.float64)
        for i in (0, 2, len(feats) - 1):
            got = ir_interp.run_graph(graph, feats[i], np.float64)
            tol = 1e-12 if case.exact else 2e-6                  # (the reference rounds every layer's output to float32 here, the interpreter does not)
            assert got.shape == ref[i].shape and np.allclose(got, ref[i], rtol=tol, atol=tol), (case.name, i)


def test_every_gpu_case_is_listed_once():
    cases = CC.all_cases()
    assert len({c.key for c in cases}) == len(cases)
    listed = {c.key for c in cases}
    assert all(c.key in listed for c in CC.ring_cases() + CC.independence_cases())
    assert {c.cout for c in CC.c1_cases()} == {32, 40, 48, 56, 64} and {c.taps for c in CC.c1_cases()} == {9, 4, 1}


def test_kernel_ids_match_the_header():
    from libs.amd import capi
    header = open(os.path.join(REPO, "include", "asv_amd.h")).read()
    ids = {}
    for name in ("CONV_C1", "CONV_NARROW", "CONV_NARROW_PERS", "CONV_WIDE", "CONV_S2D"):
        ids[name] = int(re.search(r"#define\s+ASV_KERNEL_%s\s+(\d+)" % name, header).group(1))
        assert getattr(capi, "KERNEL_" + name) == ids[name]
    assert sorted(ids.values()) == [8, 9, 10, 11, 12]
    lib = capi.lib()
    assert all(lib.asv_kernel_launch_count(i) >= 0 for i in ids.values()) and lib.asv_kernel_launch_count(1 << 20) == 0 and lib.asv_kernel_launch_count(0) == 0
