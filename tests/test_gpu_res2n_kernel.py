"""res2n_chain_kernel (kernels_res2n.hip) alone: one-op programs (tests/res2n_cases.py) against their float64 reference, which rounds
where the kernel's contract rounds.

Exact family: device and float64 agree to the statistics pooling's arithmetic, 1e-5, mean and std blocks separately.
Random family: the per-branch path (the same chain as n TDNN launches) is measured against the same reference on the same case; the
fused kernel is allowed twice that error (both share every rounding point and differ by the f32 summation order; a flip at a rounding
boundary is one unit in the last place of the element type either way).

Measured on the MI355X (mean block / std block, largest over the 24 cases and both batches; `[res2n] case ...` lines):
  bf16   fused 1.35e-04 / 3.47e-04   per-branch 1.35e-04 / 3.47e-04
  f16    fused 5.72e-05 / 2.16e-04   per-branch 5.72e-05 / 2.16e-04
All 96 results are bit-equal to the per-branch path's.  Two things were needed for that: the bias is added in the epilogue, not put
into the accumulators first (bf16: 10 cases differed), and in f16 the last multiply-add and the conversion to half are ONE rounding
(v_fma_mixlo / mixhi_f16, what hipcc makes of the per-layer kernels' store) - rounding to f32 and then to half differed in 18 of 48
results, 6 of them beyond twice the per-branch error (e.g. 7.93e-05 / 9.24e-05 against 1.15e-05 / 3.54e-05).
"""

import numpy as np
import pytest

import res2n_cases as RC

pytestmark = pytest.mark.gpu


def _extract(graph, feats, et, flags=None):
    from libs.amd import capi, engine
    L = capi.lib()
    n0 = L.asv_kernel_launch_count(capi.KERNEL_RES2N)
    eng = engine.Engine(graph, precision=et, flags=flags)
    try:
        out = eng.extract_batch(feats).numpy()
        assert eng.status() == 0
        return out, L.asv_kernel_launch_count(capi.KERNEL_RES2N) - n0, eng.describe()
    finally:
        eng.close()


@pytest.mark.parametrize("et", ["bf16", "f16"])
@pytest.mark.parametrize("case", RC.all_cases(True), ids=lambda c: c.name)
def test_exact_family_vs_float64(case, et):
    for tag, lens in (("ragged", RC.RAGGED), ("small", RC.SMALL)):
        graph, feats = RC.fused_graph(case, et, lens)
        got, launches, desc = _extract(graph, feats, et)
        assert launches == 1 and "res2n" in desc
        errs = RC.errors(case, got, RC.reference64(case, et, lens))
        RC.report(case, et, tag, errs)
        assert errs["mean"] < RC.TOL_EXACT and errs["std"] < RC.TOL_EXACT, (case, et, tag, errs)


@pytest.mark.parametrize("et", ["bf16", "f16"])
@pytest.mark.parametrize("case", RC.all_cases(False), ids=lambda c: c.name)
def test_random_family_within_twice_the_per_branch_error(case, et):
    from libs.amd import capi
    for tag, lens in (("ragged", RC.RAGGED), ("small", RC.SMALL)):
        ref = RC.reference64(case, et, lens)
        graph, feats = RC.fused_graph(case, et, lens)
        got, launches, _ = _extract(graph, feats, et)
        assert launches == 1
        plain_graph, _ = RC.unfused_graph(case, et, lens)
        plain, launches, desc = _extract(plain_graph, feats, et, flags=capi.FLAG_NO_FUSE)
        assert launches == 0 and "res2n" not in desc
        fused_err, plain_err = RC.errors(case, got, ref), RC.errors(case, plain, ref)
        RC.report(case, et, tag, fused_err, plain_err)
        assert np.isfinite(got).all()
        for block in ("mean", "std"):
            assert fused_err[block] <= 2.0 * plain_err[block], (case, et, tag, block, fused_err, plain_err)
