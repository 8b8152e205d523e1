"""The unpadded stride-2 subsampling front alone on the MI355X (front_conv -> im2col(valid) -> K = 9 d layer -> flatten -> Linear
-> posenc), on the exact-input family of tests/front_cases.py: nothing but the pooling rounds, so every element type is held to
conv_cases.TOL_EXACT against float64 - the reference's own convolutions, written with torch in float64.  The position channels
give the row count L(T) of every segment and show the positions restarting at every segment."""

import numpy as np
import pytest

import front_cases as FC
from conv_cases import TOL_EXACT

pytestmark = pytest.mark.gpu

PRECISIONS = ("bf16", "f16", "f32", "f32m")


def _engine(F, precision):
    from libs.amd import engine
    return engine.Engine(FC.build(F), device_index=0, precision=precision)


def _err(got, ref):
    n = FC.OUT
    return max(float(np.abs(got[:, s] - ref[:, s]).max() / max(np.abs(ref[:, s]).max(), 1e-30)) for s in (slice(0, n), slice(n, 2 * n)))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("F", FC.WIDTHS)
def test_front_is_exact_and_segments_own_L_of_T_rows(F, precision):
    from libs.amd import capi
    mats = FC.features(F)
    ref = np.stack([FC.reference_torch64(m, F) for m in mats])
    eng = _engine(F, precision)
    eng.status()
    before = int(capi.lib().asv_kernel_launch_count(capi.KERNEL_FRONT_CONV))
    got = eng.extract_batch(mats).numpy().astype(np.float64)
    assert eng.status() == 0
    assert int(capi.lib().asv_kernel_launch_count(capi.KERNEL_FRONT_CONV)) - before == 1
    err = _err(got, ref)
    print("[front] F %2d %-4s err %.3g (bound %g)" % (F, precision, err, TOL_EXACT))
    assert err <= TOL_EXACT, (F, precision, err)
    # the position channels: mean (L - 1) / 2, std sqrt((L^2 - 1) / 12) with L = L(T) rows per segment
    pos = slice(FC.OUT - FC.POS, FC.OUT)
    for i, m in enumerate(mats):
        L = FC.rows_of(m.shape[0])
        assert np.allclose(got[i, pos], (L - 1) / 2.0, rtol=1e-6, atol=0), (F, precision, m.shape[0], got[i, pos][:2])
        want_std = np.sqrt(max((L * L - 1) / 12.0, FC.POOL_EPS))
        assert np.allclose(got[i, FC.OUT:][pos], want_std, rtol=1e-5, atol=0), (F, precision, m.shape[0])


@pytest.mark.parametrize("precision", ("bf16", "f32m"))
def test_front_neighbour_independence(precision):
    """every utterance alone has the bits it has in the batch, also next to neighbours scaled by 1e4"""
    F = 11
    mats = FC.features(F)
    eng = _engine(F, precision)
    full = eng._extract_batch(mats).numpy()
    assert np.isfinite(full).all()
    for i, m in enumerate(mats):
        assert np.array_equal(eng._extract_batch([m]).numpy()[0], full[i]), (precision, i)
        loud = [x if j == i else x * np.float32(1e4) for j, x in enumerate(mats)]
        assert np.array_equal(eng._extract_batch(loud).numpy()[i], full[i]), (precision, i, "neighbours x 1e4")


def test_too_short_a_chunk_is_refused_before_any_launch():
    from libs.amd import capi
    eng = _engine(11, "f32")
    before = int(capi.lib().asv_kernel_launch_count(capi.KERNEL_FRONT_CONV))
    with pytest.raises(ValueError, match="at least 7"):
        eng.extract_batch([FC.features(11)[2], np.zeros((6, 11), np.float32)])
    assert int(capi.lib().asv_kernel_launch_count(capi.KERNEL_FRONT_CONV)) == before
