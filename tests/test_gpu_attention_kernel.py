"""The self-attention op alone on the MI355X, per element type, against float64 (cases: tests/attention_cases.py).

Bound.  Exponentials round, so there is no exact bound.  The yardstick is the same computation in float32 torch on CPU (with the
probabilities and the stored output rounded to the element type in the 16-bit modes), measured against float64 on the ragged batch
of lengths 1, 2, 63, 64, 65, 130 (block_err: the mean block and the std block of the pooled rows, each relative to its largest
value, worst utterance).  The device is allowed 4 x that error.  Measured on CPU (tests/test_transformer_host.py re-measures):

    heads d_k    f32        bf16       f16
      1    16   6.78e-08   3.21e-03   6.10e-04
      1    64   8.59e-08   7.07e-03   7.17e-04
      1   128   1.42e-07   5.40e-03   3.79e-04
      4    16   6.65e-08   2.37e-03   2.81e-04
      4    64   1.02e-07   4.21e-03   3.28e-04
      4   128   9.69e-08   3.66e-03   4.53e-04
      4    64   1.03e-07   6.02e-04   7.10e-05      the 130-row utterance alone, in two chunks of 65 rows

(the 16-bit figures are the rounding of the stored attention output: up to 2^-9 / 2^-12 of a value, which the one- and two-row
utterances of the batch do not average down).  The device's own errors against float64, measured on an MI355X when the kernel was
written (the test prints them): f32 7.4e-08 / 2.4e-07 / 1.8e-07 / 7.4e-08 / 2.0e-07 / 2.2e-07 and 3.0e-07 chunked - the bounds are
2.7e-07 .. 5.7e-07 and 4.1e-07; bf16 1.5e-03 .. 3.5e-03 (chunked 7.6e-04); f16 1.7e-04 .. 5.3e-04 (chunked 8.4e-05).
"""

import numpy as np
import pytest

import attention_cases as AC

pytestmark = pytest.mark.gpu

YARDSTICK = {                       # measured on CPU, see the module docstring; test_transformer_host.py holds them to the measurement
    (1, 16): dict(f32=6.78e-08, bf16=3.21e-03, f16=6.10e-04), (1, 64): dict(f32=8.59e-08, bf16=7.07e-03, f16=7.17e-04),
    (1, 128): dict(f32=1.42e-07, bf16=5.40e-03, f16=3.79e-04), (4, 16): dict(f32=6.65e-08, bf16=2.37e-03, f16=2.81e-04),
    (4, 64): dict(f32=1.02e-07, bf16=4.21e-03, f16=3.28e-04), (4, 128): dict(f32=9.69e-08, bf16=3.66e-03, f16=4.53e-04),
    "chunked": dict(f32=1.03e-07, bf16=6.02e-04, f16=7.10e-05),
}


def _engine(heads, d_k, et):
    from libs.amd import engine
    return engine.Engine(AC.build(heads, d_k), device_index=0, precision=et)


def _launches():
    from libs.amd import capi
    return int(capi.lib().asv_kernel_launch_count(capi.KERNEL_ATTENTION))


@pytest.mark.parametrize("et", AC.ELEM_TYPES)
@pytest.mark.parametrize("d_k", AC.D_KS)
@pytest.mark.parametrize("heads", AC.HEADS)
def test_attention_vs_float64(heads, d_k, et):
    """the ragged batch within 4 x the float32 yardstick's error; one launch of the kernel per op and extraction"""
    mats = AC.features()
    ref = np.stack([AC.reference64(m, heads, d_k) for m in mats])
    eng = _engine(heads, d_k, et)
    before = _launches()
    got = eng.extract_batch(mats).numpy()
    assert _launches() - before == 1
    err, bound = AC.block_err(got, ref), 4.0 * YARDSTICK[(heads, d_k)][et]
    print("[attention] heads %d d_k %3d %-4s device err %.3g  bound 4 x %.3g = %.3g" % (heads, d_k, et, err, YARDSTICK[(heads, d_k)][et], bound))
    assert np.isfinite(got).all()
    assert err <= bound, (heads, d_k, et, err, bound)


@pytest.mark.parametrize("et", AC.ELEM_TYPES)
def test_chunked_utterance(et):
    """a 130-row utterance split by max_chunk into two 65-row chunks: softmax inside a chunk only, the pooled rows averaged by length"""
    heads, d_k = 4, 64
    m = AC.features()[5]
    ref = AC.reference64(m, heads, d_k, max_chunk=65)
    assert AC.block_err(ref, AC.reference64(m, heads, d_k)) > 1e-3             # the chunked result is another one
    eng = _engine(heads, d_k, et)
    before = _launches()
    got = eng.extract_batch([m], max_chunk=65).numpy()
    assert _launches() - before == 1
    err, bound = AC.block_err(got, ref), 4.0 * YARDSTICK["chunked"][et]
    print("[attention] chunked %-4s device err %.3g  bound %.3g" % (et, err, bound))
    assert err <= bound, (et, err, bound)


@pytest.mark.parametrize("et", AC.ELEM_TYPES)
@pytest.mark.parametrize("heads,d_k", [(1, 16), (4, 64), (2, 128)])
def test_neighbour_independence(heads, d_k, et):
    """every utterance alone has the bits it has in the batch - also when the OTHER utterances are scaled by 1e4 (scores beyond
    the half range in f16: whatever they become stays in their own rows)"""
    mats = AC.features()
    eng = _engine(heads, d_k, et)
    full = eng.extract_batch(mats).numpy()
    assert np.isfinite(full).all()
    for i, m in enumerate(mats):
        alone = eng.extract_batch([m]).numpy()[0]
        assert np.array_equal(alone, full[i]), (heads, d_k, et, i)
        loud = [x if j == i else x * np.float32(1e4) for j, x in enumerate(mats)]
        assert np.array_equal(eng.extract_batch(loud).numpy()[i], full[i]), (heads, d_k, et, i, "neighbours x 1e4")
