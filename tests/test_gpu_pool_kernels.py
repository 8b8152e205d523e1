"""The pooling kernels of kernels_pool.hip alone, per element type, against float64.

A program of one op (tests/pool_cases.py) runs exactly one of stats_pool_kernel (plain and NARROW), sum_chunk_kernel + finish,
attentive_pool_kernel, mq_attentive_pool_kernel, the two lde kernels and combine_kernel on inputs that are already representable
in the mode's element type, so the float64 reference sees the kernel's numbers and nothing but the kernel is between them.
Ragged batches put every segment length next to the rows-per-step and rows-per-unrolled-trip of every variant (f32 statistics
16 / 64, 16-bit 32 / 128, NARROW 64 / 256, the 16-bit attentive two-frame trip 32 / 64).

Bounds: 1e-5 for the statistics kernels, 2e-5 for the attentive kernels (means; std squared, see pool_cases.std2_err) and LDE, for
f32, bf16 and f16 rows alike; tests/test_pool_reference_host.py holds the float32 numpy reference to a quarter of each.  Every
case prints its measured error ("[pool] case ...").
"""

import numpy as np
import pytest

import pool_cases as PC

pytestmark = pytest.mark.gpu


def _extract(case, et, feats=None, max_chunk=10000, prepare=None, check=None):
    """One Engine for the case's graph; the batch (or every batch of `feats`) extracted; status 0; closed.  `prepare(engine)` runs
    before the extraction, `check(engine)` behind it."""
    from libs.amd import engine
    graph, batch = PC.build(case, et)
    eng = engine.Engine(graph, precision=et)
    try:
        if prepare is not None:
            prepare(eng)
        outs = [eng.extract_batch(f, max_chunk=max_chunk).numpy() for f in ([batch] if feats is None else feats)]
        if check is not None:
            check(eng)
        assert eng.status() == 0
    finally:
        eng.close()
    return outs[0] if feats is None else outs


def _check(case, et, got):
    errs = PC.errors(case, got, PC.reference64(case, et))
    PC.report(case, et, errs)
    for block, (err, tol) in errs.items():
        assert err < tol, (case.name, et, block, err, tol)
    return errs


@pytest.mark.parametrize("et", PC.ELEM_TYPES)
@pytest.mark.parametrize("ch_off", [0, 16])
@pytest.mark.parametrize("channels", PC.STATS_CHANNELS)
def test_stats_pool_vs_float64(channels, ch_off, et):
    """stddev x unbiased x var_mode; unbiased = 2 is NaN at one frame exactly where the reference is (pool_cases._nan_rel_err)."""
    for case in PC.stats_cases(channels, ch_off):
        got = _extract(case, et)
        _check(case, et, got)
        if case.p["stddev"] and case.p["unbiased"] == 2:
            assert np.isnan(got[0, channels:]).all() and not np.isnan(got[1:]).any() and not np.isnan(got[0, :channels]).any()


@pytest.mark.parametrize("et", PC.ELEM_TYPES)
def test_stats_pool_eps_forms(et):
    """eps = 1e-2 with a constant channel: sqrt(max(var, eps)) and sqrt(var + eps) are both 0.1 there and differ everywhere else
    (by 1.6e-2 where the std is 0.3: the comparison with the reference decides which form the kernel took)."""
    clamp, add = (_extract(case, et) for case in PC.stats_eps_cases())
    for case, got in zip(PC.stats_eps_cases(), (clamp, add)):
        _check(case, et, got)
    assert np.allclose(clamp[:, 48 + 5], 0.1, rtol=1e-6) and np.allclose(add[:, 48 + 5], 0.1, rtol=1e-6)
    others = np.arange(48) != 5
    assert (add[1:, 48:][:, others] > clamp[1:, 48:][:, others]).all()


@pytest.mark.parametrize("et", PC.ELEM_TYPES)
def test_grid_means_chunked_and_per_bin(et):
    """sum_chunk_kernel + finish on 2016, 2048, 2080, 4128 and 96 rows (one chunk is 2048 rows), and the groups / row_stride path
    of stats_pool_kernel for the per-bin statistics of the same map.  The pool op runs as its own launch."""
    def ran_alone(eng):
        assert [op.kind for op in eng.ops] == ["grid_input", "pool"] and "stats_pool" in eng.describe()
        eng.set_profiling(2)

    def own_launch(eng):
        rows = [r for r in eng.get_profile() if r["name"] == "stats_pool"]
        eng.set_profiling(0)
        assert len(rows) == 1 and rows[0]["op_index"] == 1 and rows[0]["launches"] >= 1, rows

    for case in PC.grid_cases():
        _check(case, et, _extract(case, et, prepare=ran_alone, check=own_launch))


@pytest.mark.parametrize("et", PC.ELEM_TYPES)
@pytest.mark.parametrize("ch_off", [0, 16])
@pytest.mark.parametrize("channels", PC.ATT_CHANNELS)
def test_attentive_pool_vs_float64(channels, ch_off, et):
    """per-channel, shared, grouped (16; 50 with 200 channels) logits, softplus2 without and with the prior frame."""
    for case in PC.att_cases(channels, ch_off):
        _check(case, et, _extract(case, et))


@pytest.mark.parametrize("et", PC.ELEM_TYPES)
@pytest.mark.parametrize("case", PC.att_pattern_cases(), ids=lambda c: "%s-%s" % (c.p["form"], c.p["pattern"]))
def test_attentive_pool_adversarial_logits(case, et):
    """Rising logits (every trip of the one-pass path rescales), falling logits (never after the first frame), one dominant
    frame in the last row.  In the 16-bit kernel a lane takes rows r and r + 32 per two-frame trip: the last row of the 33-frame
    utterance is the second frame of lane 0's only trip, the last rows of the 65-, 129- and 257-frame utterances are taken by a
    single lane in the tail loop, behind its trips."""
    _check(case, et, _extract(case, et))


@pytest.mark.parametrize("et", PC.ELEM_TYPES)
@pytest.mark.parametrize("case", PC.mq_cases(), ids=lambda c: "hc%d-q%d-%s" % (c.p["head_ch"], c.p["queries"], "shared" if c.p["shared"] else "chan"))
def test_mq_attentive_pool_vs_float64(case, et):
    """The one-launch kernel against float64 (not against the separate launches, whose accumulation statements it shares)."""
    from libs.amd import capi
    L = capi.lib()

    def fused(eng):
        assert [op.kind for op in eng.ops] == ["mqattpool"]

    before = L.asv_kernel_launch_count(capi.KERNEL_MQ_ATTPOOL)
    got = _extract(case, et, check=fused)
    assert L.asv_kernel_launch_count(capi.KERNEL_MQ_ATTPOOL) == before + 1
    _check(case, et, got)


@pytest.mark.parametrize("et", PC.ELEM_TYPES)
@pytest.mark.parametrize("channels", PC.LDE_CHANNELS)
def test_lde_pool_vs_float64(channels, et):
    """1 .. 64 centres, both sides of every KMAX of lde_accumulate_kernel; the last centre's weight underflows to 0."""
    for case in PC.lde_cases(channels):
        _check(case, et, _extract(case, et))


@pytest.mark.parametrize("et", PC.ELEM_TYPES)
def test_chunk_combine_vs_float64(et):
    """257, 100, 101 and 1 frames in chunks of 100: combine_kernel's frame-weighted mean of the chunk statistics."""
    case = PC.combine_cases()[0]
    _check(case, et, _extract(case, et, max_chunk=PC.COMBINE_CHUNK))


@pytest.mark.parametrize("et", PC.ELEM_TYPES)
@pytest.mark.parametrize("case", PC.independence_cases(), ids=lambda c: "%s-%s" % (c.family, "-".join(str(v) for _, v in sorted(c.p.items()))))
def test_neighbours_do_not_change_the_bits(case, et):
    """Utterances 0, 5 and the last (the grid batch has five: 0, 2 and the last), extracted alone, give the bits they have in
    the ragged batch."""
    _, batch = PC.build(case, et)
    picks = sorted({0, 5 if len(batch) > 5 else 2, len(batch) - 1})
    outs = _extract(case, et, feats=[batch] + [[batch[i]] for i in picks])
    whole = outs[0]
    assert not np.isnan(whole).any()
    for i, alone in zip(picks, outs[1:]):
        assert alone.shape == (1, whole.shape[1]) and np.array_equal(alone[0], whole[i]), (case.name, et, i)
