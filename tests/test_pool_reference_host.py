"""The reference side of tests/test_gpu_pool_kernels.py, on the host: for every case the GPU file runs, the float32 numpy
reference stays within a quarter of the tolerance the kernel is held to (so a tolerance cannot hide a kernel error behind the
reference's own), the one-op multi-query programs fuse into one op that asks for the same numbers, and the reference is NaN
where the kernels promise NaN."""

import numpy as np
import pytest

import ir_interp
import pool_cases as PC


def _quarter(cases, et):
    worst = {}
    for case in cases:
        graph, feats = PC.build(case, et)
        chunk = PC.COMBINE_CHUNK if case.family == "combine" else None
        ref32 = PC.reference(graph, feats, np.float32, chunk)
        errs = PC.errors(case, ref32, PC.reference64(case, et))
        for block, (err, tol) in errs.items():
            worst[block] = max(worst.get(block, 0.0), err)
            assert err <= tol / 4, (case.name, et, block, err, tol)
    return worst


@pytest.mark.parametrize("et", PC.ELEM_TYPES)
@pytest.mark.parametrize("family", ["stats", "grid", "att", "mq", "lde", "combine"])
def test_float32_reference_stays_within_a_quarter_of_the_tolerance(family, et):
    cases = [c for c in PC.all_cases() if c.family == family]
    assert cases
    worst = _quarter(cases, et)
    print("[pool-host] %s %s: %d cases, float32 reference vs float64: %s" % (family, et, len(cases), " ".join("%s %.2e" % kv for kv in sorted(worst.items()))))


def test_every_gpu_case_is_listed_once():
    cases = PC.all_cases()
    assert len({c.key for c in cases}) == len(cases)


def test_inputs_are_representable_and_views_are_fenced():
    """Rounded inputs survive another rounding unchanged; everything outside the views is the filler."""
    for et in PC.ELEM_TYPES:
        for case in (PC.att_cases(48, 16)[0], PC.stats_cases(24, 16)[1], PC.mq_cases()[3], PC.lde_cases(16)[1]):
            graph, feats = PC.build(case, et)
            m = np.concatenate(feats)
            assert np.array_equal(PC.round_to(m, et), m) and np.isfinite(m).all()
            used = np.zeros(graph.feat_dim, dtype=bool)
            for op in graph.ops:
                for v in op.inputs():
                    assert v.tid == 0
                    used[v.ch_off:v.ch_off + v.channels] = True
            fill = PC.round_to(np.float32(PC.FILL).reshape(1), et)[0]
            assert np.all(m[:, ~used] == fill)
            assert graph.feat_dim == -(-(np.flatnonzero(used).max() + 1) // 16) * 16 + 16      # 16 filler columns behind the last padded view


def test_logit_spread_is_at_most_32():
    for et in PC.ELEM_TYPES:
        for case in PC.att_cases(200, 16) + PC.att_pattern_cases() + PC.mq_cases()[:4]:
            graph, feats = PC.build(case, et)
            for op in graph.ops:
                for m in feats:
                    e = m[:, op.logits.ch_off:op.logits.ch_off + op.logits.channels].astype(np.float64)
                    if op.softplus2:
                        e = 2.0 * np.log(np.log1p(np.exp(e)))
                    if op.prior_logit is not None:
                        e = np.concatenate([e, op.prior_logit[None, :]])
                    assert (e.max(axis=0) - e.min(axis=0)).max() <= 32.0, case.name


def test_adversarial_patterns_move_the_running_maximum_where_they_say():
    """Along the rows one lane of the 16-bit kernel visits (every 32nd), 'inc' logits rise strictly, 'dec' fall strictly; 'last'
    has its maximum in the last row, by more than 20."""
    for et in PC.ELEM_TYPES:
        for case in PC.att_pattern_cases():
            graph, feats = PC.build(case, et)
            lo, n = graph.ops[0].logits.ch_off, graph.ops[0].logits.channels
            for m in feats:
                e = m[:, lo:lo + n]
                if case.p["pattern"] == "last":
                    assert e.shape[0] == 1 or (e[-1] - e[:-1].max(axis=0)).min() > 20
                    continue
                for start in range(min(32, e.shape[0])):
                    d = np.diff(e[start::32], axis=0)
                    assert (d > 0).all() if case.p["pattern"] == "inc" else (d < 0).all()


def test_prior_is_the_maximum_in_one_utterance_and_far_below_in_another():
    case = [c for c in PC.att_cases(48, 0) if c.p["form"] == "sp2prior"][0]
    for et in PC.ELEM_TYPES:
        graph, feats = PC.build(case, et)
        op = graph.ops[0]
        logit = lambda m: 2.0 * np.log(np.log1p(np.exp(m[:, op.logits.ch_off:op.logits.ch_off + 48].astype(np.float64))))
        even, odd = np.arange(48) % 2 == 0, np.arange(48) % 2 == 1
        assert (logit(feats[3])[:, even].max(axis=0) < op.prior_logit[even]).all()
        assert (logit(feats[9])[:, odd].min(axis=0) - op.prior_logit[odd]).min() > 20


@pytest.mark.parametrize("case", PC.mq_cases(), ids=lambda c: c.name)
def test_fusion_matches_the_separate_ops(case):
    graph, feats = PC.build(case, "bf16")
    H, Q = case.p["heads"], case.p["queries"]
    assert [op.kind for op in graph.ops] == ["attpool"] * (H * Q)
    fused = graph.fused_mqpool_ops()
    assert [op.kind for op in fused] == ["mqattpool"]
    mq = fused[0]
    assert (mq.heads, mq.queries, mq.shared) == (H, Q, case.p["shared"]) and mq.x.channels == H * case.p["head_ch"]
    assert mq.out == graph.output
    for m in feats[:9]:
        separate = ir_interp.run_graph(graph, m)
        assert np.array_equal(ir_interp.run_graph(graph, m, ops=PC.expand_mqattpool(mq)), separate)
        assert separate.shape == (H * Q * 2 * case.p["head_ch"],)


def test_reference_is_nan_for_unbiased_2_at_length_1():
    """torch.var's default at one frame (the kernel comment of stats_pool_kernel promises the same): NaN in the std half of the
    one-frame utterance in both variance modes, nowhere else."""
    for var_mode in (0, 1):
        case = [c for c in PC.stats_cases(48, 16) if c.p["stddev"] and c.p["unbiased"] == 2 and c.p["var_mode"] == var_mode][0]
        for dtype in (np.float32, np.float64):
            graph, feats = PC.build(case, "f32")
            ref = PC.reference(graph, feats, dtype)
            want = np.zeros(ref.shape, dtype=bool)
            want[[i for i, m in enumerate(feats) if m.shape[0] == 1], 48:] = True
            assert want.any() and np.array_equal(np.isnan(ref), want)
    for unbiased in (0, 1):
        case = [c for c in PC.stats_cases(48, 16) if c.p["stddev"] and c.p["unbiased"] == unbiased][0]
        assert np.isfinite(PC.reference64(case, "f32")).all()
