"""All-pairs PLDA score matrices on the MI355X (asv_plda_llr_matrix, asv_two_cov_matrix: csrc/kernels_score_matrix.hip) and PLDA
score normalisation (scoring.plda_asnorm_trials) against float64 numpy restatements, the per-trial entry points and the
reference-generated fixture tests/golden/plda_matrix.npz (tests/gen_plda_matrix_golden.py).

Bounds (tests/plda_matrix_cases.py): per element 2^-24 |want| for the one f32 rounding of the output + 4 (2 dim + 16) 2^-52 M with
M = sum_k |a_k b_k| + |row_i| - the float64 summation bound of the K = 2 dim product in either order, times 4 for the roundings of
the preparation.  All data is non-symmetric: the f32 C/D row map on the f64 matrix instruction would put 3 of 4 results in the
wrong row and a symmetric matrix would hide part of that."""

import functools

import numpy as np
import pytest

import helpers
import plda_matrix_cases as PM

pytestmark = pytest.mark.gpu


def _report(what, err, bound):
    print("%s: max |err| %.3g, max err / bound %.3g" % (what, err.max(), (err / bound).max()))


@functools.lru_cache(maxsize=None)
def _llr_case(shape, mixed_n):
    """inputs, the reference-order float64 matrix and M of one shape - computed once, read-only afterwards"""
    E, T, dim = shape
    enroll, test, psi, n = PM.make_llr_case(E, T, dim, seed=1000 + E + 7 * T + 13 * dim, mixed_n=mixed_n)
    want = PM.llr_reference_order(enroll, test, psi, n)
    _, M = PM.llr_expansion(enroll, test, psi, n)
    for a in (want, M):
        a.setflags(write=False)
    return enroll, test, psi, n, want, M


def _plda(psi):
    from libs.amd import scoring
    dim = psi.shape[0]
    return scoring.Plda(np.zeros(dim), np.eye(dim), psi.astype(np.float64))


@pytest.mark.parametrize("mixed_n", [False, True], ids=["n1", "n137"])
@pytest.mark.parametrize("shape", PM.LLR_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_llr_matrix_vs_float64_restatement_and_trials(shape, mixed_n):
    enroll, test, psi, n, want, M = _llr_case(shape, mixed_n)
    E, T, dim = shape
    plda = _plda(psi)
    got = plda.llr_matrix(enroll, test, n)
    assert got.shape == (E, T) and str(got.dtype) == "torch.float32" and got.is_cuda
    got = got.cpu().numpy().astype(np.float64)
    err, bound = np.abs(got - want), PM.llr_bound(want, M, dim, 1)
    _report("llr_matrix %s vs float64" % (shape,), err, bound)
    assert (err <= bound).all(), (shape, mixed_n, float((err / bound).max()))
    # the same numbers from the per-trial entry point over the full E x T list (its own f32 rounding: 2^-23 |want| together)
    ei, ti = (a.reshape(-1).astype(np.int32) for a in np.meshgrid(np.arange(E), np.arange(T), indexing="ij"))
    trials = plda.llr_trials(enroll, test, ei, ti, n).cpu().numpy().astype(np.float64).reshape(E, T)
    err2, bound2 = np.abs(got - trials), PM.llr_bound(want, M, dim, 2)
    _report("llr_matrix %s vs llr_trials" % (shape,), err2, bound2)
    assert (err2 <= bound2).all(), (shape, mixed_n, float((err2 / bound2).max()))


@pytest.mark.parametrize("shape", PM.TWO_COV_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_two_cov_matrix_vs_float64_and_trials(shape):
    from libs.amd import scoring
    E, T, dim = shape
    enroll, test, mean, within, between = PM.make_two_cov_case(E, T, dim, seed=2000 + E + 7 * T + 13 * dim)
    model = scoring.TwoCovPlda(mean, within, between)
    want, M = PM.two_cov_matrix(enroll, test, model.gamma, model.lam, model.c)
    bound = PM.two_cov_bound(M, dim)
    got = model.score_matrix(enroll, test)
    assert got.shape == (E, T) and str(got.dtype) == "torch.float64" and got.is_cuda
    got = got.cpu().numpy()
    err = np.abs(got - want)
    _report("two_cov matrix %s vs float64" % (shape,), err, bound)
    assert (err <= bound).all(), (shape, float((err / bound).max()))
    ei, ti = (a.reshape(-1).astype(np.int32) for a in np.meshgrid(np.arange(E), np.arange(T), indexing="ij"))
    trials = model.score_trials(enroll, test, ei, ti).cpu().numpy().reshape(E, T)
    err2 = np.abs(got - trials)
    _report("two_cov matrix %s vs score_trials" % (shape,), err2, bound)
    assert (err2 <= bound).all(), (shape, float((err2 / bound).max()))


def test_matrices_vs_reference_fixture():
    from libs.amd import scoring
    g = np.load(helpers.GOLDEN + "/plda_matrix.npz")
    dim, psi, n = int(g["dim"]), g["psi"], g["num_utts"]
    plda = _plda(psi)
    for tag, a, na, b in (("enroll_test", g["enroll_t"], n, g["test_t"]), ("enroll_cohort", g["enroll_t"], n, g["cohort_t"]),
                          ("test_cohort", g["test_t"], None, g["cohort_t"])):
        want = g["llr_" + tag]
        _, M = PM.llr_expansion(a, b, psi, na)
        got = plda.llr_matrix(a, b, na).cpu().numpy().astype(np.float64)
        err, bound = np.abs(got - want), PM.llr_bound(want, M, dim, 1)
        _report("fixture llr_" + tag, err, bound)
        assert (err <= bound).all(), (tag, float((err / bound).max()))
    model = scoring.TwoCovPlda(g["mean"], g["within_var"], g["between_var"])
    _, M = PM.two_cov_matrix(g["enroll_raw"], g["test_raw"], model.gamma, model.lam, model.c)
    err, bound = np.abs(model.score_matrix(g["enroll_raw"], g["test_raw"]).cpu().numpy() - g["two_cov"]), PM.two_cov_bound(M, dim)
    _report("fixture two_cov", err, bound)
    assert (err <= bound).all(), float((err / bound).max())


def test_plda_asnorm_trials_is_the_composition_and_matches_the_reference():
    """plda_asnorm_trials == llr_trials + 2 x llr_matrix + score_normalize by hand, bit for bit; and within 4 spread_<tag> (what one
    f32 ulp on every input does to the reference's own output) + 2e-6 max(1, max |want|) (the tolerance of
    test_score_norm_vs_reference_fixture_and_oracle for identical inputs) of the reference's ScoreNormalization.py.  The fixture's
    vectors are already transformed: the model handed over has the identity transform and no length normalisation."""
    import torch
    from libs.amd import scoring
    g = np.load(helpers.GOLDEN + "/plda_matrix.npz")
    psi, n, ei, ti = g["psi"], g["num_utts"], g["trials_e"], g["trials_t"]
    plda = _plda(psi)
    for tag, top_n, cross in (("snorm", 0, False), ("asnorm10", int(g["top_n"]), False), ("asnorm10x", int(g["top_n"]), True)):
        got = scoring.plda_asnorm_trials(plda, g["enroll_t"], g["test_t"], g["cohort_t"], ei, ti, enroll_num_utts=n, top_n=top_n, cross_select=cross,
                                         normalize_length=False)
        e, t, c = (plda.transform_vectors(x, k, normalize_length=False) for x, k in ((g["enroll_t"], n), (g["test_t"], None), (g["cohort_t"], None)))
        hand = scoring.score_normalize(plda.llr_trials(e, t, ei, ti, n), plda.llr_matrix(e, c, n), plda.llr_matrix(t, c), ei, ti, top_n=top_n, cross_select=cross)
        assert torch.equal(got, hand), tag
        want = g[tag]
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        tol = 4.0 * float(g["spread_" + tag]) + 2e-6 * max(1.0, np.abs(want).max())
        print("plda_asnorm_trials %s: max |err| %.3g, tolerance %.3g" % (tag, err.max(), tol))
        assert err.max() <= tol, (tag, float(err.max()), tol)


@pytest.mark.parametrize("kw", [{}, {"simple_length_norm": True}, {"normalize_length": False}], ids=["defaults", "simple_norm", "no_norm"])
def test_plda_asnorm_trials_passes_its_transform_options_on(kw):
    """A trained model on raw vectors, the default transform (PLDA length normalisation) and the two other settings: bit-identical to
    the hand composition with the same settings, and the three settings give different scores (a dropped keyword cannot hide)."""
    import torch
    from libs.amd import scoring
    g = np.load(helpers.GOLDEN + "/plda_matrix.npz")
    plda = scoring.Plda.from_covariances(g["mean"], g["within_var"], g["between_var"])
    enroll, n, ei, ti = g["enroll_raw"], g["num_utts"], g["trials_e"], g["trials_t"]
    test, cohort = g["test_raw"], (g["test_raw"][::-1] * np.float32(0.9) + np.float32(0.05) * g["enroll_raw"][(np.arange(31) * 5) % 23]).astype(np.float32)
    got = scoring.plda_asnorm_trials(plda, enroll, test, cohort, ei, ti, enroll_num_utts=n, top_n=10, **kw)
    full = dict(normalize_length=True, simple_length_norm=False)
    full.update(kw)
    e, t, c = plda.transform_vectors(enroll, n, **full), plda.transform_vectors(test, None, **full), plda.transform_vectors(cohort, None, **full)
    hand = scoring.score_normalize(plda.llr_trials(e, t, ei, ti, n), plda.llr_matrix(e, c, n), plda.llr_matrix(t, c), ei, ti, top_n=10, cross_select=False)
    assert torch.equal(got, hand) and bool(torch.isfinite(got).all())
    others = [o for o in ({}, {"simple_length_norm": True}, {"normalize_length": False}) if o != kw]
    for o in others:
        assert not torch.equal(got, scoring.plda_asnorm_trials(plda, enroll, test, cohort, ei, ti, enroll_num_utts=n, top_n=10, **o)), (kw, o)


def test_two_streams_two_sizes_without_synchronisation():
    """asv_plda_llr_matrix is asynchronous and its operand scratch is stream-ordered: calls of different sizes on two streams, nothing
    in between, all come out right (the pattern of test_trial_indices_are_validated_and_scratch_is_per_stream)."""
    import torch
    cases = [_llr_case((130, 257, 150), True), _llr_case((65, 63, 24), False)]
    dev = [[torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None for a in c[:4]] for c in cases]
    pldas = [_plda(c[2]) for c in cases]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for k in range(6):
        which = k % 2
        with torch.cuda.stream(streams[which]):
            e, t, _, n = dev[which]
            outs.append(pldas[which].llr_matrix(e, t, n))
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        _, _, _, _, want, M = cases[k % 2]
        dim = cases[k % 2][2].shape[0]
        err = np.abs(o.cpu().numpy().astype(np.float64) - want)
        assert (err <= PM.llr_bound(want, M, dim, 1)).all(), k


def test_validation_raises_before_anything_is_launched():
    """Every ValueError below is raised by the wrapper before it reaches the library: nothing is launched."""
    from libs.amd import capi, scoring
    enroll, test, psi, n, _, _ = _llr_case((17, 5, 3), True)
    plda = _plda(psi)
    with pytest.raises(ValueError, match="3-dimensional model"):
        plda.llr_matrix(enroll, np.zeros((5, 4), dtype=np.float32))
    with pytest.raises(ValueError, match="3-dimensional model"):
        plda.llr_matrix(np.zeros((17, 2), dtype=np.float32), test)
    with pytest.raises(ValueError, match="17 enrolment vectors but"):
        plda.llr_matrix(enroll, test, n[:-1])
    with pytest.raises(ValueError, match="empty set"):
        plda.llr_matrix(np.zeros((0, 3), dtype=np.float32), test)
    with pytest.raises(ValueError, match="empty set"):
        plda.llr_matrix(enroll, np.zeros((0, 3), dtype=np.float32))
    enroll2, test2, mean, within, between = PM.make_two_cov_case(17, 5, 3, seed=5)
    model = scoring.TwoCovPlda(mean, within, between)
    with pytest.raises(ValueError, match="3-dimensional model"):
        model.score_matrix(enroll2, np.zeros((5, 4), dtype=np.float32))
    with pytest.raises(ValueError, match="empty set"):
        model.score_matrix(np.zeros((0, 3), dtype=np.float32), test2)
    # the C ABI itself refuses what the wrapper would have let through, with a message
    import ctypes as C
    import torch
    e = torch.from_numpy(enroll).cuda()
    out = torch.empty((17, 5), dtype=torch.float32, device="cuda")
    null = C.c_void_p(0)
    ptr = lambda x: C.c_void_p(x.data_ptr())
    p = torch.from_numpy(psi).cuda()
    tt = torch.from_numpy(test).cuda()
    lib = capi.lib()
    for args in ((ptr(e), 0, ptr(tt), 5, 3, ptr(p), null, ptr(out), null), (ptr(e), 17, ptr(tt), 5, 4097, ptr(p), null, ptr(out), null),
                 (ptr(e), 17, null, 5, 3, ptr(p), null, ptr(out), null)):
        assert lib.asv_plda_llr_matrix(*args) < 0 and b"asv_plda_llr_matrix" in lib.asv_last_error()
