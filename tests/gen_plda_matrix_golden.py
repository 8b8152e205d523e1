#!/usr/bin/env python3
"""Generate tests/golden/plda_matrix.npz by running the REFERENCE's own code: PldaEstimation, transform_ivector and
log_likelihood_ratio of score/pyplda/plda_base.py, CalculateVar / PLDAScoring of score/pyplda/gaussian-plda-scoring.py and
score/ScoreNormalization.py.  Build container only (needs the reference tree, like oracle/gen_golden.py, whose shims this file uses,
as tests/gen_plda_adapt_golden.py does).

What it records: a dim-24 model; 23 enrolment speaker means (1..5 utterances), 31 test and 41 cohort vectors.  The vectors
transformed by transform_ivector and psi are ROUNDED TO f32 and installed in the reference model as float64, so that the device is
handed the very inputs the reference scored.  LLR matrices enrol x test, enrol x cohort and test x cohort (the test vectors in the
enrolment role with one utterance each, the cohort always on the test side) by looping log_likelihood_ratio over all pairs in
float64; the two-covariance matrix enrol x test from PLDAScoring on the f32-rounded raw vectors; 300 distinct trials; and the
outputs of ScoreNormalization.py (snorm; asnorm top 10; asnorm top 10 --cross-select true) on text files of those LLRs rounded to
f32 and written with repr, as oracle/gen_golden.py run_score_norm does.

`spread_<tag>`: the script run a second time on the same LLRs, each moved by one f32 ulp up or down (seeded), max |difference| of
the outputs - a property of the reference alone, from which the tests derive their tolerance.  The generator asserts that every
row's top-10 cohort set is the same in both runs (a boundary gap of one ulp would make that comparison meaningless); SEED below is
the first seed for which it held.

    PYTHONDONTWRITEBYTECODE=1 python tests/gen_plda_matrix_golden.py
"""

import importlib.util
import os
import sys
import tempfile
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
os.environ.setdefault("PYTHONPYCACHEPREFIX", os.path.join(tempfile.gettempdir(), "gen_plda_matrix_pycache"))
sys.dont_write_bytecode = True
sys.pycache_prefix = os.environ["PYTHONPYCACHEPREFIX"]

import numpy as np  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from oracle import gen_golden as G  # noqa: E402
import plda_matrix_cases as PM  # noqa: E402

NAME = "plda_matrix"
DIM, SEED, EM_ITERS, TOP_N = 24, 91, 10, 10             # SEED 91: the first one tried; the top-10 assertion held
N_ENROLL, N_TEST, N_COHORT, N_TRIALS = 23, 31, 41, 300
TAGS = (("snorm", "snorm", 0, "false"), ("asnorm10", "asnorm", TOP_N, "false"), ("asnorm10x", "asnorm", TOP_N, "true"))


def load_script(path, modname):
    argv, sys.argv = sys.argv, ["x"]
    try:
        spec = importlib.util.spec_from_file_location(modname, path)
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    finally:
        sys.argv = argv
    return m


def all_pairs_llr(plda, enroll_t, num_utts, test_t):
    return np.array([[float(plda.log_likelihood_ratio(e, int(n), t)) for t in test_t] for e, n in zip(enroll_t, num_utts)])


def run_score_norm(sn, et, ec, tc, ei, ti):
    """ScoreNormalization.py on text files of f32 scores written with repr -> {tag: float64 [n_trials]}."""
    out = {}
    with tempfile.TemporaryDirectory() as td:
        def write(path, rows):
            with open(path, "w") as f:
                for a, b, v in rows:
                    f.write("%s %s %s\n" % (a, b, repr(float(np.float32(v)))))
        write(os.path.join(td, "et"), [("e%d" % a, "t%d" % b, v) for a, b, v in zip(ei, ti, et)])
        write(os.path.join(td, "ec"), [("e%d" % a, "c%d" % c, ec[a, c]) for a in range(ec.shape[0]) for c in range(ec.shape[1])])
        write(os.path.join(td, "tc"), [("t%d" % b, "c%d" % c, tc[b, c]) for b in range(tc.shape[0]) for c in range(tc.shape[1])])
        for tag, method, top_n, cross in TAGS:
            args = types.SimpleNamespace(method=method, top_n=top_n, second_cohort="true", cross_select=cross, input_score=os.path.join(td, "et"),
                                         enroll_cohort_score=os.path.join(td, "ec"), test_cohort_score=os.path.join(td, "tc"),
                                         output_score=os.path.join(td, "out_" + tag))
            (sn.snorm if method == "snorm" else sn.asnorm)(args)
            lines = [line.split() for line in open(args.output_score)]
            assert [tuple(l[:2]) for l in lines] == [("e%d" % a, "t%d" % b) for a, b in zip(ei, ti)], "the reference keeps the trial order"
            out[tag] = np.asarray([float(l[2]) for l in lines], dtype=np.float64)
    return out


def one_ulp(x, rng):
    x = np.asarray(x, dtype=np.float32)
    toward = np.where(rng.rand(*x.shape) < 0.5, np.float32(-np.inf), np.float32(np.inf)).astype(np.float32)
    return np.nextafter(x, toward)


def top_sets(m, k):
    return [frozenset(np.argsort(-row, kind="stable")[:k].tolist()) for row in m]


def main():
    if not os.path.isdir(G.REF):
        sys.exit("gen_plda_matrix_golden.py needs the reference tree at %s (build container only)" % G.REF)
    G.install_shims()
    sys.path.insert(0, os.path.join(G.REF, "pytorch"))
    import libs.support.kaldi_io as ref_kaldi_io
    sys.modules["kaldi_io"] = ref_kaldi_io
    pyplda = os.path.join(G.REF, "score", "pyplda")
    sys.path.insert(0, pyplda)
    import plda_base as PB
    PB.logger.setLevel("WARNING")
    twocov = load_script(os.path.join(pyplda, "gaussian-plda-scoring.py"), "ref_twocov")
    sn = load_script(os.path.join(G.REF, "score", "ScoreNormalization.py"), "ref_score_norm")
    synth = G.load_synth()

    # ---- model (as run_scoring_plda: planted speakers, the reference's EM)
    train, labels = synth.synth_speaker_embeddings(60, 8, DIM, seed=SEED, within=1.0, between=0.8)
    stats = PB.PldaStats(DIM)
    for spk in np.unique(labels):
        stats.add_samples(1.0, train[labels == spk].astype(np.float64))
    assert stats.is_sorted()
    est = PB.PldaEstimation(stats)
    est.estimate(num_em_iters=EM_ITERS)
    plda = est.get_output()
    plda.offset = np.asarray(plda.offset).reshape(-1)             # 1-D like the vectors (see oracle/gen_golden.py run_scoring_plda)

    # ---- vector sets: enrolment speaker means over 1..5 utterances (f32), test and cohort utterances
    rng = np.random.RandomState(SEED + 1)
    spk_utts, _ = synth.synth_speaker_embeddings(N_ENROLL, 5, DIM, seed=SEED + 2, within=1.0, between=0.8)
    spk_utts = spk_utts.reshape(N_ENROLL, 5, DIM)
    num_utts = rng.randint(1, 6, size=N_ENROLL).astype(np.int32)
    assert set(num_utts.tolist()) == {1, 2, 3, 4, 5}
    enroll = np.stack([spk_utts[i, :n].astype(np.float64).mean(0) for i, n in enumerate(num_utts)]).astype(np.float32)
    test, _ = synth.synth_speaker_embeddings(N_TEST, 1, DIM, seed=SEED + 3, within=1.0, between=0.8)
    cohort, _ = synth.synth_speaker_embeddings(N_COHORT, 1, DIM, seed=SEED + 4, within=1.0, between=0.8)

    def transformed(x, n):
        return np.stack([plda.transform_ivector(v, int(k)) for v, k in zip(x.astype(np.float64), n)]).astype(np.float32)
    ones_t, ones_c = np.ones(N_TEST, dtype=np.int32), np.ones(N_COHORT, dtype=np.int32)
    enroll_t, test_t, cohort_t = transformed(enroll, num_utts), transformed(test, ones_t), transformed(cohort, ones_c)
    psi32 = np.asarray(plda.psi, dtype=np.float64).reshape(-1).astype(np.float32)
    plda.psi = psi32.astype(np.float64)                            # the device's inputs, installed in the reference model
    e64, t64, c64 = enroll_t.astype(np.float64), test_t.astype(np.float64), cohort_t.astype(np.float64)
    llr_et = all_pairs_llr(plda, e64, num_utts, t64)
    llr_ec = all_pairs_llr(plda, e64, num_utts, c64)
    llr_tc = all_pairs_llr(plda, t64, ones_t, c64)

    # ---- two-covariance matrix on the f32-rounded raw vectors
    gamma, lam, c, k = twocov.CalculateVar(est.between_var, est.within_var + 5e-5 * np.eye(DIM), est.mean)
    two_cov = np.array([[float(twocov.PLDAScoring(a.reshape(-1, 1), b.reshape(-1, 1), gamma, lam, c, k)) for b in test.astype(np.float64)]
                        for a in enroll.astype(np.float64)])

    # ---- trials and score normalisation
    pairs = rng.permutation(N_ENROLL * N_TEST)[:N_TRIALS]
    ei, ti = (pairs // N_TEST).astype(np.int32), (pairs % N_TEST).astype(np.int32)
    assert len(set(zip(ei.tolist(), ti.tolist()))) == N_TRIALS
    et32, ec32, tc32 = llr_et[ei, ti].astype(np.float32), llr_ec.astype(np.float32), llr_tc.astype(np.float32)
    normed = run_score_norm(sn, et32, ec32, tc32, ei, ti)
    prng = np.random.RandomState(SEED + 5)
    et_p, ec_p, tc_p = one_ulp(et32, prng), one_ulp(ec32, prng), one_ulp(tc32, prng)
    assert (et_p != et32).all() and (ec_p != ec32).all() and (tc_p != tc32).all()
    assert top_sets(ec32, TOP_N) == top_sets(ec_p, TOP_N) and top_sets(tc32, TOP_N) == top_sets(tc_p, TOP_N), \
        "a top-%d boundary within one f32 ulp: change SEED" % TOP_N
    normed_p = run_score_norm(sn, et_p, ec_p, tc_p, ei, ti)

    out = dict(dim=np.int64(DIM), seed=np.int64(SEED), top_n=np.int64(TOP_N), psi=psi32, num_utts=num_utts,
               enroll_t=enroll_t, test_t=test_t, cohort_t=cohort_t, llr_enroll_test=llr_et, llr_enroll_cohort=llr_ec, llr_test_cohort=llr_tc,
               enroll_raw=enroll, test_raw=test, mean=np.asarray(est.mean).reshape(-1), within_var=np.array(est.within_var),
               between_var=np.array(est.between_var), two_cov=two_cov, trials_e=ei, trials_t=ti)
    for tag, _, _, _ in TAGS:
        out[tag] = normed[tag]
        out["spread_" + tag] = np.float64(np.abs(normed[tag] - normed_p[tag]).max())
        print("%-10s max |normed| %.4g   spread (one f32 ulp on every input) %.3g" % (tag, np.abs(normed[tag]).max(), out["spread_" + tag]))
    # the expansion the device computes, against the reference's own numbers (the host test repeats this)
    for tag, (a, n, b) in (("enroll_test", (enroll_t, num_utts, test_t)), ("enroll_cohort", (enroll_t, num_utts, cohort_t)), ("test_cohort", (test_t, None, cohort_t))):
        S, M = PM.llr_expansion(a, b, psi32, n)
        err = np.abs(S - out["llr_" + tag])
        print("llr_%-14s max |LLR| %.4g   expansion - reference: max %.3g = %.3g of the float64 bound" %
              (tag, np.abs(out["llr_" + tag]).max(), err.max(), (err / PM.llr_bound(0.0, M, DIM, 0)).max()))
    os.makedirs(G.GOLDEN, exist_ok=True)
    path = os.path.join(G.GOLDEN, NAME + ".npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
