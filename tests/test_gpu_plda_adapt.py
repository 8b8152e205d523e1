"""PLDA domain adaptors with the adaptation-set statistics from the MI355X (asv_scatter_f64), the in-domain PLDA from the device
EM (asv_plda_train) and the scores from the device scoring kernels, against the reference's own outputs
(tests/golden/plda_domain_adapt.npz).  tests/test_plda_adapt_host.py holds the host half and explains the tolerance rule, which
is the same here: the device statistics are float64 sums of the float32 inputs, in another order than the reference's
vector-by-vector loop."""

import numpy as np
import pytest

from plda_adapt_common import ADAPTORS, check_against_fixture, check_llr, llr_f64, load_fixture, models, read_kaldi_text_plda, run_adaptor, run_script

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return load_fixture()


@pytest.mark.parametrize("name", ADAPTORS)
def test_adaptor_with_device_statistics_matches_the_reference(g, name):
    out_model, in_model = models(g)
    check_against_fixture(g, name, run_adaptor(name, out_model, in_model, g["adapt"]))


def coral_numpy(mean_o, W, B, x):
    """CORAL in float64 numpy, from the definition: A = variance^1/2 (W + B)^-1/2."""
    x = x.astype(np.float64)
    mean = x.mean(0)
    d = mean - mean_o
    variance = x.T.dot(x) / len(x) - np.outer(mean, mean) + np.outer(d, d)
    so, qo = np.linalg.eigh(W + B)
    si, qi = np.linalg.eigh(0.5 * (variance + variance.T))
    A = (qi * np.sqrt(si)).dot(qi.T).dot((qo / np.sqrt(so)).dot(qo.T))
    return mean, A.dot(W).dot(A.T), A.dot(B).dot(A.T), si


@pytest.mark.parametrize("n,dim", [(25, 24), (257, 24), (400, 24), (131, 40)])
def test_coral_at_the_edges_of_the_statistics_kernel(g, n, dim):
    """Set sizes around the 16-row K step and the 64-wide tiles of the float64 GEMM behind asv_scatter_f64 (25: two K steps, the
    second nearly empty, and barely more vectors than dimensions; 257 = 16 * 16 + 1; dim 40: no multiple of 16 or 32).

    Tolerance: both sides sum n float64 products per entry, in different orders - at most n * eps relative on the statistics,
    each; the matrix square root of the adaptation variance amplifies a perturbation by at most sqrt(cond) / 2 (cond is taken
    from the numpy side), and A enters W and B twice: 8 * n * eps * (1 + sqrt(cond) / 2), floored at the 1e-12 of the other
    tests."""
    from libs.amd import scoring
    if dim == 24:
        out_model, _ = models(g)
        x = g["adapt"][:n]
    else:
        r = np.random.RandomState(5)
        w, b = r.standard_normal((dim, 3 * dim)), r.standard_normal((dim, 3 * dim))
        out_model = scoring.PldaCovariances(r.standard_normal(dim), w.dot(w.T) / (3 * dim), 0.5 * b.dot(b.T) / (3 * dim))
        x = (r.standard_normal((n, dim)) * np.linspace(0.5, 2.0, dim) + 2.0 * r.standard_normal(dim)).astype(np.float32)
    total, xtx = scoring.second_moments(x)
    x64 = x.astype(np.float64)
    assert np.abs(total - x64.sum(0)).max() <= 2 * n * np.finfo(np.float64).eps * np.abs(x64).sum(0).max()
    assert np.abs(xtx - x64.T.dot(x64)).max() <= 2 * n * np.finfo(np.float64).eps * np.abs(xtx).max()
    mean, S_w, S_b, spectrum = coral_numpy(out_model.mean, out_model.within_var, out_model.between_var, x)
    tol = max(1e-12, 8 * n * np.finfo(np.float64).eps * (1 + 0.5 * np.sqrt(spectrum[-1] / spectrum[0])))
    got = scoring.coral(out_model, x)
    errs = [np.abs(a - b).max() / np.abs(b).max() for a, b in ((got.mean, mean), (got.within_var, S_w), (got.between_var, S_b))]
    print("coral n=%d dim=%d: rel err mean %.3g, within %.3g, between %.3g (tolerance %.3g, cond %.3g)" % (n, dim, *errs, tol, spectrum[-1] / spectrum[0]))
    assert max(errs) <= tol


def test_in_domain_training_adaptation_and_scoring_on_the_device(g):
    """asv_plda_train on the labelled in-domain set (covariance form) -> cip / lip_reg against the out-of-domain model ->
    to_plda -> device transform + LLR, against the LLRs the reference computed from its own EM, adaptors and scoring.  The
    bound is the one every comparison of the float32 scoring kernels with reference LLRs in this suite uses
    (tests/test_gpu_scoring.py: test_plda_transform_and_llr_vs_reference_fixture and
    test_unsupervised_plda_adaptation_and_zca_match_the_reference; the EM itself is pinned to 1e-9 by
    test_plda_training_on_the_device_matches_the_reference_em, far below it)."""
    from libs.amd import scoring
    out_model, _ = models(g)
    in_model = scoring.train_plda_covariances(g["in_x"], g["in_labels"], num_iters=int(g["em_iters"]))
    assert isinstance(in_model, scoring.PldaCovariances)
    assert np.abs(in_model.mean - g["in_mean"]).max() < 1e-10
    assert np.abs(in_model.within_var - g["in_within_var"]).max() < 1e-9 and np.abs(in_model.between_var - g["in_between_var"]).max() < 1e-9
    for name, model in (("cip", scoring.cip(out_model, g["adapt"], in_model)), ("lip_reg", scoring.lip_reg(out_model, in_model))):
        plda = model.to_plda()
        t = plda.transform_vectors(g["ev"])
        llr = plda.llr_trials(t, t, g["trials_e"], g["trials_t"]).cpu().numpy()
        want = g[name + "_llr"]
        err = np.abs(llr - want).max()
        print("%s: device LLR max abs err %.3g (max |llr| %.3g)" % (name, err, np.abs(want).max()))
        assert err < 2e-3 * max(1.0, np.abs(want).max() / 10), name


def test_adaptation_lowers_the_eer_on_the_in_domain_trials(g):
    """On the planted data the unadapted out-of-domain model scores the in-domain trials worse than the CORAL-adapted one - in
    the reference's own scores (the generator asserts it) and here, all on the device."""
    from libs.amd import scoring
    out_model, in_model = models(g)
    eers = {}
    for tag, model in (("unadapted", out_model), ("coral", scoring.coral(out_model, g["adapt"]))):
        plda = model.to_plda()
        t = plda.transform_vectors(g["ev"])
        eers[tag], _ = scoring.eer(plda.llr_trials(t, t, g["trials_e"], g["trials_t"]), g["trials_tgt"])
    print("EER: unadapted %.2f %%, CORAL %.2f %% (reference: %.2f / %.2f)" % (eers["unadapted"], eers["coral"], 100 * float(g["eer_unadapted"]), 100 * float(g["eer_coral"])))
    assert eers["coral"] < eers["unadapted"]
    assert float(g["eer_coral"]) < float(g["eer_unadapted"])


@pytest.mark.parametrize("script,name", [("ivector-adapt-plda-coral.py", "coral"), ("ivector-adapt-plda-coralplus.py", "coral_plus"),
                                         ("ivector-adapt-plda-cip.py", "cip"), ("ivector-adapt-plda-cip-reg.py", "cip_reg"),
                                         ("ivector-adapt-plda.py", None)])
def test_scripts_with_device_statistics_end_to_end(g, tmp_path, script, name):
    """The five scripts whose statistics come from the device (the two others run in tests/test_plda_adapt_host.py): arks in,
    Kaldi text <Plda> out, scored by the float64 restatement - the fixture's LLRs; for the Kaldi-style adaptor (no fixture of this
    shape: tests/test_gpu_scoring.py pins its arithmetic) the LLRs of the same call made in this process."""
    from libs.amd import scoring
    from libs.support import kaldi_io
    out_model, in_model = models(g)
    out_model.write_stats_ark(str(tmp_path / "plda_out"))
    in_model.write_stats_ark(str(tmp_path / "plda_in"))
    kaldi_io.write_vec_flt_ark_scp(str(tmp_path / "adapt.ark"), str(tmp_path / "adapt.scp"), [("utt%03d" % i, v) for i, v in enumerate(g["adapt"])])
    rspecifier = "scp:%s" % (tmp_path / "adapt.scp") if name == "cip" else "ark:%s" % (tmp_path / "adapt.ark")
    args = [tmp_path / "plda_out", rspecifier] + ([tmp_path / "plda_in"] if name in ("cip", "cip_reg") else []) + [tmp_path / "plda_adapt"]
    r = run_script(script, "--gpu-id", "0", *args)
    assert r.returncode == 0, r.stderr
    mean, transform, psi = read_kaldi_text_plda(str(tmp_path / "plda_adapt"))
    llr = llr_f64(mean, transform, psi, g["ev"], g["trials_e"], g["trials_t"])
    if name is not None:
        check_llr(g, name, llr)
    else:
        want = scoring.Plda.read_stats_ark(str(tmp_path / "plda_out")).adapt_unsupervised(g["adapt"])
        want = llr_f64(want.mean, want.transform, want.psi, g["ev"], g["trials_e"], g["trials_t"])
        assert np.abs(llr - want).max() <= 1e-12 * np.abs(want).max()
