"""PLDA domain adaptors (CORAL, CORAL+, CIP, CIP-reg, LIP, LIP-reg) of libs.amd.scoring against the outputs of the reference's
own classes (tests/golden/plda_domain_adapt.npz, written by tests/gen_plda_adapt_golden.py) - the host half: the D x D algebra.
The adaptation-set statistics come from a float64 numpy stand-in for scoring.second_moments here; tests/test_gpu_plda_adapt.py
runs the same checks with the device kernel.

Tolerance, covariances / mean and LLRs alike: 10 x the spread the generator recorded between the reference and a float64
restatement that symmetrises its eigh inputs (spread_<adaptor>, spread_llr_<adaptor>; a property of the reference's arithmetic
alone), floored at 1e-12, on max |delta| / max |value|.  The factor 10 covers LAPACK builds.

Scripts: the two that need no device (LIP, LIP-reg) run end to end here, and all seven are checked for the reference's usage
line; the five whose statistics come from the device run in tests/test_gpu_plda_adapt.py (there is no CPU path)."""

import os

import numpy as np
import pytest

from plda_adapt_common import ADAPTORS, USAGE, check_against_fixture, check_llr, llr_f64, load_fixture, models, read_kaldi_text_plda, run_adaptor, run_script


@pytest.fixture(scope="module")
def g():
    return load_fixture()


@pytest.fixture
def cpu_moments(monkeypatch):
    """float64 numpy in place of the device statistics (asv_scatter_f64)."""
    from libs.amd import scoring

    def moments(vectors):
        x = np.asarray(vectors, dtype=np.float64)
        return x.sum(0), x.T.dot(x)
    monkeypatch.setattr(scoring, "second_moments", moments)


@pytest.mark.parametrize("name", ADAPTORS)
def test_adaptor_matches_the_reference(g, cpu_moments, name):
    out_model, in_model = models(g)
    keep = [np.array(m.within_var) for m in (out_model, in_model)]
    model = run_adaptor(name, out_model, in_model, g["adapt"])
    check_against_fixture(g, name, model)
    assert all((m.within_var == k).all() for m, k in zip((out_model, in_model), keep)), "the input models are not changed"


def test_defaults_are_the_reference_constructors(g, cpu_moments):
    """The fixture was made with the defaults of the reference's classes: passing them explicitly changes nothing."""
    from libs.amd import scoring
    out_model, in_model = models(g)
    a = g["adapt"]
    for got, want in ((scoring.coral(out_model, a, mean_diff_scale=1.0), scoring.coral(out_model, a)),
                      (scoring.coral_plus(out_model, a, 0.8, 0.8, 1.0), scoring.coral_plus(out_model, a)),
                      (scoring.cip(out_model, a, in_model, 0.5), scoring.cip(out_model, a, in_model)),
                      (scoring.cip_reg(out_model, a, in_model, 0.5), scoring.cip_reg(out_model, a, in_model)),
                      (scoring.lip(out_model, in_model, 0.4), scoring.lip(out_model, in_model)),
                      (scoring.lip_reg(out_model, in_model, 0.6), scoring.lip_reg(out_model, in_model))):
        assert (got.within_var == want.within_var).all() and (got.between_var == want.between_var).all() and (got.mean == want.mean).all()


def test_limiting_cases(g, cpu_moments):
    from libs.amd import scoring
    out_model, in_model = models(g)
    adapt = g["adapt"]
    m = scoring.lip(out_model, in_model, interpolation_weight=1.0)
    assert (m.within_var == out_model.within_var).all() and (m.between_var == out_model.between_var).all()
    m = scoring.lip(out_model, in_model, interpolation_weight=0.0)
    assert (m.within_var == in_model.within_var).all() and (m.between_var == in_model.between_var).all() and (m.mean == in_model.mean).all()
    m = scoring.cip(out_model, adapt, in_model, interpolation_weight=0.0)
    assert (m.within_var == in_model.within_var).all() and (m.between_var == in_model.between_var).all() and (m.mean == in_model.mean).all()
    # the defining property of CORAL: the adapted total covariance IS the adaptation variance (a transposed A, or C_i and C_o
    # swapped, breaks it)
    x = adapt.astype(np.float64)
    mean = x.mean(0)
    d = mean - out_model.mean
    variance = x.T.dot(x) / len(x) - np.outer(mean, mean) + np.outer(d, d)
    m = scoring.coral(out_model, adapt)
    assert np.abs(m.within_var + m.between_var - variance).max() <= 1e-9 * np.abs(variance).max()
    assert np.abs(m.mean - mean).max() <= 1e-12 * np.abs(mean).max()
    m0 = scoring.coral(out_model, adapt, mean_diff_scale=0.0)
    assert np.abs(m0.within_var + m0.between_var - (variance - np.outer(d, d))).max() <= 1e-9 * np.abs(variance).max()
    # Weyl: the regularised interpolations add a positive semi-definite term, no eigenvalue of the in-domain covariance drops
    for m in (scoring.lip_reg(out_model, in_model), scoring.cip_reg(out_model, adapt, in_model)):
        for new, base in ((m.within_var, in_model.within_var), (m.between_var, in_model.between_var)):
            diff = new - base
            assert np.linalg.eigvalsh(0.5 * (diff + diff.T)).min() >= -1e-12 * np.abs(base).max()
            assert np.abs(diff).max() > 1e-3 * np.abs(base).max()                # and the term is there
        assert (m.mean == in_model.mean).all()


def test_bad_input_raises_value_error(g, cpu_moments):
    from libs.amd import scoring
    out_model, in_model = models(g)
    adapt = g["adapt"]
    with np.errstate(all="raise"):
        with pytest.raises(ValueError, match="not positive definite"):            # 10 vectors in 24 dimensions: rank 10
            scoring.coral(out_model, adapt[:10])
        with pytest.raises(ValueError, match="not positive definite"):
            scoring.cip_reg(out_model, adapt[:10], in_model)
        singular = scoring.PldaCovariances(out_model.mean, out_model.within_var - out_model.within_var, out_model.between_var - out_model.between_var)
        with pytest.raises(ValueError, match="not positive definite"):
            scoring.coral(singular, adapt)
        with pytest.raises(ValueError, match="not positive definite"):
            scoring.lip_reg(out_model, singular)
    with pytest.raises(ValueError, match="at least 2"):
        scoring.coral(out_model, adapt[:1])
    with pytest.raises(ValueError, match="do not fit"):
        scoring.coral_plus(out_model, adapt[:, :20])
    small = scoring.PldaCovariances(in_model.mean[:20], in_model.within_var[:20, :20], in_model.between_var[:20, :20])
    for call in (lambda: scoring.lip(out_model, small), lambda: scoring.lip_reg(out_model, small), lambda: scoring.cip(out_model, adapt, small),
                 lambda: scoring.cip_reg(out_model, adapt, small)):
        with pytest.raises(ValueError, match="different dimensions"):
            call()
    with pytest.raises(ValueError):
        scoring.PldaCovariances(out_model.mean, out_model.within_var[:20], out_model.between_var)


def test_stats_ark_round_trip(g, tmp_path):
    """write_stats_ark writes what PldaEstimation.plda_write writes: float64, bit exact through read_stats_ark, and readable by the
    model classes that were there before."""
    from libs.amd import scoring
    from libs.support import kaldi_io
    out_model, _ = models(g)
    path = str(tmp_path / "plda")
    out_model.write_stats_ark(path)
    assert [(k, v.dtype, v.shape) for k, v in kaldi_io.read_vec_flt_ark(path)] == [
        ("mean", np.float64, (24,)), ("within_var", np.float64, (576,)), ("between_var", np.float64, (576,))]
    back = scoring.PldaCovariances.read_stats_ark(path)
    assert (back.mean == out_model.mean).all() and (back.within_var == out_model.within_var).all() and (back.between_var == out_model.between_var).all()
    a, b = scoring.Plda.read_stats_ark(path), out_model.to_plda()
    assert (a.psi == b.psi).all() and (a.transform == b.transform).all()
    with open(path, "wb") as f:
        kaldi_io.write_vec_flt(f, out_model.mean, key="mean")
    with pytest.raises(ValueError, match="within_var"):
        scoring.PldaCovariances.read_stats_ark(path)


@pytest.mark.parametrize("script,name", [("ivector-adapt-plda-lip.py", "lip"), ("ivector-adapt-plda-lip-reg.py", "lip_reg")])
def test_interpolation_scripts_end_to_end(g, tmp_path, script, name):
    out_model, in_model = models(g)
    out_model.write_stats_ark(str(tmp_path / "plda_out"))
    in_model.write_stats_ark(str(tmp_path / "plda_in"))
    r = run_script(script, "--gpu-id", "0", tmp_path / "plda_out", tmp_path / "plda_in", tmp_path / "plda_adapt")
    assert r.returncode == 0, r.stderr
    mean, transform, psi = read_kaldi_text_plda(str(tmp_path / "plda_adapt"))
    check_llr(g, name, llr_f64(mean, transform, psi, g["ev"], g["trials_e"], g["trials_t"]))
    r = run_script(script, tmp_path / "plda_out", tmp_path / "missing", tmp_path / "plda_adapt2")      # an error is loud
    assert r.returncode == 1 and "missing" in r.stderr and not os.path.exists(tmp_path / "plda_adapt2")


@pytest.mark.parametrize("script", sorted(USAGE))
def test_wrong_argument_count_prints_the_reference_usage(tmp_path, script):
    """The reference: `print('<...> \\n')` and a plain sys.exit() - status 0, nothing written."""
    count = len(USAGE[script].split())
    for args in ([], ["a"] * (count - 1), ["a"] * (count + 1), ["--gpu-id", "0"] + ["a"] * (count - 1)):
        r = run_script(script, *args)
        assert r.returncode == 0 and r.stdout == USAGE[script] + " \n\n", (script, args, r)
