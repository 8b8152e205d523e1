"""minDCF / DET curve / Cavg on the device (asv_det_curve, asv_min_dcf, asv_cavg) against the reference's recorded results
(tests/golden/det_metrics.npz) and, for sizes the fixture does not hold, against the numpy restatement that
tests/test_det_metrics_host.py proves equal to the reference on every recorded case.

Every comparison is EXACT.  That is derived, not measured: the device sorts by (score, trial index), which is the reference's
stable sort; the running counts are integers; fnr / fpr are one IEEE float64 division (and one subtraction) of the same
integers on both sides; the cost is the same five float64 operations in the same order, unfused; the Cavg counts are integers
and the float64 arithmetic on them runs in the reference's statement order.  A last-bit difference is a bug to locate."""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import test_det_metrics_host as H

pytestmark = pytest.mark.gpu


def _scoring():
    from libs.amd import scoring
    return scoring


def check_det_curve(scores, labels, want=None):
    """Device DET curve == restatement, bytes (a -0.0 threshold stays -0.0); `want`: the fixture's arrays or digests."""
    fnr, fpr, thr = (t.cpu().numpy() for t in _scoring().det_curve(scores, labels))
    assert fnr.dtype == np.float64 and fpr.dtype == np.float64 and thr.dtype == np.float32
    r_fnr, r_fpr, r_thr = H.np_det_curve(scores, labels)
    bad = np.flatnonzero((fnr != r_fnr) | (fpr != r_fpr))
    assert bad.size == 0, (bad[:5], fnr[bad[:5]], r_fnr[bad[:5]], fpr[bad[:5]], r_fpr[bad[:5]])
    assert thr.tobytes() == r_thr.tobytes()
    if want is not None and "sha256" in want:
        assert [H.sha256(fnr), H.sha256(fpr), H.sha256(thr)] == list(want["sha256"])
    elif want is not None:
        assert fnr.tobytes() == want["fnr"].tobytes() and fpr.tobytes() == want["fpr"].tobytes() and thr.tobytes() == want["thresholds"].tobytes()
    return r_fnr, r_fpr, r_thr


@pytest.mark.parametrize("name", H.cases("dcf"))
def test_det_curve_and_min_dcf_equal_the_reference_bit_for_bit(name):
    """n = 2 both ways round, 257 (one past a workgroup), 20 000 Gaussian, 20 000 in 64 tie groups (fails with the label in the sort
    key), all scores equal, -0.0 / +0.0, the minimum at the first and at the last sorted trial; all points of a case in ONE call."""
    c = H.case("dcf", name)
    check_det_curve(c["scores"], c["labels"], c)
    pts = c["points"]
    got, thr = _scoring().min_dcf(c["scores"], c["labels"], p_target=list(pts[:, 0]), c_miss=list(pts[:, 1]), c_fa=list(pts[:, 2]))
    print(name, got, list(c["min_dcf"]))
    assert got == list(c["min_dcf"]) and thr == list(c["threshold"])
    if name == "ties64":
        assert got != list(c["label_in_key_min_dcf"])


@pytest.mark.parametrize("name", ["n257", "gauss20000"])
def test_eight_operating_points_in_one_call_equal_eight_calls(name):
    c = H.case("dcf", name)
    pts = c["points"]
    assert len(pts) == 8
    many = _scoring().min_dcf(c["scores"], c["labels"], list(pts[:, 0]), list(pts[:, 1]), list(pts[:, 2]))
    for k, (p, cm, cf) in enumerate(pts):
        one = _scoring().min_dcf(c["scores"], c["labels"], float(p), float(cm), float(cf))
        assert isinstance(one[0], float) and one == (many[0][k], many[1][k])
    # a scalar beside sequences is broadcast; more than 8 points run in groups
    more = _scoring().min_dcf(c["scores"], c["labels"], list(pts[:, 0]) + [0.02, 0.2], 1, [1.0] * 10)
    assert len(more[0]) == 10 and more[0][0] == many[0][0] and more[0][1] == many[0][1]


def test_two_hundred_thousand_trials_cross_every_stage():
    """n = 200 003: an odd tail, hundreds of workgroups in the sweep, the second reduction stage over their minima."""
    rng = np.random.default_rng(7)
    n = 200003
    labels = (rng.random(n) < 0.08).astype(np.int32)
    scores = (rng.standard_normal(n) + 2.2 * labels).astype(np.float32)
    scores[rng.integers(0, n, 5000)] = scores[rng.integers(0, n, 5000)]          # some exact ties as well
    fnr, fpr, thr = check_det_curve(scores, labels)
    pts = H.case("dcf", "n257")["points"]
    got, got_thr = _scoring().min_dcf(scores, labels, list(pts[:, 0]), list(pts[:, 1]), list(pts[:, 2]))
    want = [H.np_min_dcf(fnr, fpr, thr, p, cm, cf) for p, cm, cf in pts]
    assert got == [w[0] for w in want] and got_thr == [w[1] for w in want]


def check_cavg(scores, model, true, lang_num, bins, p_target, want_best, want_cavgs):
    best, cavgs = _scoring().cavg(scores, model, true, lang_num, bins=bins, p_target=p_target)
    assert len(cavgs) == bins + 1
    assert cavgs == [float(x) for x in want_cavgs], [(i, a, b) for i, (a, b) in enumerate(zip(cavgs, want_cavgs)) if a != b][:4]
    assert best == float(want_best)
    return best


@pytest.mark.parametrize("name", H.cases("cavg"))
def test_cavg_equals_the_reference_bit_for_bit(name):
    """2 / 5 / 6 / 10 / 40 languages (40: counters beyond the per-wavefront LDS histogram), bins 1 / 7 / 20, unknown utterances,
    scores exactly on thresholds, a sparse pair list with empty slots."""
    c = H.case("cavg", name)
    lang_num, bins, p_target = int(c["params"][0]), int(c["params"][1]), float(c["params"][2])
    check_cavg(c["scores"], c["model_lang"].astype(np.int32), c["true_lang"].astype(np.int32), lang_num, bins, p_target, c["min_cavg"], c["cavgs"])


def test_cavg_unknown_utterances_count_for_the_last_language():
    a, b = H.case("cavg", "l10_unknown"), H.case("cavg", "l10_unknown_dropped")
    got = [_scoring().cavg(c["scores"], c["model_lang"].astype(np.int32), c["true_lang"].astype(np.int32), 10)[0] for c in (a, b)]
    assert got == [float(a["min_cavg"]), float(b["min_cavg"])] and got[0] != got[1]


def test_cavg_of_five_thousand_utterances_in_matrix_form():
    rng = np.random.default_rng(11)
    n_utts, lang_num = 5000, 10
    true = rng.integers(0, lang_num, n_utts)
    sc = rng.standard_normal((n_utts, lang_num))
    sc[np.arange(n_utts), true] += 1.5
    true[rng.random(n_utts) < 0.1] = -1
    scores, model, tl = sc.reshape(-1).astype(np.float32), np.tile(np.arange(lang_num), n_utts).astype(np.int32), np.repeat(true, lang_num).astype(np.int32)
    for bins in (1, 20):
        want_best, want = H.np_cavg(scores, model, tl, lang_num, bins, 0.5)
        check_cavg(scores, model, tl, lang_num, bins, 0.5, want_best, want)


def test_every_error_is_a_message_and_the_device_stays_usable():
    import torch
    from libs.amd import capi
    S = _scoring()
    c = H.case("dcf", "n257")
    s, l = c["scores"], c["labels"]
    nan = s.copy()
    nan[100] = np.nan
    bad_dcf = [
        ("at least 2", lambda: S.min_dcf(s[:1], l[:1])),
        ("at least 2", lambda: S.det_curve(s[:1], l[:1])),
        ("both target and non-target", lambda: S.min_dcf(s, np.zeros_like(l))),
        ("both target and non-target", lambda: S.min_dcf(s, np.ones_like(l))),
        ("both target and non-target", lambda: S.det_curve(s, np.ones_like(l))),
        ("c_miss must be greater than 0", lambda: S.min_dcf(s, l, c_miss=0)),
        ("c_fa must be greater than 0", lambda: S.min_dcf(s, l, c_fa=-1.0)),
        ("p_target must be greater than 0 and less than 1", lambda: S.min_dcf(s, l, p_target=0.0)),
        ("p_target must be greater than 0 and less than 1", lambda: S.min_dcf(s, l, p_target=[0.01, 1.0])),
        ("NaN", lambda: S.min_dcf(nan, l)),
        ("NaN", lambda: S.det_curve(nan, l)),
    ]
    g = H.case("cavg", "l2")
    gs, gm, gt = g["scores"], g["model_lang"].astype(np.int32), g["true_lang"].astype(np.int32)
    gnan = gs.copy()
    gnan[3] = np.nan

    def patched(a, i, v):
        a = a.copy()
        a[i] = v
        return a
    bad_cavg = [
        ("at least 2", lambda: S.cavg(gs, np.zeros_like(gm), np.zeros_like(gt), 1)),
        ("at least 1", lambda: S.cavg(gs, gm, gt, 2, bins=0)),
        ("model_lang outside", lambda: S.cavg(gs, patched(gm, 5, 2), gt, 2)),
        ("model_lang outside", lambda: S.cavg(gs, patched(gm, 5, -1), gt, 2)),
        ("true_lang outside", lambda: S.cavg(gs, gm, patched(gt, 7, 2), 2)),
        ("true_lang outside", lambda: S.cavg(gs, gm, patched(gt, 7, -2), 2)),
        ("NaN", lambda: S.cavg(gnan, gm, gt, 2)),
        ("divides by the zero range", lambda: S.cavg(np.full_like(gs, 0.25), gm, gt, 2)),
    ]
    for what, call in bad_dcf + bad_cavg:
        with pytest.raises(capi.AsvError, match=what):
            call()
    # the number of operating points is checked by the C entry point itself (the Python function groups longer lists by 8)
    sd, ld = torch.from_numpy(s).cuda(), torch.from_numpy(l.astype(np.int32)).cuda()
    for n_points in (0, 9):
        arr = (C.c_double * 9)(*([0.5] * 9))
        out, thr = (C.c_double * 9)(), (C.c_float * 9)()
        rc = capi.lib().asv_min_dcf(C.c_void_p(sd.data_ptr()), C.c_void_p(ld.data_ptr()), len(s), arr, arr, arr, n_points, out, thr, None)
        assert rc < 0 and b"operating points" in capi.lib().asv_last_error()
    assert S.min_dcf(s, l)[0] == float(c["min_dcf"][0])
    assert S.cavg(gs, gm, gt, 2)[0] == float(g["min_cavg"])


def test_eer_is_unchanged_by_a_min_dcf_call():
    c = H.case("dcf", "gauss20000")
    before = _scoring().eer(c["scores"], c["labels"].astype(np.int32))
    _scoring().min_dcf(c["scores"], c["labels"])
    _scoring().det_curve(c["scores"], c["labels"])
    assert _scoring().eer(c["scores"], c["labels"].astype(np.int32)) == before


def test_command_line_tools_print_the_reference_strings(tmp_path, capsys):
    """compute_min_dcf.py as a process of its own (its path bootstrap included), computeCavg.py through its main()."""
    c, paths = H.write_cli_files(tmp_path, "dcf")
    script = os.path.join(H.PKG, "kaldi", "sid", "compute_min_dcf.py")
    r = subprocess.run([sys.executable, script] + [str(x) for x in c["args"]] + [str(paths["scores"]), str(paths["trials"])], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == str(c["stdout"]) and ("minDCF is %s at threshold" % str(c["stdout"]).strip()) in r.stderr
    g, gpaths = H.write_cli_files(tmp_path, "cavg")
    cli = H.load_script("computeCavg.py")
    for form, key in (("-pairs", "pairs"), ("-matrix", "matrix")):
        assert cli.main([form, str(gpaths["trials"]), str(gpaths[key])]) == 0
        assert capsys.readouterr().out == str(g["stdout"])
