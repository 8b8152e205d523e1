"""minDCF / DET curve / Cavg on the host: the C ABI list, the command-line drop-ins' parsing (against a stubbed scoring module)
and a vectorised numpy restatement of the reference's two metric scripts that reproduces every recorded case of
tests/golden/det_metrics.npz (written by tests/gen_det_metrics_golden.py from the reference's own code) EXACTLY - the GPU tests
use it where the fixture holds no arrays."""

import hashlib
import importlib.util
import os

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "asv-subtools_amd")
_golden = {}


def golden():
    if not _golden:
        with np.load(os.path.join(REPO, "tests", "golden", "det_metrics.npz")) as z:
            _golden.update({k: z[k] for k in z.files})
    return _golden


def cases(kind):
    return sorted({k.split("/")[1] for k in golden() if k.startswith(kind + "/")})


def case(kind, name):
    prefix = "%s/%s/" % (kind, name)
    return {k[len(prefix):]: v for k, v in golden().items() if k.startswith(prefix)}


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- the restatement ---------------------------------------------------------------------------------------------------------

def np_det_curve(scores, labels):
    """ComputeErrorRates: a stable sort by score alone (numpy orders -0.0 and +0.0 as equal, like Python), integer running
    counts, one float64 division each."""
    scores = np.asarray(scores, dtype=np.float32)
    order = np.argsort(scores, kind="stable")
    lab = (np.asarray(labels)[order] != 0).astype(np.int64)
    cum_tgt, cum_non = np.cumsum(lab), np.cumsum(1 - lab)
    fnr = cum_tgt / float(cum_tgt[-1])
    fpr = 1 - cum_non / float(cum_non[-1])
    return fnr, fpr, scores[order]


def np_min_dcf(fnr, fpr, thresholds, p_target, c_miss, c_fa):
    """ComputeMinDcf: numpy evaluates the expression in Python's order, one rounding per operation; argmin is the first minimum."""
    c_det = c_miss * fnr * p_target + c_fa * fpr * (1 - p_target)
    i = int(np.argmin(c_det))
    return float(c_det[i] / min(c_miss * p_target, c_fa * (1 - p_target))), float(thresholds[i])


def np_cavg(scores, model_lang, true_lang, lang_num, bins=20, p_target=0.5):
    """get_cavg: the pairs are counted per (model, true language or unknown, number of thresholds at or below the score); the
    float64 arithmetic on the counts is the reference's, statement by statement."""
    s = np.asarray(scores, dtype=np.float32).astype(np.float64)
    m, t = np.asarray(model_lang, dtype=np.int64), np.asarray(true_lang, dtype=np.int64)
    lo, hi = float(s.min()), float(s.max())
    precision = (hi - lo) / bins
    thr = np.asarray([lo + section * precision for section in range(bins + 1)])
    k = (s[:, None] >= thr[None, :]).sum(axis=1)
    hist = np.zeros((lang_num, lang_num + 1, bins + 2), dtype=np.int64)
    np.add.at(hist, (m, np.where(t < 0, lang_num, t), k), 1)
    accepted = hist[:, :, ::-1].cumsum(axis=2)[:, :, ::-1]            # [.., k]: pairs with at least k thresholds at or below
    cavgs = []
    for section in range(bins + 1):
        target_cavg = []
        for lang in range(lang_num):
            LTa = float(accepted[lang, lang, 0])
            LTm = float(accepted[lang, lang, 0] - accepted[lang, lang, section + 1])
            p_miss = LTm / LTa if LTa != 0.0 else 0.0
            total = 0
            for i in range(lang_num):
                LNa = 0 if i == lang else accepted[lang, i, 0]
                LNf = 0 if i == lang else accepted[lang, i, section + 1]
                if i == lang_num - 1:                                  # LNa[-1] / LNf[-1]: the unknown utterances
                    LNa, LNf = LNa + accepted[lang, lang_num, 0], LNf + accepted[lang, lang_num, section + 1]
                total = total + (float(LNf) / float(LNa) if LNa != 0 else 0.0)
            p_nontarget = (1 - p_target) / (lang_num - 1)
            target_cavg.append(p_target * p_miss + p_nontarget * total)
        acc = 0
        for v in target_cavg:
            acc = acc + v
        cavgs.append(acc / lang_num)
    return min(cavgs), cavgs


# ---- the restatement against the reference's recorded results ------------------------------------------------------------------

@pytest.mark.parametrize("name", cases("dcf"))
def test_numpy_restatement_reproduces_the_reference_det_curve_and_min_dcf(name):
    c = case("dcf", name)
    fnr, fpr, thr = np_det_curve(c["scores"], c["labels"])
    if "sha256" in c:
        assert [sha256(fnr), sha256(fpr), sha256(thr)] == list(c["sha256"])
    else:
        assert fnr.tobytes() == c["fnr"].tobytes() and fpr.tobytes() == c["fpr"].tobytes()
        assert thr.tobytes() == c["thresholds"].tobytes()              # bytes: a -0.0 stays a -0.0
    for (p, cm, cf), want, want_thr in zip(c["points"], c["min_dcf"], c["threshold"]):
        got, got_thr = np_min_dcf(fnr, fpr, thr, p, cm, cf)
        assert got == want and got_thr == want_thr, (name, p, cm, cf, got, want)


def test_tie_case_tells_a_label_in_key_sort_from_the_stable_sort():
    c = case("dcf", "ties64")
    assert len(np.unique(c["scores"])) == 64
    assert (c["label_in_key_min_dcf"] != c["min_dcf"]).any()


@pytest.mark.parametrize("name", cases("cavg"))
def test_numpy_restatement_reproduces_the_reference_cavg(name):
    c = case("cavg", name)
    lang_num, bins, p_target = int(c["params"][0]), int(c["params"][1]), float(c["params"][2])
    best, cavgs = np_cavg(c["scores"], c["model_lang"], c["true_lang"], lang_num, bins, p_target)
    assert np.asarray(cavgs).tobytes() == c["cavgs"].tobytes() and best == float(c["min_cavg"])


def test_unknown_utterances_are_folded_not_dropped():
    assert float(case("cavg", "l10_unknown")["min_cavg"]) != float(case("cavg", "l10_unknown_dropped")["min_cavg"])


# ---- C ABI list ------------------------------------------------------------------------------------------------------------------

def test_capi_lists_the_three_symbols_and_the_header_declares_them():
    from libs.amd import capi
    hdr = open(os.path.join(REPO, "include", "asv_amd.h")).read()
    for name in ("asv_det_curve", "asv_min_dcf", "asv_cavg"):
        assert name in capi.SYMBOLS and ("int %s(" % name) in hdr


# ---- command-line drop-ins ---------------------------------------------------------------------------------------------------------

def load_script(rel):
    spec = importlib.util.spec_from_file_location("cli_" + os.path.basename(rel).replace(".", "_").replace("-", "_"), os.path.join(PKG, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class StubScoring(object):
    """Records what the command line hands to libs.amd.scoring and answers with the numpy restatement."""

    def __init__(self):
        self.calls = []

    def min_dcf(self, scores, labels, p_target=0.01, c_miss=1, c_fa=1):
        self.calls.append(("min_dcf", np.asarray(scores), np.asarray(labels), p_target, c_miss, c_fa))
        assert np.asarray(scores).dtype == np.float32
        return np_min_dcf(*np_det_curve(scores, labels), p_target, c_miss, c_fa)

    def cavg(self, scores, model_lang, true_lang, lang_num, bins=20, p_target=0.5):
        self.calls.append(("cavg", np.asarray(scores), np.asarray(model_lang), np.asarray(true_lang), lang_num, bins, p_target))
        assert np.asarray(scores).dtype == np.float32
        return np_cavg(scores, model_lang, true_lang, lang_num, bins, p_target)


def write_cli_files(tmp_path, kind):
    c = case("cli", kind)
    paths = {}
    for key in c:
        if key.endswith("_txt"):
            paths[key[:-4]] = tmp_path / (key[:-4] + ".txt")
            paths[key[:-4]].write_text(str(c[key]))
    return c, paths


def test_min_dcf_cli_prints_the_reference_string(tmp_path, capsys):
    cli = load_script(os.path.join("kaldi", "sid", "compute_min_dcf.py"))
    c, paths = write_cli_files(tmp_path, "dcf")
    stub = StubScoring()
    assert cli.main([str(x) for x in c["args"]] + [str(paths["scores"]), str(paths["trials"])], scoring=stub) == 0
    out = capsys.readouterr()
    assert out.out == str(c["stdout"])
    assert out.err.splitlines()[-1].startswith("minDCF is %s at threshold " % str(c["stdout"]).strip())
    assert out.err.splitlines()[-1].endswith("(p-target=0.05, c-miss=1.0,c-fa=1.0)")
    assert cli.main([str(paths["scores"]), str(paths["trials"])], scoring=stub) == 0          # the defaults: 0.01 / 1 / 1
    assert capsys.readouterr().out == str(c["stdout_default"])
    (_, scores, labels, p, cm, cf) = stub.calls[-1]
    assert (p, cm, cf) == (0.01, 1, 1) and len(scores) == len(labels) == len(str(c["scores_txt"]).splitlines())
    assert labels.sum() == sum(line.endswith(" target") for line in str(c["trials_txt"]).splitlines())


def test_min_dcf_cli_rejects_a_scored_pair_the_trials_file_lacks_and_bad_costs(tmp_path):
    cli = load_script(os.path.join("kaldi", "sid", "compute_min_dcf.py"))
    c, paths = write_cli_files(tmp_path, "dcf")
    lines = str(c["trials_txt"]).splitlines(True)
    first_scored = tuple(str(c["scores_txt"]).splitlines()[0].split()[:2])
    paths["trials"].write_text("".join(l for l in lines if tuple(l.split()[:2]) != first_scored))
    with pytest.raises(KeyError, match="Missing entry for %s and %s" % first_scored):
        cli.main([str(paths["scores"]), str(paths["trials"])], scoring=StubScoring())
    for bad in (["--c-fa", "0"], ["--c-miss", "-1"], ["--p-target", "0"], ["--p-target", "1"]):
        with pytest.raises(ValueError, match="must be greater than 0"):
            cli.main(bad + [str(paths["scores"]), str(paths["trials"])], scoring=StubScoring())


def test_cavg_cli_pairs_and_matrix_forms_parse_to_the_same_arrays(tmp_path, capsys):
    cli = load_script("computeCavg.py")
    c, paths = write_cli_files(tmp_path, "cavg")
    lang2id, utt2lang_id, listed = cli.read_trials(str(paths["trials"]))
    assert [k for k, _ in sorted(lang2id.items(), key=lambda kv: kv[1])] == list(c["lang_order"]) == sorted(lang2id)
    a = cli.read_pair_scores(str(paths["pairs"]), lang2id, utt2lang_id, listed)
    b = cli.read_matrix_scores(str(paths["matrix"]), lang2id, utt2lang_id, listed)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert np.array_equal(a[0], c["model_lang"]) and np.array_equal(a[1], c["true_lang"])
    assert (a[1] == -1).any() and len(a[2]) < len(str(c["pairs_txt"]).splitlines())            # unknown utterances; unlisted pairs dropped
    for form, key in (("-pairs", "pairs"), ("-matrix", "matrix")):
        stub = StubScoring()
        assert cli.main([form, str(paths["trials"]), str(paths[key])], scoring=stub) == 0
        assert capsys.readouterr().out == str(c["stdout"])
        assert stub.calls[0][4:] == (4, 20, 0.5)
    assert cli.main(["-pairs", str(paths["trials"])], scoring=StubScoring()) == 0
    assert capsys.readouterr().out.startswith("usage:")


def test_getcavg_wrapper_calls_the_pair_form_and_keeps_the_number():
    text = open(os.path.join(PKG, "score", "metric", "getCavg.sh")).read()
    assert "subtools/computeCavg.py -pairs" in text and "awk '{print $2}'" in text
    assert os.access(os.path.join(PKG, "score", "metric", "getCavg.sh"), os.X_OK) and os.access(os.path.join(PKG, "computeCavg.py"), os.X_OK)
