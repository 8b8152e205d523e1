#!/usr/bin/env python3
"""Generate tests/golden/det_metrics.npz by running the REFERENCE's metric code: ComputeErrorRates / ComputeMinDcf of
kaldi/sid/compute_min_dcf.py (imported) and get_cavg of computeCavg.py.  Build container only (needs the reference tree).  The
fixture holds inputs and recorded results, nothing else.

computeCavg.py is a Python 2 script: its `__main__` block does not parse under Python 3, the functions above it do.  Its text is
executed up to that block.  The one pin: Python 2's sum() adds left to right; from 3.12 on sum() of floats is compensated, so
the name `sum` is bound to a plain left-to-right sum in that namespace - the arithmetic the script was written for.

All scores are float32 values (handed to the reference as Python floats), because that is what the device is given.  Cases
above 4096 trials record sha256 digests of the fnr / fpr / thresholds bytes in place of the arrays (committed-file size).

    PYTHONDONTWRITEBYTECODE=1 python tests/gen_det_metrics_golden.py
"""

import hashlib
import importlib.util
import io
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402

REF = G.REF
OUT = os.path.join(REPO, "tests", "golden", "det_metrics.npz")
FULL_ARRAYS_UP_TO = 4096

# (p_target, c_miss, c_fa): the reference's default first, then the other points of the cnsrc / SRE tables and two extreme priors
POINTS = [(0.01, 1, 1), (0.05, 1, 1), (0.001, 1, 1), (0.005, 10, 1), (0.5, 1, 5), (0.999, 1, 1), (0.001, 2.5, 0.75), (0.3, 1, 1)]


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_compute_min_dcf", os.path.join(REF, "kaldi", "sid", "compute_min_dcf.py"))
    dcf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dcf)
    text = open(os.path.join(REF, "computeCavg.py")).read()
    head = text[:text.index("if __name__ == '__main__':")]

    def plain_sum(values, start=0):
        for v in values:
            start = start + v
        return start
    ns = {"__name__": "ref_compute_cavg", "sum": plain_sum}
    exec(compile(head, "computeCavg.py", "exec"), ns)
    return dcf, ns["get_cavg"]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def dcf_case(dcf, out, name, scores, labels, points=POINTS):
    scores = np.asarray(scores, dtype=np.float32)
    labels = np.asarray(labels, dtype=np.int8)
    fnrs, fprs, thresholds = dcf.ComputeErrorRates([float(x) for x in scores], [int(x) for x in labels])
    res = [dcf.ComputeMinDcf(fnrs, fprs, thresholds, p, cm, cf) for p, cm, cf in points]
    fnr, fpr, thr = np.asarray(fnrs, dtype=np.float64), np.asarray(fprs, dtype=np.float64), np.asarray(thresholds, dtype=np.float64)
    assert np.array_equal(thr.astype(np.float32).astype(np.float64), thr)
    out["dcf/%s/scores" % name] = scores
    out["dcf/%s/labels" % name] = labels
    out["dcf/%s/points" % name] = np.asarray(points, dtype=np.float64)
    out["dcf/%s/min_dcf" % name] = np.asarray([r[0] for r in res], dtype=np.float64)
    out["dcf/%s/threshold" % name] = np.asarray([r[1] for r in res], dtype=np.float64)
    if len(scores) <= FULL_ARRAYS_UP_TO:
        out["dcf/%s/fnr" % name], out["dcf/%s/fpr" % name], out["dcf/%s/thresholds" % name] = fnr, fpr, thr.astype(np.float32)
    else:
        out["dcf/%s/sha256" % name] = np.asarray([digest(fnr), digest(fpr), digest(thr.astype(np.float32))])
    return fnrs, fprs, thresholds, res


def label_in_key_min_dcf(dcf, scores, labels, points):
    """What a sort by (score, label) - the EER kernel's key - would give: NOT the reference's order inside a tie group."""
    order = sorted(range(len(scores)), key=lambda i: (float(scores[i]), int(labels[i])))
    fnrs, fprs, thresholds = dcf.ComputeErrorRates([float(scores[i]) for i in order], [int(labels[i]) for i in order])
    return [dcf.ComputeMinDcf(fnrs, fprs, thresholds, p, cm, cf)[0] for p, cm, cf in points]


def cavg_case(get_cavg, out, name, model, true, scores, lang_num, bins=20, p_target=0.5):
    scores = np.asarray(scores, dtype=np.float32)
    model, true = np.asarray(model, dtype=np.int32), np.asarray(true, dtype=np.int32)
    pairs = [[int(m), int(t), float(s)] for m, t, s in zip(model, true, scores)]
    stats = [p[2] for p in pairs]
    cavgs, best = get_cavg(pairs, lang_num, min(stats), max(stats), bins, p_target)
    out["cavg/%s/scores" % name] = scores
    out["cavg/%s/model_lang" % name] = model.astype(np.int16)
    out["cavg/%s/true_lang" % name] = true.astype(np.int16)
    out["cavg/%s/params" % name] = np.asarray([lang_num, bins, p_target], dtype=np.float64)
    out["cavg/%s/cavgs" % name] = np.asarray(cavgs, dtype=np.float64)
    out["cavg/%s/min_cavg" % name] = np.float64(best)
    return cavgs, best


def matrix_pairs(rng, n_utts, lang_num, unknown_fraction=0.0, sep=1.5, quantum=None):
    """Every utterance scored against every language, row by row (the -matrix form)."""
    true = rng.integers(0, lang_num, n_utts)
    sc = rng.standard_normal((n_utts, lang_num))
    sc[np.arange(n_utts), true] += sep
    if quantum:
        sc = np.round(sc / quantum) * quantum
    known = rng.random(n_utts) >= unknown_fraction
    model = np.tile(np.arange(lang_num), n_utts)
    return model, np.repeat(np.where(known, true, -1), lang_num), sc.reshape(-1).astype(np.float32), np.repeat(known, lang_num)


def main():
    if not os.path.isdir(REF):
        sys.exit("gen_det_metrics_golden.py needs the reference tree at %s (build container only)" % REF)
    dcf, get_cavg = load_reference()
    rng = np.random.default_rng(20261017)
    out = {}

    def gauss(n_tgt, n_non):
        s = np.concatenate([rng.standard_normal(n_tgt) + 2.0, rng.standard_normal(n_non)]).astype(np.float32)
        l = np.concatenate([np.ones(n_tgt, dtype=np.int8), np.zeros(n_non, dtype=np.int8)])
        perm = rng.permutation(n_tgt + n_non)
        return s[perm], l[perm]

    dcf_case(dcf, out, "n2", [0.25, -0.5], [1, 0])
    dcf_case(dcf, out, "n2_inverted", [-0.5, 0.25], [1, 0])
    dcf_case(dcf, out, "n257", *gauss(40, 217))
    dcf_case(dcf, out, "gauss20000", *gauss(2000, 18000))
    # heavy ties: 64 distinct values, labels independent of position inside a tie group
    s, l = gauss(5000, 15000)
    s = (np.round(np.clip(s, -3.0, 4.875) * 8) / 8).astype(np.float32)
    assert len(np.unique(s)) == 64, len(np.unique(s))
    _, _, _, res = dcf_case(dcf, out, "ties64", s, l)
    other = label_in_key_min_dcf(dcf, s, l, POINTS)
    differs = [a[0] != b for a, b in zip(res, other)]
    assert any(differs), "the tie case does not tell a (score, label) sort from the reference's stable sort"
    out["dcf/ties64/label_in_key_min_dcf"] = np.asarray(other, dtype=np.float64)
    print("ties64: %d of %d operating points differ under a (score, label) sort" % (sum(differs), len(differs)))
    s, l = gauss(30, 70)
    dcf_case(dcf, out, "all_equal", np.full(100, 0.5, dtype=np.float32), l)
    # -0.0 and +0.0 are one tie group in input order; around it a few other values
    z = np.asarray([0.0, -0.0, 1.0, -0.0, 0.0, -1.0, 0.0, -0.0, -0.0, 0.0, 0.5, -0.0], dtype=np.float32)
    zl = np.asarray([1, 0, 1, 0, 0, 0, 1, 1, 0, 0, 1, 1], dtype=np.int8)
    fn, fp, th, _ = dcf_case(dcf, out, "signed_zeros", z, zl)
    assert [str(float(x)) for x in th[1:10]] == ["0.0", "-0.0", "-0.0", "0.0", "0.0", "-0.0", "-0.0", "0.0", "-0.0"]
    # every target below every non-target: the cost is lowest at the first sorted trial for p_target = 0.999, at the last for 0.001
    n_t, n_n = 300, 700
    s = np.concatenate([rng.random(n_t) - 2.0, rng.random(n_n) + 2.0]).astype(np.float32)
    l = np.concatenate([np.ones(n_t, dtype=np.int8), np.zeros(n_n, dtype=np.int8)])
    perm = rng.permutation(n_t + n_n)
    s, l = s[perm], l[perm]
    _, _, th, res = dcf_case(dcf, out, "ends", s, l, [(0.999, 1, 1), (0.001, 1, 1)])
    assert res[0][1] == th[0] == float(s.min()) and res[1][1] == th[-1] == float(s.max())

    # the command line: a scores file and a trials file (a superset, other order) as text, and the reference's stdout
    s, l = gauss(60, 340)
    names = [("spk%03d" % rng.integers(0, 40), "utt%04d" % i) for i in range(len(s))]
    score_txt = "".join("%s %s %.4f\n" % (a, b, x) for (a, b), x in zip(names, s))
    rows = ["%s %s %s\n" % (a, b, "target" if t else "nontarget") for (a, b), t in zip(names, l)] + ["spk999 utt9999 nontarget\n"]
    trials_txt = "".join(rows[i] for i in rng.permutation(len(rows)))
    parsed = [float(line.split()[2]) for line in score_txt.splitlines()]
    fn, fp, th = dcf.ComputeErrorRates(parsed, [int(x) for x in l])
    out["cli/dcf/scores_txt"], out["cli/dcf/trials_txt"] = np.asarray(score_txt), np.asarray(trials_txt)
    out["cli/dcf/args"] = np.asarray(["--p-target", "0.05", "--c-miss", "1", "--c-fa", "1"])
    out["cli/dcf/stdout"] = np.asarray("{0:.4f}\n".format(dcf.ComputeMinDcf(fn, fp, th, 0.05, 1.0, 1.0)[0]))
    out["cli/dcf/stdout_default"] = np.asarray("{0:.4f}\n".format(dcf.ComputeMinDcf(fn, fp, th, 0.01, 1, 1)[0]))

    # ---- Cavg
    m, t, s, _ = matrix_pairs(rng, 300, 2)
    cavg_case(get_cavg, out, "l2", m, t, s, 2)
    cavg_case(get_cavg, out, "l2_bins1", m, t, s, 2, bins=1)
    m, t, s, _ = matrix_pairs(rng, 2000, 10)
    cavg_case(get_cavg, out, "l10", m, t, s, 10)
    cavg_case(get_cavg, out, "l10_p03_bins7", m, t, s, 10, bins=7, p_target=0.3)
    # 10 % of the utterances of unknown language: folded into the last language's non-target slot - not the same as dropping them
    m, t, s, known = matrix_pairs(rng, 1000, 10, unknown_fraction=0.1)
    assert 0 < (~known).sum() < known.size
    a = cavg_case(get_cavg, out, "l10_unknown", m, t, s, 10)
    b = cavg_case(get_cavg, out, "l10_unknown_dropped", m[known], t[known], s[known], 10)
    assert a[1] != b[1] and float(s[known].min()) == float(s.min()) and float(s[known].max()) == float(s.max())
    # scores on a grid of 1/16 over a range of 5 with 20 bins: the thresholds are multiples of 1/4, many scores sit exactly on one
    m, t, s, _ = matrix_pairs(rng, 400, 5, unknown_fraction=0.05, quantum=0.0625)
    s = np.clip(s, -2.0, 3.0).astype(np.float32)
    assert float(s.min()) == -2.0 and float(s.max()) == 3.0 and np.isin(s, -2.0 + 0.25 * np.arange(21)).sum() > 100
    cavg_case(get_cavg, out, "on_threshold", m, t, s, 5)
    # 40 languages: more counters than a wavefront keeps in LDS
    m, t, s, _ = matrix_pairs(rng, 200, 40, unknown_fraction=0.05)
    cavg_case(get_cavg, out, "l40", m, t, s, 40)
    # a sparse pair list: languages without target pairs, (model, true) slots without pairs, the last language never a model
    m, t, s, _ = matrix_pairs(rng, 500, 6, unknown_fraction=0.2)
    keep = (rng.random(m.size) < 0.3) & (m != 5) & ~((m == 2) & (t == 2)) & ~((m == 0) & (t == 3))
    cavg_case(get_cavg, out, "sparse", m[keep], t[keep], s[keep], 6)

    # the command line: trials + pair-form scores + the same scores as a matrix; `Cavg <round(x, 4)>` as the reference prints it
    langs = ["zh-cn", "ct-cn", "id-id", "ja-jp"]                      # sorted: ct-cn id-id ja-jp zh-cn
    order = sorted(langs)
    n_utts = 120
    true = rng.integers(0, 4, n_utts)
    sc = rng.standard_normal((n_utts, 4))
    sc[np.arange(n_utts), true] += 1.5
    unknown = rng.random(n_utts) < 0.1
    utts = ["u%04d" % i for i in range(n_utts)]
    trials = io.StringIO()
    for i, u in enumerate(utts):
        for j, lang in enumerate(langs):
            if j == (i % 4) and i % 7 == 0 and j != true[i]:
                continue                                               # a scored pair the trials file does not list: dropped
            trials.write("%s %s %s\n" % (lang, u, "target" if (j == true[i] and not unknown[i]) else "nontarget"))
    listed = {tuple(line.split()[:2]) for line in trials.getvalue().splitlines()}
    pairs_txt = "".join("%s %s %.4f\n" % (lang, u, sc[i, j]) for i, u in enumerate(utts) for j, lang in enumerate(langs))
    matrix_txt = " ".join(langs) + "\n" + "".join("%s %s\n" % (u, " ".join("%.4f" % x for x in sc[i])) for i, u in enumerate(utts))
    pairs = [[order.index(lang), (order.index(langs[true[i]]) if not unknown[i] else -1), float("%.4f" % sc[i, j])]
             for i, u in enumerate(utts) for j, lang in enumerate(langs) if (lang, u) in listed]
    assert len(pairs) < n_utts * 4
    stats = [p[2] for p in pairs]
    _, best = get_cavg(pairs, 4, min(stats), max(stats), 20, 0.5)
    as_f32 = [[m, t, float(np.float32(x))] for m, t, x in pairs]           # what the device is given: the printed value must not hinge on it
    assert round(get_cavg(as_f32, 4, min(p[2] for p in as_f32), max(p[2] for p in as_f32), 20, 0.5)[1], 4) == round(best, 4)
    out["cli/cavg/trials_txt"], out["cli/cavg/pairs_txt"], out["cli/cavg/matrix_txt"] = np.asarray(trials.getvalue()), np.asarray(pairs_txt), np.asarray(matrix_txt)
    out["cli/cavg/stdout"] = np.asarray("Cavg %s\n" % round(best, 4))
    out["cli/cavg/lang_order"] = np.asarray(order)
    out["cli/cavg/model_lang"] = np.asarray([p[0] for p in pairs], dtype=np.int16)
    out["cli/cavg/true_lang"] = np.asarray([p[1] for p in pairs], dtype=np.int16)

    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print("%s: %d arrays, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
