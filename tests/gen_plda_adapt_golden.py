#!/usr/bin/env python3
"""Generate tests/golden/plda_domain_adapt.npz by running the REFERENCE's PLDA domain adaptors: the classes of
score/pyplda/ivector-adapt-plda-{coral,coralplus,cip,cip-reg,lip,lip-reg}.py, fed and scored by plda_base.py's own
PldaEstimation (10 iterations), PLDA.get_output(), transform_ivector and log_likelihood_ratio.  Build container only (needs
the reference tree, like oracle/gen_golden.py, whose shims this file uses).  (tests/golden/plda_adapt.npz is the fixture of
the Kaldi-style adaptor, written by oracle/gen_golden.py; this one stands beside it.)

The models travel between the reference's classes as they do between its scripts: through the 'mean' / 'within_var' /
'between_var' arks of PldaEstimation.plda_write (float64, lossless).  The adaptation vectors are float32, as they come out of
an ark, and are handed to add_stats as float64: fed float32, `np.matmul(ivector, ivector.T)` (ivector-adapt-plda-coral.py:38)
rounds every outer product to float32 before it is accumulated, an accident of numpy's type promotion that the float64
statistics of this project (and of Kaldi) do not share.  oracle/gen_golden.py feeds PldaUnsupervisedAdaptor the same way.

Next to the reference's outputs the file records, per adaptor, `spread_<adaptor>` and `spread_llr_<adaptor>`: max |delta| /
max |value| between the reference and a plain-numpy float64 restatement that symmetrises every eigh input (the reference does
not).  That spread is a property of the reference's arithmetic alone; the tests derive their tolerance from it.

    PYTHONDONTWRITEBYTECODE=1 python tests/gen_plda_adapt_golden.py
"""

import importlib.util
import os
import sys
import tempfile

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
os.environ.setdefault("PYTHONPYCACHEPREFIX", os.path.join(tempfile.gettempdir(), "gen_plda_adapt_pycache"))
sys.dont_write_bytecode = True
sys.pycache_prefix = os.environ["PYTHONPYCACHEPREFIX"]

import numpy as np  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402

NAME = "plda_domain_adapt"
ADAPTORS = ("coral", "coral_plus", "cip", "cip_reg", "lip", "lip_reg")
SCRIPTS = {"coral": "ivector-adapt-plda-coral.py", "coral_plus": "ivector-adapt-plda-coralplus.py", "cip": "ivector-adapt-plda-cip.py",
           "cip_reg": "ivector-adapt-plda-cip-reg.py", "lip": "ivector-adapt-plda-lip.py", "lip_reg": "ivector-adapt-plda-lip-reg.py"}
DIM, SEED, EM_ITERS = 24, 71, 10


def load_script(path, modname):
    """The file names carry hyphens: no import statement reaches them.  Their command line sits behind a __main__ guard."""
    spec = importlib.util.spec_from_file_location(modname, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def planted_sets(synth):
    """Out-of-domain: 60 speakers x 8.  In-domain (30 x 6 labelled, 400 unlabelled from 100 further speakers, 40 held out from
    10 more): the same kind of speaker structure seen through another channel - rotated, rescaled per axis and shifted."""
    r = np.random.RandomState(SEED)
    rot, _ = np.linalg.qr(r.standard_normal((DIM, DIM)))
    scale = np.linspace(0.5, 2.0, DIM)
    shift = 10.0 * r.standard_normal(DIM)     # embeddings far from centred: what an unadapted mean gets wrong

    def in_domain(n_spk, per_spk, seed):
        x, labels = synth.synth_speaker_embeddings(n_spk, per_spk, DIM, seed=seed, within=1.0, between=1.5)
        return ((x.astype(np.float64).dot(rot)) * scale + shift).astype(np.float32), labels
    out_x, out_l = synth.synth_speaker_embeddings(60, 8, DIM, seed=SEED + 1, within=1.0, between=1.5)
    in_x, in_l = in_domain(30, 6, SEED + 2)
    adapt, _ = in_domain(100, 4, SEED + 3)
    ev, ev_l = in_domain(10, 4, SEED + 4)
    ei, ti, tgt = synth.synth_trials(ev_l, 200, seed=SEED + 5)
    return dict(out_x=out_x, out_labels=out_l, in_x=in_x, in_labels=in_l, adapt=adapt, ev=ev, ev_labels=ev_l,
                trials_e=ei, trials_t=ti, trials_tgt=tgt)


def reference_em(PB, x, labels, path):
    stats = PB.PldaStats(DIM)
    for spk in np.unique(labels):
        stats.add_samples(1.0, x[labels == spk].astype(np.float64))
    assert stats.is_sorted()
    est = PB.PldaEstimation(stats)
    est.estimate(num_em_iters=EM_ITERS)
    est.plda_write(path)
    return np.asarray(est.mean).reshape(-1), np.array(est.within_var), np.array(est.between_var)


def reference_llr(PB, mean, within, between, ev, ei, ti):
    """PLDA.get_output() + transform_ivector + log_likelihood_ratio (plda_base.py:93-136, 186-214)."""
    plda = PB.PLDA()
    plda.mean, plda.within_var, plda.between_var = np.asarray(mean).reshape(-1, 1), within, between
    plda.get_output()
    plda.offset = np.asarray(plda.offset).reshape(-1)           # 1-D like the vectors (see oracle/gen_golden.py run_scoring_plda)
    tr = np.stack([plda.transform_ivector(v, 1) for v in ev.astype(np.float64)])
    return np.array([float(plda.log_likelihood_ratio(tr[a], 1, tr[b])) for a, b in zip(ei, ti)])


def reference_adaptors(mods, out_ark, in_ark, adapt):
    """-> {adaptor: (mean, within_var, between_var)}, every step the main() of the adaptor's script takes, minus the files."""
    def coral_of(mod, cls="CORAL"):
        c = getattr(mod, cls)()
        c.plda_read(out_ark)
        for v in adapt.astype(np.float64):
            c.add_stats(1, v)
        c.update_plda()
        return c
    res = {}
    c = coral_of(mods["coral"])
    res["coral"] = c
    res["coral_plus"] = coral_of(mods["coral_plus"], "CORALPlus")
    cip = mods["cip"].CIP()
    cip.interpolation(coral_of(mods["cip"]), in_ark)
    res["cip"] = cip
    cipreg = mods["cip_reg"].CIPReg()
    cipreg.plda_read(in_ark)
    cipreg.interpolation(coral_of(mods["cip_reg"]))
    res["cip_reg"] = cipreg
    lip = mods["lip"].LIP()
    lip.interpolation(out_ark, in_ark)
    res["lip"] = lip
    lipreg = mods["lip_reg"].LIPReg()
    lipreg.interpolation(out_ark, in_ark)
    res["lip_reg"] = lipreg
    return {k: (np.asarray(v.mean).reshape(-1), np.array(v.within_var), np.array(v.between_var)) for k, v in res.items()}


# ---- the restatement: float64 numpy, every eigh input symmetrised

def _sym(m):
    return 0.5 * (m + m.T)


def _coral(out, adapt):
    x = adapt.astype(np.float64)
    n = x.shape[0]
    mean = x.sum(0) / n
    var = x.T.dot(x) / n - np.outer(mean, mean)
    d = mean - out[0]
    var = var + 1.0 * np.outer(d, d)
    eo, qo = np.linalg.eigh(_sym(out[1] + out[2]))
    ei, qi = np.linalg.eigh(_sym(var))
    a = qi.dot(np.diag(np.sqrt(ei))).dot(qi.T).dot(qo.dot(np.diag(1.0 / np.sqrt(eo))).dot(qo.T))
    return mean, a.dot(out[1]).dot(a.T), a.dot(out[2]).dot(a.T)


def _reg(base, target, scale):
    s, q = np.linalg.eigh(_sym(base))
    t = np.diag(1.0 / np.sqrt(s)).dot(q.T)
    e, p = np.linalg.eigh(_sym(t.dot(target).dot(t.T)))
    b_inv = np.linalg.inv(q.dot(np.diag(1.0 / np.sqrt(s))).dot(p))
    return base + scale * b_inv.T.dot(np.maximum(0, np.diag(e) - np.eye(len(s)))).dot(b_inv)


def restated_adaptors(out, inn, adapt):
    m, sw, sb = _coral(out, adapt)
    return {"coral": (m, sw, sb),
            "coral_plus": (m, _reg(out[1], sw, 0.8), _reg(out[2], sb, 0.8)),
            "cip": (inn[0], 0.5 * sw + 0.5 * inn[1], 0.5 * sb + 0.5 * inn[2]),
            "cip_reg": (inn[0], _reg(inn[1], sw, 0.5), _reg(inn[2], sb, 0.5)),
            "lip": (inn[0], 0.4 * out[1] + 0.6 * inn[1], 0.4 * out[2] + 0.6 * inn[2]),
            "lip_reg": (inn[0], _reg(inn[1], out[1], 1 - 0.6), _reg(inn[2], out[2], 1 - 0.6))}


def restated_llr(mean, within, between, ev, ei, ti):
    """plda_base.py:93-136 and 186-214 for all trials at once (one example per side)."""
    t1 = np.linalg.inv(np.linalg.cholesky(within))
    psi, u = np.linalg.eigh(_sym(t1.dot(between).dot(t1.T)))
    y = (ev.astype(np.float64) - mean).dot(u.T.dot(t1).T)
    y = y * np.sqrt(len(mean) / (y * y / (psi + 1.0)).sum(1))[:, None]
    e, t = y[ei], y[ti]
    var_c, var_n = 1.0 + psi / (psi + 1.0), 1.0 + psi
    given = -0.5 * (np.log(var_c).sum() + ((t - psi / (psi + 1.0) * e) ** 2 / var_c).sum(1))
    without = -0.5 * (np.log(var_n).sum() + (t ** 2 / var_n).sum(1))
    return given - without


def main():
    if not os.path.isdir(G.REF):
        sys.exit("gen_plda_adapt_golden.py needs the reference tree at %s (build container only)" % G.REF)
    G.install_shims()                                              # scipye among them (plda_base.py:6)
    sys.path.insert(0, os.path.join(G.REF, "pytorch"))
    import libs.support.kaldi_io as ref_kaldi_io
    sys.modules["kaldi_io"] = ref_kaldi_io                         # plda_base.py imports a top-level kaldi_io
    if not hasattr(ref_kaldi_io, "read_vec"):
        ref_kaldi_io.read_vec = ref_kaldi_io.read_vec_flt_auto     # score/pyplda calls kaldi_io.read_vec
    pyplda = os.path.join(G.REF, "score", "pyplda")
    sys.path.insert(0, pyplda)
    import plda_base as PB
    PB.logger.setLevel("WARNING")
    mods = {k: load_script(os.path.join(pyplda, f), "ref_adapt_" + k) for k, f in SCRIPTS.items()}
    synth = G.load_synth()
    out = planted_sets(synth)
    ei, ti, tgt = out["trials_e"], out["trials_t"], out["trials_tgt"]
    with tempfile.TemporaryDirectory() as td:
        out_ark, in_ark = os.path.join(td, "plda_out"), os.path.join(td, "plda_in")
        out_model = reference_em(PB, out["out_x"], out["out_labels"], out_ark)
        in_model = reference_em(PB, out["in_x"], out["in_labels"], in_ark)
        ref = reference_adaptors(mods, out_ark, in_ark, out["adapt"])
    for tag, (m, w, b) in (("out", out_model), ("in", in_model)):
        out[tag + "_mean"], out[tag + "_within_var"], out[tag + "_between_var"] = m, w, b
    out["unadapted_llr"] = reference_llr(PB, *out_model, out["ev"], ei, ti)
    restated = restated_adaptors(out_model, in_model, out["adapt"])
    for k in ADAPTORS:
        m, w, b = ref[k]
        llr = reference_llr(PB, m, w, b, out["ev"], ei, ti)
        out[k + "_mean"], out[k + "_within_var"], out[k + "_between_var"], out[k + "_llr"] = m, w, b, llr
        rm, rw, rb = restated[k]
        spread = max(np.abs(rw - w).max() / np.abs(w).max(), np.abs(rb - b).max() / np.abs(b).max(), np.abs(rm - m).max() / np.abs(m).max())
        spread_llr = np.abs(restated_llr(rm, rw, rb, out["ev"], ei, ti) - llr).max() / np.abs(llr).max()
        out["spread_" + k], out["spread_llr_" + k] = np.float64(spread), np.float64(spread_llr)
        print("%-10s spread: covariances %.3g, LLR %.3g   (max |W| %.3g, max |B| %.3g, max |llr| %.3g)"
              % (k, spread, spread_llr, np.abs(w).max(), np.abs(b).max(), np.abs(llr).max()))
    # adaptation must matter on this data: the reference's own scores, the oracle's EER (computeEER-like-Bosaris.py semantics)
    from oracle import scoring_oracle as S
    for k in ("unadapted",) + ADAPTORS:
        out["eer_" + k] = np.float64(S.compute_eer(out[k + "_llr"], tgt)[0])
    print("EER (percent): " + ", ".join("%s %.2f" % (k, 100 * out["eer_" + k]) for k in ("unadapted",) + ADAPTORS))
    assert out["eer_coral"] < out["eer_unadapted"], "the planted shift does not make CORAL matter: change the shift"
    out.update(dim=np.int64(DIM), seed=np.int64(SEED), em_iters=np.int64(EM_ITERS))
    os.makedirs(G.GOLDEN, exist_ok=True)
    path = os.path.join(G.GOLDEN, NAME + ".npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
