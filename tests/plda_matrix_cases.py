"""Shared by tests/test_gpu_plda_matrix.py, tests/test_plda_matrix_host.py and tests/gen_plda_matrix_golden.py: float64 numpy
restatements of the all-pairs PLDA scores and the error bounds the tests hold the device to.

The Kaldi-style LLR of score/pyplda/plda_base.py:109-136, for an enrolment vector e with n utterances and a test vector t:
    c_d = n psi_d / (n psi_d + 1)      v_d = 1 + psi_d / (n psi_d + 1)      m_d = c_d e_d
    LLR = -0.5 (sum log v_d + sum (t_d - m_d)^2 / v_d) + 0.5 (sum log(1 + psi_d) + sum t_d^2 / (1 + psi_d))
`llr_reference_order` evaluates exactly these statements; `llr_expansion` expands the squares into
    LLR = sum_d [ (m_d / v_d) t_d + (0.5 / (1 + psi_d) - 0.5 / v_d) t_d^2 ] - 0.5 sum (log v_d + m_d^2 / v_d) + 0.5 sum log(1 + psi_d)
= <A_i, B_j> + row_i, the form the device computes."""

import numpy as np

F32_EPS = 2.0 ** -24          # one rounding to f32
F64_EPS = 2.0 ** -52

# (E, T, dim): one element; K = 6 (no multiple of 4) with ragged edges; one past / one short of a 64-wide fragment group; several
# 128-tiles in both directions with several K chunks; the largest K
LLR_SHAPES = [(1, 1, 4), (17, 5, 3), (65, 63, 24), (130, 257, 150), (64, 128, 512)]
TWO_COV_SHAPES = [s for s in LLR_SHAPES if s[2] <= 150]


def make_llr_case(E, T, dim, seed, mixed_n):
    """Random, non-symmetric f32 inputs: enrol / test vectors of the size length-normalised PLDA vectors have (|x|^2 ~ dim), psi
    between 0.2 and 12, num_utts from {1, 3, 7} or None."""
    r = np.random.RandomState(seed)
    psi = np.exp(r.uniform(-1.5, 2.5, dim)).astype(np.float32)
    enroll = (r.standard_normal((E, dim)) * np.sqrt(psi / (1.0 + psi)) + 0.3).astype(np.float32)
    test = (r.standard_normal((T, dim)) * 1.1 - 0.2).astype(np.float32)
    n = r.choice(np.array([1, 3, 7], dtype=np.int32), size=E).astype(np.int32) if mixed_n else None
    return enroll, test, psi, n


def llr_reference_order(enroll, test, psi, num_utts=None):
    """plda_base.py:109-136 statement by statement in float64, all pairs: [E, T]."""
    e, t, psi = (np.asarray(a, dtype=np.float64) for a in (enroll, test, psi))
    n = np.ones(e.shape[0]) if num_utts is None else np.asarray(num_utts, dtype=np.float64)
    out = np.empty((e.shape[0], t.shape[0]))
    var0 = psi + 1.0
    without = -0.5 * (np.sum(np.log(var0)) + (t ** 2.0).dot(np.reciprocal(var0)))                  # [T]
    for i in range(e.shape[0]):
        mean = n[i] * psi / (n[i] * psi + 1.0) * e[i]
        var = 1.0 + psi / (n[i] * psi + 1.0)
        given = -0.5 * (np.sum(np.log(var)) + ((t - mean) ** 2.0).dot(np.reciprocal(var)))
        out[i] = given - without
    return out


def llr_expansion(enroll, test, psi, num_utts=None):
    """-> (S [E, T] = A B^T + row, M [E, T] = |A| |B|^T + |row|), float64."""
    e, t, psi = (np.asarray(a, dtype=np.float64) for a in (enroll, test, psi))
    n = (np.ones(e.shape[0]) if num_utts is None else np.asarray(num_utts, dtype=np.float64))[:, None]
    den = n * psi + 1.0
    mean = n * psi / den * e
    var = 1.0 + psi / den
    A = np.concatenate([mean / var, 0.5 / (1.0 + psi) - 0.5 / var], axis=1)
    B = np.concatenate([t, t * t], axis=1)
    row = -0.5 * np.sum(np.log(var) + mean * mean / var, axis=1) + 0.5 * np.sum(np.log(1.0 + psi))
    return A.dot(B.T) + row[:, None], np.abs(A).dot(np.abs(B).T) + np.abs(row)[:, None]


def llr_bound(want, M, dim, f32_roundings=1):
    """Per element: f32_roundings * 2^-24 |want| for the f32 roundings of the output(s) + 4 (2 dim + 16) 2^-52 M: the float64
    summation bound of a K = 2 dim product plus the row term, in either order, times 4 for the roundings of the preparation."""
    return f32_roundings * F32_EPS * np.abs(want) + 4.0 * (2 * dim + 16) * F64_EPS * M


def make_two_cov_case(E, T, dim, seed):
    """Non-symmetric random f32 vectors and a two-covariance model from random SPD covariances: (enroll, test, mean, within, between)."""
    r = np.random.RandomState(seed)
    a, b = r.standard_normal((dim, dim + 8)), r.standard_normal((dim, dim + 8))
    within = a.dot(a.T) / (dim + 8) + 0.1 * np.eye(dim)
    between = 0.7 * b.dot(b.T) / (dim + 8) + 0.05 * np.eye(dim)
    mean = 0.5 * r.standard_normal(dim)
    enroll = (r.standard_normal((E, dim)) + 0.4).astype(np.float32)
    test = (1.3 * r.standard_normal((T, dim)) - 0.1).astype(np.float32)
    return enroll, test, mean, within, between


def two_cov_matrix(enroll, test, gamma, lam, c):
    """gaussian-plda-scoring.py:23-29 (k = 0) for all pairs -> (S [E, T], M' [E, T] = the sum of the absolute terms, the two-stage
    products taken as |x| |L| |y|)."""
    e, t = np.asarray(enroll, dtype=np.float64), np.asarray(test, dtype=np.float64)
    S = e.dot(lam).dot(t.T) + t.dot(lam).dot(e.T).T + np.sum(e.dot(gamma) * e, axis=1)[:, None] + np.sum(t.dot(gamma) * t, axis=1)[None, :] \
        + e.dot(c)[:, None] + t.dot(c)[None, :]
    ae, at, al, ag, ac = np.abs(e), np.abs(t), np.abs(lam), np.abs(gamma), np.abs(c)
    M = ae.dot(al).dot(at.T) + at.dot(al).dot(ae.T).T + np.sum(ae.dot(ag) * ae, axis=1)[:, None] + np.sum(at.dot(ag) * at, axis=1)[None, :] \
        + ae.dot(ac)[:, None] + at.dot(ac)[None, :]
    return S, M


def two_cov_bound(M, dim):
    return 4.0 * (2 * dim + 16) * F64_EPS * M
