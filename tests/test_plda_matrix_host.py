"""Host-side checks of the PLDA score matrices (no GPU): the expansion the device computes equals the reference's own all-pairs LLRs
(tests/golden/plda_matrix.npz, written by tests/gen_plda_matrix_golden.py from plda_base.py), and the new entry points are declared
by the header, bound by ctypes with the same argument lists and exported by the built library."""

import ctypes as C
import os
import re

import numpy as np

import helpers
import plda_matrix_cases as PM


def test_expansion_equals_the_reference_llr_matrices():
    g = np.load(helpers.GOLDEN + "/plda_matrix.npz")
    dim, psi, n = int(g["dim"]), g["psi"], g["num_utts"]
    assert psi.dtype == np.float32 and g["enroll_t"].dtype == np.float32 and set(n.tolist()) == {1, 2, 3, 4, 5}
    assert g["enroll_t"].shape == (23, dim) and g["test_t"].shape == (31, dim) and g["cohort_t"].shape == (41, dim)
    for tag, a, na, b in (("enroll_test", g["enroll_t"], n, g["test_t"]), ("enroll_cohort", g["enroll_t"], n, g["cohort_t"]),
                          ("test_cohort", g["test_t"], None, g["cohort_t"])):
        want = g["llr_" + tag]
        S, M = PM.llr_expansion(a, b, psi, na)
        bound = PM.llr_bound(want, M, dim, f32_roundings=0)                # float64 against float64: no f32 rounding anywhere
        assert (np.abs(S - want) <= bound).all(), (tag, float((np.abs(S - want) / bound).max()))
        # and the statement-order restatement the GPU tests use as their reference is the reference
        assert (np.abs(PM.llr_reference_order(a, b, psi, na) - want) <= bound).all(), tag
        assert not np.allclose(want[:20, :20], want[:20, :20].T)           # non-symmetric: a transposed fragment map cannot hide


def test_two_cov_restatement_equals_the_reference_matrix():
    g = np.load(helpers.GOLDEN + "/plda_matrix.npz")
    mean, within, between = g["mean"], g["within_var"] + 5e-5 * np.eye(int(g["dim"])), g["between_var"]
    tot_inv, w2b_inv, w_inv = np.linalg.inv(between + within), np.linalg.inv(within + 2 * between), np.linalg.inv(within)
    gamma, lam, c = (-1 / 4) * (w2b_inv + w_inv) + (1 / 2) * tot_inv, (-1 / 4) * (w2b_inv - w_inv), (w2b_inv - tot_inv).dot(mean)
    S, M = PM.two_cov_matrix(g["enroll_raw"], g["test_raw"], gamma, lam, c)
    assert (np.abs(S - g["two_cov"]) <= PM.two_cov_bound(M, int(g["dim"]))).all()


def test_new_entry_points_are_declared_bound_and_exported(repo_root):
    from libs.amd import capi
    hdr = open(os.path.join(repo_root, "include", "asv_amd.h")).read()
    ctype_of = {"const float *": C.c_void_p, "float *": C.c_void_p, "const int32_t *": C.c_void_p, "double *": C.c_void_p, "void *": C.c_void_p,
                "int": C.c_int, "const double *": C.POINTER(C.c_double)}
    lib = capi.lib()
    for name in ("asv_plda_llr_matrix", "asv_two_cov_matrix"):
        assert name in capi.SYMBOLS
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, "%s is not declared in include/asv_amd.h" % name
        params = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
        types = [re.sub(r"\s*\w+$", "", a) if not a.endswith("*") else a for a in params]            # drop the parameter name
        fn = getattr(lib, name)                                            # AttributeError = the library does not export it
        assert fn.restype is C.c_int
        assert [ctype_of[t] for t in types] == list(fn.argtypes), (name, types)
    # `scores` of the two-covariance matrix and its host model arrays: device pointer vs host float64 pointers, as in asv_two_cov_trials
    assert lib.asv_two_cov_matrix.argtypes[5:8] == lib.asv_two_cov_trials.argtypes[5:8]


def test_score_matrix_kernel_resources(tmp_path):
    """Build-time properties score_matrix_kernel<float | double> is designed around (kernels_score_matrix.hip): 16 accumulators of 4 f64 and
    a register-prefetched K chunk inside 256 registers with no scratch = two waves per SIMD, 2 x 72 KiB of LDS = two workgroups per CU,
    and the K chunk's 4 x 16 f64 matrix instructions."""
    import pytest
    from test_kernel_resources import HIPCC, device_asm
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path / "score_matrix.s"
    blocks = [b for b in re.split(r"remark: [^\n]*Function Name: ", device_asm("kernels_score_matrix", out))[1:] if "score_matrix_kernel" in b.split()[0]]
    assert len(blocks) == 2
    for b in blocks:
        name = b.split()[0]
        get = lambda pat: int(re.search(pat, b).group(1))
        assert get(r"VGPRs Spill: (\d+)") == 0 and get(r"ScratchSize \[bytes/lane\]: (\d+)") == 0, name
        assert get(r" VGPRs: (\d+)") + get(r"AGPRs: (\d+)") <= 256 and get(r"Occupancy \[waves/SIMD\]: (\d+)") == 2, name
        assert get(r"LDS Size \[bytes/block\]: (\d+)") == 2 * 2 * 16 * 144 * 8, name
    assert sum("v_mfma_f64_16x16x4_f64" in line.split(";")[0] for line in out.read_text().splitlines()) == 2 * 64
