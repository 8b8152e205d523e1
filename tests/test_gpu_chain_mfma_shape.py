"""The chain kernel (kernels_tdnn_chain.hip) on the 16x16x32 matrix instruction: a lane group now holds 4 frames of a 16-frame fragment, the
pooling epilogue walks 16-frame fragments and merges lane groups l and l ^ 32 about a common pivot before it publishes a half.  What can
go wrong lies at 16-frame granularity, so the batch is built to put an utterance start and an utterance end on every row residue modulo 16:
lane groups without a frame of an utterance in its first fragment, several runs per fragment, 1-frame utterances, gap rows at every
position.  ASV_AMD_CHAIN_TAIL is read once per process: every setting runs in a child process, once per module."""

import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
from helpers import rel_err

pytestmark = pytest.mark.gpu

LENS = [7, 17, 15, 9, 10, 2, 3, 2, 1, 13, 11, 6, 5, 5, 17, 17, 13, 7, 17, 11, 5, 17, 1, 11]
GAP = 4                      # rows between utterances in the frame domain (kHalo)
REPEAT = 55                  # 55 x 322 rows: less than one round of 128-frame tiles, more than one of 64-frame tiles -> the 96-frame form
DEVLIB = os.path.join(helpers.REPO, "asv-subtools_amd", "libasv_amd_dev.so")

# Largest per-utterance error against the exact-f32 extraction of the same engine, measured ONCE on the parent commit's library
# (fd4c6ea, the 32x32x16 kernel) with this file's batches: (precision, frames per tile) -> e_parent.  The new kernel is another 16-bit
# evaluation of the same function: e_new < 1.3 e_parent + 1e-4 (the rule of test_layer_chain_kernel_matches_per_layer_kernels).
E_PARENT = {
    ("bf16", 64): 2.8265e-03, ("bf16", 128): 2.8265e-03, ("bf16", 96): 2.8265e-03,
    ("f16", 64): 3.3254e-04, ("f16", 128): 3.3254e-04, ("f16", 96): 3.3440e-04,
}

CODE = r'''
import os, sys, numpy as np
sys.path[:0] = [%r, %r, %r]
import helpers
from libs.amd import synth
lens, repeat = %r, %r
what = sys.argv[2].split(",")
g, sd, model = helpers.golden_model("xvector_near_ragged")
model.cuda()
mats = [synth.synth_feats(t, 80, 6100 + i) for i, t in enumerate(lens)]
scaled = [(m * 1.0e5).astype(np.float32) if i %% 3 == 0 else m for i, m in enumerate(mats)]
def run(ms):
    return model._amd_engine()._extract_batch(list(ms)).numpy()
out = {}
for prec in ("bf16", "f16"):
    model.amd_precision = prec
    if "dev" in what:                                  # the developer library: the switch is read at every launch
        for m in ("0", "1", "2", "3"):
            os.environ["ASV_AMD_CHAIN_MFMA"] = m
            out[prec + "_mfma" + m] = run(mats)
        continue
    out[prec] = run(mats)
    if "big" in what:
        out[prec + "_big"] = run(mats * repeat)
    out[prec + "_nb"] = run(scaled)
    out[prec + "_alone"] = np.stack([run([m])[0] for i, m in enumerate(mats) if i %% 3])
if "ref" in what:
    model.amd_precision = "f32"
    out["f32"] = run(mats)
    from oracle import np_oracle as O
    out["oracle_nb"] = np.stack([O.extract_embedding(lambda c: O.xvector_embed(c, sd, "near"), m) for m in scaled])
np.savez(sys.argv[1], **out)
''' % (helpers.REPO, os.path.join(helpers.REPO, "asv-subtools_amd", "pytorch"), os.path.join(helpers.REPO, "tests"), LENS, REPEAT)


def run_child(path, what, **env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ("ASV_AMD_CHAIN_TAIL", "ASV_AMD_CHAIN_MFMA")}
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", CODE, path, what], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return dict(np.load(path))


def run_forms(tmp_dir, **env_extra):
    """Both settings, each in its own process: {"auto": 64-frame tiles for the list, 96-frame tiles for its 55 repeats; "t128": 128-frame tiles}."""
    return {"auto": run_child(os.path.join(str(tmp_dir), "auto.npz"), "ref,big", **env_extra),
            "t128": run_child(os.path.join(str(tmp_dir), "t128.npz"), "small", ASV_AMD_CHAIN_TAIL="0", **env_extra)}


def worst(got, ref):
    """largest per-utterance error of a batch whose utterance k is utterance k modulo len(ref) of the reference batch"""
    return max(rel_err(got[k], ref[k % len(ref)]) for k in range(len(got)))


def errors_vs_f32(res):
    ref = res["auto"]["f32"]
    return {(prec, form): worst(res[key][name], ref)
            for prec in ("bf16", "f16") for form, key, name in ((64, "auto", prec), (128, "t128", prec), (96, "auto", prec + "_big"))}


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    return run_forms(tmp_path_factory.mktemp("chain_mfma_shape"))


def test_length_list_puts_a_seam_on_every_residue():
    row, starts, ends = GAP, set(), set()
    for t in LENS:
        starts.add(row % 16)
        ends.add((row + t - 1) % 16)
        row += t + GAP
    assert row == 322
    assert starts == set(range(16)) and ends == set(range(16))


def test_seams_at_16_frame_granularity(forms):
    e = errors_vs_f32(forms)
    for key in sorted(e):
        print("chain mfma shape: %s, %d-frame tiles: e_new %.3e, e_parent %.3e" % (key[0], key[1], e[key], E_PARENT[key]))
    for prec in ("bf16", "f16"):
        small, t128, big = forms["auto"][prec], forms["t128"][prec], forms["auto"][prec + "_big"]
        assert small.shape == (len(LENS), 512) and big.shape == (len(LENS) * REPEAT, 512)
        assert np.isfinite(small).all() and np.isfinite(t128).all() and np.isfinite(big).all()
        for form in (64, 128, 96):
            assert e[(prec, form)] < 1.3 * E_PARENT[(prec, form)] + 1e-4, (prec, form, e[(prec, form)], E_PARENT[(prec, form)])
        # the tile forms against each other: same products per row, other merge order of the moments
        assert rel_err(small, t128) < 2e-5, (prec, rel_err(small, t128))
        assert worst(big, t128) < 2e-5, (prec, worst(big, t128))
        assert not np.array_equal(small, t128) and not np.array_equal(big[:len(LENS)], t128)     # the other forms did run


def test_neighbours_scaled_by_1e5(forms):
    """Every third utterance scaled by 1e5: an utterance's partials are built from its own frames only, about a pivot of its own.  Every
    unscaled utterance against its own extraction alone; every utterance against the oracle (bf16 2e-2, the tolerances of
    test_pooled_moments_ignore_the_neighbour); in f16 the scaled utterances leave the half range and are not compared."""
    want = forms["auto"]["oracle_nb"]
    plain = [i for i in range(len(LENS)) if i % 3]
    for key in ("auto", "t128"):
        for prec in ("bf16", "f16"):
            got, alone = forms[key][prec + "_nb"], forms[key][prec + "_alone"]
            for j, i in enumerate(plain):
                assert rel_err(got[i], alone[j]) < 2e-2, (key, prec, i, rel_err(got[i], alone[j]))
            for i in (range(len(LENS)) if prec == "bf16" else plain):
                assert rel_err(got[i], want[i]) < 2e-2, (key, prec, i, rel_err(got[i], want[i]))


@pytest.mark.skipif(not os.path.exists(DEVLIB), reason="developer library not built (make -C asv-subtools_amd/csrc dev)")
def test_both_shapes_in_the_developer_build(tmp_path):
    """ASV_AMD_CHAIN_MFMA (developer build only): bit 0 = the Y-writing phases, bit 1 = the last layer on the 16x16x32 shape.  Narrow (3)
    against wide (0): same moments, other summation order (the bound of devlib_cases.py); not bit-equal: the other kernel did run.  The
    single-phase settings meet the same bound.  (Measured: the Y-writing phases alone are bit-identical on both shapes - one 16x16x32
    instruction sums its 32 products in the order of two 32x32x16 - so only the last layer's pooling order shows in the output.)"""
    res = run_child(str(tmp_path / "dev.npz"), "dev", ASV_AMD_LIB=DEVLIB, ASV_AMD_LIVE_TUNE="1")
    for prec in ("bf16", "f16"):
        wide, narrow = res[prec + "_mfma0"], res[prec + "_mfma3"]
        assert np.isfinite(wide).all() and np.isfinite(narrow).all()
        assert not np.array_equal(narrow, wide), prec
        for m in ("1", "2", "3"):
            assert rel_err(res[prec + "_mfma" + m], wide) < 1e-4, (prec, m, rel_err(res[prec + "_mfma" + m], wide))
