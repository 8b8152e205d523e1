"""The persistent 8-phase TDNN GEMM (kernels_tdnn_p8.hip, tdnn_gemm_p8p_kernel) on the 16x16x32 matrix instruction: same wave tile, same
LDS image, 8 x 4 accumulators of 4 registers; a lane now holds one frame of a 16-frame fragment and 4 channels of a 16-channel fragment.
The output must stay bit-identical to the variant-3 kernel's (same products into each accumulator in ascending k).  What the existing
cases (tests/test_gpu_kernels.py, forced onto small batches) never reach: a workgroup that walks more than one tile (the persistent
loop's has_next path: the next tile's first K-tile requested in front of the epilogue, the epilogue's scratch in buffer 1), and utterance
seams on every row residue modulo 16 (the validity bit of a lane is now bit (f & 1) * 16 + lane % 16 of its fragment's word)."""

import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
from helpers import rel_err
from test_gpu_kernels import MODE_TOL, _mode_args, _oracle_layer, _tdnn_forward
from test_gpu_chain_mfma_shape import LENS

pytestmark = pytest.mark.gpu

DEVLIB = os.path.join(helpers.REPO, "asv-subtools_amd", "libasv_amd_dev.so")
GAP = 4                      # rows between utterances in the frame domain


def _layer(cin, cout, ctx, lens, seed):
    r = np.random.RandomState(seed)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    x = r.randn(int(offsets[-1]), cin).astype(np.float32)
    left, right = min(0, ctx[0]), max(0, ctx[-1])
    w = (r.randn(cout, cin, right - left + 1) / np.sqrt(cin * len(ctx))).astype(np.float32)
    b = (0.1 * r.randn(cout)).astype(np.float32)
    scale = r.uniform(0.5, 1.5, cout).astype(np.float32)
    shift = (0.2 * r.randn(cout)).astype(np.float32)
    return x, offsets, w, b, scale, shift


def _cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _utts_for_tiles(tiles, n_tiles, frames):
    """fewest utterances of `frames` frames whose frame domain (GAP rows in front of, between and behind them, padded to 256 rows)
    holds at least `tiles` tiles of 256 x 256 at `n_tiles` channel tiles"""
    n = 1
    while -(-(GAP + n * (frames + GAP)) // 256) * n_tiles < tiles:
        n += 1
    return n


MULTI_TILE_CASES = [(64, 512, [0]), (128, 512, [-2, 2])]
_oracle_cache = {}


def _multi_tile_case(case):
    """layer, inputs and f64 oracle of a case: built once, shared by the element types"""
    if case not in _oracle_cache:
        cin, cout, ctx = MULTI_TILE_CASES[case]
        lens = [300] * _utts_for_tiles(_cu_count() + 2, cout // 256, 300)
        x, offsets, w, b, scale, shift = _layer(cin, cout, ctx, lens, 7 * cin + cout)
        _oracle_cache[case] = (x, offsets, w, b, scale, shift, _oracle_layer(x, offsets, w, b, ctx, "relu", scale, shift, False))
    return _oracle_cache[case]


@pytest.mark.parametrize("case", range(len(MULTI_TILE_CASES)), ids=lambda c: "%dx%d_ctx%s" % (MULTI_TILE_CASES[c][0], MULTI_TILE_CASES[c][1], "_".join(map(str, MULTI_TILE_CASES[c][2]))))
@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_more_than_one_tile_per_workgroup(case, mode, monkeypatch):
    """CU count + 2 tiles of 256 x 256: the production rule (ASV_AMD_P8=1) takes the layer, and two workgroups walk a second tile.  Bit
    for bit the variant-3 kernel's output (ASV_AMD_P8=0), and the f64 oracle at the mode's tolerance."""
    from libs.amd import capi
    L = capi.lib()
    cin, cout, ctx = MULTI_TILE_CASES[case]
    x, offsets, w, b, scale, shift, want = _multi_tile_case(case)
    prec, flags = _mode_args(mode + "_mfma")
    monkeypatch.setenv("ASV_AMD_LIVE_TUNE", "1")
    monkeypatch.setenv("ASV_AMD_P8", "1")
    n0, m0 = L.asv_kernel_launch_count(capi.KERNEL_TDNN_P8), L.asv_kernel_launch_count(capi.KERNEL_TDNN_BIG3)
    got = _tdnn_forward(x, offsets, w, b, ctx, "relu", scale, shift, False, prec, flags)
    assert (L.asv_kernel_launch_count(capi.KERNEL_TDNN_P8), L.asv_kernel_launch_count(capi.KERNEL_TDNN_BIG3)) == (n0 + 1, m0), "the 8-phase kernel did not take this layer"
    monkeypatch.setenv("ASV_AMD_P8", "0")
    ref = _tdnn_forward(x, offsets, w, b, ctx, "relu", scale, shift, False, prec, flags)
    assert (L.asv_kernel_launch_count(capi.KERNEL_TDNN_P8), L.asv_kernel_launch_count(capi.KERNEL_TDNN_BIG3)) == (n0 + 1, m0 + 1)
    assert np.array_equal(got, ref), "8-phase kernel and variant-3 kernel differ in %d values" % int((got != ref).sum())
    e = rel_err(got, want)
    print("p8 mfma shape, %d tiles, %s: rel err vs oracle %.3e" % (-(-(GAP + (len(offsets) - 1) * 304) // 256) * (cout // 256), mode, e))
    assert e < MODE_TOL[mode]


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_seams_at_16_frame_granularity(mode, monkeypatch):
    """An utterance start and an utterance end on every row residue modulo 16 (the length list of tests/test_gpu_chain_mfma_shape.py):
    the 80-channel first layer on the variant-3 kernel against the oracle, and a 64-channel twin on the 8-phase kernel (forced from two
    tiles on) bit for bit against the variant-3 kernel and against the oracle.  (The C ABI returns the utterances' rows only: a gap row
    that was not zeroed would show in the neighbouring rows of the next layer, not here.)"""
    from libs.amd import capi
    L = capi.lib()
    ctx = [-2, -1, 0, 1, 2]
    prec, flags = _mode_args(mode + "_mfma")
    monkeypatch.setenv("ASV_AMD_LIVE_TUNE", "1")
    monkeypatch.setenv("ASV_AMD_P8", "2")
    x, offsets, w, b, scale, shift = _layer(80, 512, ctx, LENS, 80)
    m0 = L.asv_kernel_launch_count(capi.KERNEL_TDNN_BIG3)
    got = _tdnn_forward(x, offsets, w, b, ctx, "relu", scale, shift, False, prec, flags)
    assert L.asv_kernel_launch_count(capi.KERNEL_TDNN_BIG3) == m0 + 1
    assert rel_err(got, _oracle_layer(x, offsets, w, b, ctx, "relu", scale, shift, False)) < MODE_TOL[mode]
    x, offsets, w, b, scale, shift = _layer(64, 512, ctx, LENS, 64)
    n0 = L.asv_kernel_launch_count(capi.KERNEL_TDNN_P8)
    got = _tdnn_forward(x, offsets, w, b, ctx, "relu", scale, shift, False, prec, flags)
    assert L.asv_kernel_launch_count(capi.KERNEL_TDNN_P8) == n0 + 1, "the 8-phase kernel did not take the twin"
    monkeypatch.setenv("ASV_AMD_P8", "0")
    ref = _tdnn_forward(x, offsets, w, b, ctx, "relu", scale, shift, False, prec, flags)
    assert L.asv_kernel_launch_count(capi.KERNEL_TDNN_P8) == n0 + 1 and L.asv_kernel_launch_count(capi.KERNEL_TDNN_BIG3) == m0 + 2
    assert np.array_equal(got, ref), "8-phase kernel and variant-3 kernel differ in %d values" % int((got != ref).sum())
    assert rel_err(got, _oracle_layer(x, offsets, w, b, ctx, "relu", scale, shift, False)) < MODE_TOL[mode]


DEV_CODE = r'''
import os, sys, numpy as np
sys.path[:0] = [%r, %r, %r]
from libs.amd import capi
from test_gpu_kernels import _mode_args, _tdnn_forward
from test_gpu_gemm_mfma_shape import _layer
L = capi.lib()
os.environ["ASV_AMD_P8"] = "2"
out = {}
for name, (cin, cout, ctx, lens) in {"taps3": (192, 320, [-2, 0, 2], [77, 256, 1, 255, 300]), "tap1": (128, 512, [0], [300, 9, 8, 500])}.items():
    x, offsets, w, b, scale, shift = _layer(cin, cout, ctx, lens, cin + cout)
    for mode in ("bf16", "f16"):
        prec, flags = _mode_args(mode + "_mfma")
        for shape in ("0", "1"):
            os.environ["ASV_AMD_P8_MFMA"] = shape
            n0 = L.asv_kernel_launch_count(capi.KERNEL_TDNN_P8)
            out["%%s_%%s_%%s" %% (name, mode, shape)] = _tdnn_forward(x, offsets, w, b, ctx, "relu", scale, shift, False, prec, flags)
            assert L.asv_kernel_launch_count(capi.KERNEL_TDNN_P8) == n0 + 1, (name, mode, shape)
np.savez(sys.argv[1], **out)
''' % (helpers.REPO, os.path.join(helpers.REPO, "asv-subtools_amd", "pytorch"), os.path.join(helpers.REPO, "tests"))


@pytest.mark.skipif(not os.path.exists(DEVLIB), reason="developer library not built (make -C asv-subtools_amd/csrc dev)")
def test_both_shapes_in_the_developer_build(tmp_path):
    """ASV_AMD_P8_MFMA (developer build only, read at every launch under ASV_AMD_LIVE_TUNE): 0 = 32x32x16, 1 = 16x16x32 in the persistent
    8-phase kernel.  Equal bits on a three-tap and a one-tap layer in both element types; the child asserts on the launch counter that
    the 8-phase kernel ran each time."""
    path = str(tmp_path / "dev.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("ASV_AMD_P8", "ASV_AMD_P8_MFMA")}
    env.update(ASV_AMD_LIB=DEVLIB, ASV_AMD_LIVE_TUNE="1")
    r = subprocess.run([sys.executable, "-c", DEV_CODE, path], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = dict(np.load(path))
    for name in ("taps3", "tap1"):
        for mode in ("bf16", "f16"):
            wide, narrow = res["%s_%s_0" % (name, mode)], res["%s_%s_1" % (name, mode)]
            assert np.isfinite(wide).all() and np.abs(wide).max() > 0
            assert np.array_equal(wide, narrow), (name, mode, int((wide != narrow).sum()))
