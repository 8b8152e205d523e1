"""The 16-bit grid convolution kernels of kernels_conv2d.hip alone, per element type, against float64.

A case (tests/conv_cases.py) is  grid_input -> [head] -> ONE layer -> per-bin pooling: the layer under test runs on exactly one of
grid_conv_c1_kernel, grid_conv_narrow_kernel, grid_conv_narrow_pers_kernel, grid_conv_wide_kernel, grid_conv_s2d_kernel (bf16 and
IEEE-half instantiations, fast and GENERIC epilogues; c1 also f32), or - one bin beyond the wide kernel's halo - on whatever tile
takes it.  Exact family: no f32 operation on the device can round, so device and reference differ by the pooling's arithmetic
alone: 1e-5, mean block and std block separately.  Rounded family (tanh, sigmoid, the SE form): the calibrated bound of
conv_cases.TOL_ROUNDED.  Every case prints its measured error ("[conv] case ...").

Which kernel ran: asv_kernel_launch_count moves by one for the kernel the case names (and for grid_conv_c1_kernel where it is the
head layer of a 32- / 64-channel case) and not at all for the others.

Environment switches: ASV_AMD_CONV_PERS and ASV_AMD_CONV_PERS_WGS are read per launch only under ASV_AMD_LIVE_TUNE, which is latched
at a process's first launch - so this process runs the narrow layers on the default (persistent) form, and ONE fresh child process
started with ASV_AMD_LIVE_TUNE=1 runs them on the one-tile form and walks the capped launches of the persistent ring (`pers_child`).
"""

import os
import subprocess
import sys

import numpy as np
import pytest

import conv_cases as CC

pytestmark = pytest.mark.gpu

COUNTERS = ("CONV_C1", "CONV_NARROW", "CONV_NARROW_PERS", "CONV_WIDE", "CONV_S2D")
H16 = ("bf16", "f16")


def _counts():
    from libs.amd import capi
    L = capi.lib()
    return np.array([L.asv_kernel_launch_count(getattr(capi, "KERNEL_" + n)) for n in COUNTERS], dtype=np.int64)


def _expected_launches(case, narrow_form="CONV_NARROW_PERS"):
    """launches per extraction: the kernel under test, and grid_conv_c1_kernel as the head of a 32- / 64-channel case"""
    want = dict.fromkeys(COUNTERS, 0)
    if case.kernel != "c1" and case.cin <= 64:
        want["CONV_C1"] += 1
    name = {"c1": "CONV_C1", "narrow": narrow_form, "wide": "CONV_WIDE", "s2d": "CONV_S2D", "fallback": None}[case.kernel]
    if name:
        want[name] += 1
    return np.array([want[n] for n in COUNTERS], dtype=np.int64)


def _expected_ops(case):
    head = [] if case.kernel == "c1" else ["tdnn"]
    return ["grid_input"] + head + (["pool", "tdnn"] if case.form == "se" else []) + ["tdnn", "pool"]


def _extract(case, et, batches=None):
    """One Engine for the case; its batch (or every batch of `batches`) extracted; status 0; the launch counters moved by what the
    case names, once per extraction; closed."""
    from libs.amd import engine
    graph, feats = CC.build(case, et)
    eng = engine.Engine(graph, precision=et)
    try:
        assert [op.kind for op in eng.ops] == _expected_ops(case)
        outs = []
        for f in ([feats] if batches is None else batches):
            before = _counts()
            outs.append(eng.extract_batch(f).numpy())
            moved = _counts() - before
            assert np.array_equal(moved, _expected_launches(case)), (case.name, et, dict(zip(COUNTERS, moved)))
        assert eng.status() == 0
    finally:
        eng.close()
    return outs[0] if batches is None else outs


def _check(case, et, got, note=""):
    assert not np.isnan(got).any(), (case.name, et)
    errs = CC.errors(case, got, CC.reference64(case, et))
    CC.report(case, et, errs, note)
    for block, err in errs.items():
        assert err < case.tol(et), (case.name, et, block, err, case.tol(et))
    return errs


def _pers_default():
    v = os.environ.get("ASV_AMD_CONV_PERS")
    return v is None or v.strip() not in ("0", "")


# ------------------------------------------------------------------------------------------ the child process

CHILD_WGS = ("", "1", "3")                       # ASV_AMD_CONV_PERS_WGS: uncapped, one workgroup walks every tile, three (the last run is shorter)


def _child_main(path):
    """Runs in the child (ASV_AMD_LIVE_TUNE=1): every narrow case on the one-tile kernel (ASV_AMD_CONV_PERS=0), the ring cases on the
    persistent kernel uncapped and capped; outputs and the launch counters' moves -> npz."""
    from libs.amd import engine
    out = {}
    ring = {c.key for c in CC.ring_cases()}
    for et in H16:
        for case in CC.narrow_cases(32) + CC.narrow_cases(64):
            graph, feats = CC.build(case, et)
            eng = engine.Engine(graph, precision=et)
            runs = [("one", "0", "")] + ([("pers" + w, "1", w) for w in CHILD_WGS] if case.key in ring else [])
            for tag, pers, wgs in runs:
                os.environ["ASV_AMD_CONV_PERS"] = pers
                os.environ.pop("ASV_AMD_CONV_PERS_WGS", None)
                if wgs:
                    os.environ["ASV_AMD_CONV_PERS_WGS"] = wgs
                before = _counts()
                out["%s|%s|%s" % (case.name, et, tag)] = eng.extract_batch(feats).numpy()
                out["%s|%s|%s|moved" % (case.name, et, tag)] = _counts() - before
            out["%s|%s|status" % (case.name, et)] = np.array(eng.status())
            eng.close()
    np.savez(path, **out)


@pytest.fixture(scope="module")
def pers_child(tmp_path_factory):
    import helpers
    path = str(tmp_path_factory.mktemp("conv") / "child.npz")
    code = "import sys; sys.path[:0] = %r; import test_gpu_grid_conv_h16 as t; t._child_main(sys.argv[1])" % (
        [helpers.REPO, os.path.join(helpers.REPO, "asv-subtools_amd", "pytorch"), os.path.join(helpers.REPO, "tests")],)
    env = dict(os.environ, ASV_AMD_LIVE_TUNE="1")
    r = subprocess.run([sys.executable, "-c", code, path], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return dict(np.load(path))


# ------------------------------------------------------------------------------------------ tests

@pytest.mark.parametrize("et", CC.ELEM_TYPES)
def test_c1_kernel_vs_float64(et):
    """32 - 64 output channels (4 - 8 channel chunks: 5, 6 and 7 leave idle threads and odd rows_per_step), 9 / 4 backward / 1 taps,
    F = 82 (halo 84 = C1_HALO) and F = 3, fast and GENERIC (affine_first) epilogues; f32 too (the parity modes' form)."""
    for case in CC.c1_cases():
        _check(case, et, _extract(case, et))


@pytest.mark.parametrize("et", H16)
@pytest.mark.parametrize("F", [82, 61, 8])
@pytest.mark.parametrize("C", [32, 64])
def test_narrow_kernels_vs_float64(C, F, et, pers_child):
    """F = 82 (halo 84 of CHALO 88), 61 (odd), 8; fast epilogue with and without ReLU, GENERIC through affine_first and a residual,
    the rounded family on the small map.  Here: the default form (persistent).  In the child: the one-tile kernel, the same bound
    and, as kernels_conv2d.hip promises (same (tap, k-group) order), the same bits."""
    assert _pers_default(), "ASV_AMD_CONV_PERS=0 in the environment: this test expects the default dispatch"
    for case in CC.narrow_cases(C, F):
        got = _extract(case, et)
        _check(case, et, got, " (persistent)")
        key = "%s|%s|one" % (case.name, et)
        one = pers_child[key]
        assert np.array_equal(pers_child[key + "|moved"], _expected_launches(case, "CONV_NARROW")), (case.name, et, pers_child[key + "|moved"])
        assert int(pers_child["%s|%s|status" % (case.name, et)]) == 0
        _check(case, et, one, " (one tile)")
        assert np.array_equal(one, got), (case.name, et, float(np.abs(one - got).max()))


@pytest.mark.parametrize("et", H16)
@pytest.mark.parametrize("case", CC.ring_cases(), ids=lambda c: "c%d-%s" % (c.cin, c.form))
def test_persistent_ring_after_it_has_wrapped(case, et, pers_child):
    """ASV_AMD_CONV_PERS_WGS = 1: one workgroup walks all 68 (C = 32) / 136 (C = 64) tiles, the 960- / 576-row ring wraps 17 / 30
    times; = 3: runs of 23, 23, 22 / 46, 46, 44 tiles.  The bits of the uncapped launch, and the float64 bound."""
    runs = {w: pers_child["%s|%s|pers%s" % (case.name, et, w)] for w in CHILD_WGS}
    for w in CHILD_WGS:
        moved = pers_child["%s|%s|pers%s|moved" % (case.name, et, w)]
        assert np.array_equal(moved, _expected_launches(case, "CONV_NARROW_PERS")), (case.name, et, w, moved)
        _check(case, et, runs[w], " (persistent, ASV_AMD_CONV_PERS_WGS=%s)" % (w or "unset"))
    rows = CC.row_layout(CC.lengths(case), case.F)[2]
    assert rows // (256 if case.cin == 32 else 128) == (68 if case.cin == 32 else 136)
    for w in ("1", "3"):
        assert np.array_equal(runs[w], runs[""]), (case.name, et, w, float(np.abs(runs[w] - runs[""]).max()))


@pytest.mark.parametrize("et", H16)
@pytest.mark.parametrize("C", [128, 256])
def test_wide_kernel_vs_float64(C, et):
    """C = 128 at F = 22 (the largest map its 24-row halo admits) and 10, C = 256 at F = 14 (halo 16) and 5; fast and GENERIC."""
    for case in CC.wide_cases(C):
        _check(case, et, _extract(case, et))


@pytest.mark.parametrize("et", H16)
def test_s2d_kernel_vs_float64(et):
    """128 -> 64 channels, the four backward taps, F = 46 (reach 48 = S2D_HLO) and 20; fast and GENERIC."""
    for case in CC.s2d_cases():
        _check(case, et, _extract(case, et))


@pytest.mark.parametrize("et", H16)
def test_one_bin_too_wide_falls_back_and_stays_exact(et):
    """C = 128 at F = 23 and C = 256 at F = 15: no launch of the wide kernel (nor of any other of this family but the head's), and
    the exact-family bound on the tile that takes them."""
    for case in CC.fallback_cases():
        _check(case, et, _extract(case, et))


@pytest.mark.parametrize("et", H16)
@pytest.mark.parametrize("case", CC.independence_cases(), ids=lambda c: "%s-c%d-F%d" % (c.kernel, c.cin, c.F))
def test_neighbours_do_not_change_the_bits(case, et):
    """Utterance 0, one short utterance and the last, each extracted alone, give the bits they have in the batch."""
    _, feats = CC.build(case, et)
    lens = [m.shape[0] for m in feats]
    short = [i for i, t in enumerate(lens) if t <= 3 and 0 < i < len(lens) - 1][0]
    picks = [0, short, len(lens) - 1]
    outs = _extract(case, et, batches=[feats] + [[feats[i]] for i in picks])
    whole = outs[0]
    _check(case, et, whole)
    for i, alone in zip(picks, outs[1:]):
        assert alone.shape == (1, whole.shape[1]) and np.array_equal(alone[0], whole[i]), (case.name, et, i)
