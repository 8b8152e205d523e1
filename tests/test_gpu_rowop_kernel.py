"""rowop_kernel (csrc/kernels_rowop.hip) alone, through the C ABI (asv_rowop_forward), per element type, against float64.

One op per run (tests/rowop_cases.py): each new activation alone, LayerNorm without and with gamma / beta, act -> LN, LN -> act,
affine -> act, act -> affine; 16, 48, 1500 (pitch 1504) and - utts domain - 3000 channels; frames-domain segments of 1, 2, 37,
64 and 65 frames (169 rows); once in place, once at channel offset 16 of a wider buffer.

Gates (rowop_cases' docstring): f32 buffers  e_dev <= 4 e_ref + 2^-24  with e = max |y - y64| / max |y64| and e_ref torch's
float32 CPU result; 16-bit buffers: every element within one unit in the last place of the float64 result rounded to the type.
No NaN / Inf anywhere; columns outside the view keep what they held; the launch counter moves by one per op.
Every case prints its figures ("[rowop] ...").

Measured (profiles/rowop_ab.txt): f32, every layout: e_dev / (4 e_ref + 2^-24) <= 0.205; 16-bit: all 120 (layout, op, type) cases
have every element within one unit.  act -> LN meets the 16-bit gate because the kernel evaluates an activation in front of a
LayerNorm in float64: with the f32 activation one element of 253 500 (bf16 c1500-mish_ln) lay 12 - 13 units off - the activation's
error of ~2^-24 times the cancellation against the row mean."""

import ctypes as C

import numpy as np
import pytest

import rowop_cases as RC

pytestmark = pytest.mark.gpu

LAYOUT_NAMES = [l[0] for l in RC.LAYOUTS]


def _run(case, et):
    from libs.amd import capi
    L = capi.lib()
    before = L.asv_kernel_launch_count(capi.KERNEL_ROWOP)
    buf = RC.run_device(case, et)
    assert L.asv_kernel_launch_count(capi.KERNEL_ROWOP) == before + 1
    x = RC.inputs(case, et)
    lo, hi = case.ch_off, case.ch_off + case.channels
    assert buf.shape == x.shape and np.isfinite(buf).all(), (case.name, et)
    outside = np.ones(x.shape[1], dtype=bool)
    outside[lo:hi] = False
    assert np.array_equal(buf[:, outside], x[:, outside]), "%s %s: columns outside the view changed" % (case.name, et)
    return buf[:, lo:hi]


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_rowop_f32_vs_float64_and_torch(layout):
    worst = 0.0
    for case in [c for c in RC.all_cases() if c.lname == layout]:
        got, y64 = _run(case, "f32"), RC.reference64(case, "f32")
        e_dev, e_ref = RC.max_err(got, y64), RC.max_err(RC.reference_torch32(case, "f32"), y64)
        ratio = e_dev / (4.0 * e_ref + 2.0 ** -24)
        worst = max(worst, ratio)
        print("[rowop] f32 %-28s e_dev %.3e e_ref %.3e  e_dev / (4 e_ref + 2^-24) = %.3f" % (case.name, e_dev, e_ref, ratio))
        assert e_dev <= 4.0 * e_ref + 2.0 ** -24, (case.name, e_dev, e_ref)
    print("[rowop] f32 %s: largest ratio %.3f" % (layout, worst))


@pytest.mark.parametrize("et", ["bf16", "f16"])
@pytest.mark.parametrize("layout", [l[0] for l in RC.LAYOUTS if l[1] == "frames"])
def test_rowop_16bit_within_one_unit_in_the_last_place(layout, et):
    bad = []
    for case in [c for c in RC.all_cases() if c.lname == layout]:
        got, y64 = _run(case, et), RC.reference64(case, et)
        d = RC.ulp_distance(got, y64, et)
        print("[rowop] %s %-28s max distance %d units in the last place, %d of %d elements beyond one" % (et, case.name, int(d.max()), int((d > 1).sum()), d.size))
        if d.max() > 1:
            bad.append((case.name, int(d.max()), int((d > 1).sum())))
    assert not bad, bad


def test_rows_do_not_depend_on_their_neighbours():
    """A row op is per row: the 65-frame segment alone gives the bits it has in the batch (f32 and bf16)."""
    import torch
    from libs.amd import capi
    L = capi.lib()
    case = [c for c in RC.all_cases() if c.name == "c48-mish_ln"][0]
    for et in ("f32", "bf16"):
        whole = RC.run_device(case, et)
        x = np.array(RC.inputs(case, et)[-65:])
        d, keep = RC.make_desc(case)
        xd = torch.from_numpy(x).cuda()
        yd = torch.empty_like(xd)
        offsets = np.array([0, 65], dtype=np.int32)
        capi.check(L.asv_rowop_forward(C.byref(d), RC.PRECISION[et], capi.DOMAIN_FRAMES, case.width, C.c_void_p(xd.data_ptr()), offsets.ctypes.data_as(capi.c_int32_p), 1,
                                       C.c_void_p(yd.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "asv_rowop_forward")
        assert np.array_equal(yd.cpu().numpy(), whole[-65:]), et


def test_add_rowop_rejects_malformed_descriptors():
    from libs.amd import capi
    L = capi.lib()
    net = C.c_void_p()
    capi.check(L.asv_net_create(C.byref(net), 0, capi.PREC_F32, 0, 30), "asv_net_create")
    try:
        fb = capi.check(L.asv_net_new_buffer(net, capi.DOMAIN_FRAMES, 48), "asv_net_new_buffer")
        grid = capi.check(L.asv_net_define_grid(net, 0, 30, 31), "asv_net_define_grid")
        gb = capi.check(L.asv_net_new_buffer(net, grid, 16), "asv_net_new_buffer")
        ones = np.ones(48, dtype=np.float32)

        def desc(**kw):
            d = capi.RowopDesc()
            d.struct_size = C.sizeof(capi.RowopDesc)
            d.channels, d.in_buf, d.out_buf, d.eps = 48, fb, fb, 1e-5
            for k, v in kw.items():
                setattr(d, k, v)
            return d

        def rejected(d, text):
            assert L.asv_net_add_rowop(net, C.byref(d)) < 0
            msg = L.asv_last_error().decode()
            assert text in msg, msg

        rejected(desc(struct_size=8), "struct_size")
        rejected(desc(act0=10), "unknown activation")
        rejected(desc(act1=-1), "unknown activation")
        rejected(desc(in_buf=gb, out_buf=gb, channels=16), "grid")
        rejected(desc(channels=64), "exceeds buffer")
        rejected(desc(in_ch_off=8), "multiple of 16")
        rejected(desc(ln=1, gamma=capi.f32_ptr(ones)), "gamma and beta")
        rejected(desc(gamma=capi.f32_ptr(ones), beta=capi.f32_ptr(ones)), "without ln")
        rejected(desc(ln=1, eps=0.0), "positive eps")
        rejected(desc(scale0=capi.f32_ptr(ones)), "scale and shift")
        rejected(desc(out_buf=0, channels=30), "output buffer")
        # every existing entry point keeps rejecting the new ids
        e = capi.EltwiseDesc()
        e.struct_size = C.sizeof(capi.EltwiseDesc)
        e.channels, e.a_buf, e.out_buf, e.act = 30, 0, fb, capi.ACT_SWISH
        e.b_buf = e.c_buf = e.seg_scale_buf = e.seg_norm_buf = e.d_buf = e.out2_buf = -1
        assert L.asv_net_add_eltwise(net, C.byref(e)) < 0 and "unknown activation" in L.asv_last_error().decode()
        w = np.zeros((48, 30, 1), dtype=np.float32)
        t = capi.TdnnDesc()
        t.struct_size = C.sizeof(capi.TdnnDesc)
        t.in_buf, t.in2_buf, t.out_buf, t.in_ch, t.out_ch, t.n_taps, t.w_tot_context = 0, -1, fb, 30, 48, 1, 1
        t.weight, t.seg_bias_buf, t.seg_scale_buf, t.res_buf, t.act1 = capi.f32_ptr(w), -1, -1, -1, capi.ACT_GELU
        assert L.asv_net_add_tdnn(net, C.byref(t)) < 0 and "unknown activation" in L.asv_last_error().decode()
        assert L.asv_net_add_rowop(net, C.byref(desc(act0=capi.ACT_MISH, ln=1))) == 0
    finally:
        L.asv_net_destroy(net)
