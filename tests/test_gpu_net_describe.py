"""The builder's text on the MI355X (a net needs a device): asv_net_describe() of the small golden models the suite already builds, and
the message of every check the asv_net_add_* functions share, against tests/golden/net_describe.json - recorded from the library as it
stood before the host runtime was split into net_build.hip / net_run.hip, with this module's own describe_texts() and
rejection_messages().  tools/ and the profiling read-outs key on the describe text, callers on the messages: both are part of the ABI.

One check the functions share cannot be reached through the C ABI and so has no recorded message: "padded view exceeds pitch" (eltwise,
rowop, posenc).  A view's channel offset is a multiple of 16 and offset + channels <= the buffer's channels, so the view rounded up to a
whole vector (4 or 8 elements) never passes the pitch, the channels rounded up to 16."""

import ctypes as C
import json
import os

import pytest

import helpers

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(helpers.REPO, "tests", "golden", "net_describe.json")

# fixture -> (how to build it, precision): one each of the x-vector C1, ECAPA c3 (16-bit: the one-kernel Res2 block), ResNet34-SE c5, RepSPK,
# the Transformer x-vector with the convolutional front, ECAPA with mqmha, the ECAPA benchmark blueprint (16-bit: the res2n chain), an LDE pooling,
# and a model with row ops
PROGRAMS = {
    "xvector_c1": ("plain", "f32m"),
    "ecapa_c3": ("plain", "bf16"),
    "resnet34se_c5": ("plain", "f32x"),
    "repvgg_spk_small": ("repvgg", "f16"),
    "transformer_conv_small": ("transformer", "f32"),
    "ecapa_mqmha_roadmap": ("plain", "bf16"),
    "ecapa_bench_default": ("plain", "bf16"),
    "snowdar_lde": ("plain", "f32m"),
    "rowop_lx_mish_ln": ("rowop", "f32"),
}
OP_KINDS = ["tdnn", "stats_pool", "attentive_pool", "mq_attentive_pool", "lde_pool", "res2", "res2n", "eltwise", "rowop", "grid_conv", "grid_input", "im2col",
            "grid_flatten", "front_conv", "posenc", "self_attention"]


def _model(name, how):
    if how == "repvgg":
        import repvgg_cases
        return repvgg_cases.golden_model(name)[1]
    if how == "rowop":
        import rowop_cases
        return rowop_cases.golden_model(name)[2]
    if how == "transformer":
        import transformer_cases
        return transformer_cases.golden_model(name)[2]
    return helpers.golden_model(name)[2]


def describe_texts():
    out = {}
    for name, (how, precision) in PROGRAMS.items():
        model = _model(name, how)
        model.cuda()
        model.amd_precision = precision
        out[name] = model._amd_engine().describe()
        model._invalidate_engines()
    return out


def rejection_messages():
    """{case: the exception text of capi.check} - one per shared add-helper and message style, on a bare f32 net with a 64-channel
    frames-domain buffer (1) and a 64-channel buffer on an 8 x 9 grid (2)."""
    from libs.amd import capi
    L = capi.lib()
    net = C.c_void_p()
    capi.check(L.asv_net_create(C.byref(net), 0, capi.PREC_F32, 0, 32), "asv_net_create")
    out = {}

    def reject(case, fn, d, struct_size=None):
        d.struct_size = C.sizeof(type(d)) if struct_size is None else struct_size
        with pytest.raises(capi.AsvError) as e:
            capi.check(getattr(L, fn)(net, C.byref(d)), fn)
        out[case] = str(e.value)

    try:
        frames = capi.check(L.asv_net_new_buffer(net, capi.DOMAIN_FRAMES, 64), "asv_net_new_buffer")
        grid = capi.check(L.asv_net_new_buffer(net, capi.check(L.asv_net_define_grid(net, 0, 8, 9), "asv_net_define_grid"), 64), "asv_net_new_buffer")
        # an output slice [16, 48) over the input slice [0, 32) of the same buffer
        d = capi.TdnnDesc()
        d.in_buf, d.in_ch_off, d.in_ch, d.out_buf, d.out_ch_off, d.out_ch = frames, 0, 32, frames, 16, 32
        d.in2_buf = d.seg_bias_buf = d.seg_scale_buf = d.res_buf = -1
        reject("tdnn_overlap", "asv_net_add_tdnn", d)
        reject("struct_size_both", "asv_net_add_tdnn", d, struct_size=C.sizeof(capi.TdnnDesc) - 4)
        d = capi.GridConvDesc()
        d.in_buf, d.in_ch_off, d.in_ch, d.out_buf, d.out_ch_off, d.out_ch = grid, 0, 32, grid, 16, 32
        reject("grid_conv_overlap", "asv_net_add_grid_conv", d)
        d = capi.SelfAttentionDesc()
        d.heads, d.d_k = 2, 16
        d.q_buf, d.q_ch_off, d.k_buf, d.k_ch_off, d.v_buf, d.v_ch_off, d.out_buf, d.out_ch_off = frames, 0, frames, 32, frames, 32, frames, 16
        reject("self_attention_overlap", "asv_net_add_self_attention", d)
        # neither in place nor disjoint
        d = capi.RowopDesc()
        d.channels, d.in_buf, d.in_ch_off, d.out_buf, d.out_ch_off = 32, frames, 0, frames, 16
        reject("rowop_overlap", "asv_net_add_rowop", d)
        d = capi.PosencDesc()
        d.channels, d.in_buf, d.in_ch_off, d.out_buf, d.out_ch_off = 32, frames, 0, frames, 16
        reject("posenc_overlap", "asv_net_add_posenc", d)
        reject("struct_size_short", "asv_net_add_stats_pool", capi.PoolDesc(), struct_size=4)
    finally:
        L.asv_net_destroy(net)
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_describe_texts_are_the_recorded_ones(golden):
    got = describe_texts()
    assert sorted(got) == sorted(golden["describe"])
    for name in got:
        assert got[name] == golden["describe"][name], name


def test_the_recorded_programs_reach_every_op_kind(golden):
    text = "".join(golden["describe"].values())
    assert [k for k in OP_KINDS if ": %s " % k not in text] == []


def test_rejection_messages_are_the_recorded_ones(golden):
    assert rejection_messages() == golden["rejections"]
