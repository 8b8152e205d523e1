"""Transformer x-vector extraction, host side (no GPU): the drop-in surface (state_dict keys and shapes, `from libs.nnet import *`,
a nnet.config line), the traced program and its q / k / v merge, a float64 interpreter of that program against the reference's
outputs (tests/golden/transformer_*.npz), the unpadded front against torch's own convolutions, the refusals, the ABI of the new ops,
and the CPU-measured yardsticks the GPU tests hold the device to."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import attention_cases as AC
import front_cases as FC
import helpers
import transformer_cases as TC
import transformer_interp as TI

FIXTURES = sorted(TC.CASES)
SMALL = ("TransformerXvector(40,10,training=False,transformer_type='transformer',transformer_params={'attention_dim':64,'attention_heads':2,'num_blocks':1,"
         "'linear_units':64%s}%s)")


def _trace(model, dim):
    from libs.amd import ir
    return ir.trace(model, type(model).extract_embedding.__wrapped_body__, int(dim))


@pytest.fixture(scope="module")
def traced():
    """{fixture name: (fixture, shapes, model, graph)}, traced once and shared; leave them unchanged."""
    out = {}
    for name in FIXTURES:
        g, shapes, model = TC.golden_model(name)
        out[name] = (g, shapes, model, _trace(model, g["dim"]))
    return out


# ------------------------------------------------------------------------------------------ the drop-in surface

@pytest.mark.parametrize("name", FIXTURES)
def test_state_dict_has_the_reference_keys_and_shapes(name):
    """strict load of the reference's key list (the fixture recorded it from the reference's own model), in its order"""
    g, shapes = helpers.load_golden(name)
    model = helpers.build_model(TC.BLUEPRINT, str(g["creation"]))
    ours = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert list(ours) == list(shapes) and ours == shapes
    model.load_state_dict({k: torch.zeros(s) for k, s in shapes.items()}, strict=True)
    for key in ("transformer.embed.out.0.weight", "transformer.encoders.0.self_attn.linear_q.weight", "transformer.encoders.0.feed_forward.w_1.weight",
                "transformer.encoders.0.norm1.weight", "transformer.after_norm.weight", "stats.attention.0.weight", "stats.attention.2.weight",
                "stats.attention.4.weight", "stats.norm_stats.weight"):
        assert key in ours, key
    assert ("transformer.embed.conv.0.weight" in ours) == ("_lin_" not in name)


def test_default_creation_is_the_reference_size():
    g, shapes = helpers.load_golden("transformer_default")
    assert len(shapes) == 120 and sum(int(np.prod(s)) for s in shapes.values()) == 11315328


def test_package_exports_and_eager_forward_raises():
    from libs import nnet
    import libs.nnet.transformer as T
    assert T.__all__ == ["TransformerEncoder", "ConformerEncoder", "MultiHeadedAttention", "LayerNorm", "ReConformerEncoder"]
    for name in T.__all__:
        assert getattr(nnet, name) is getattr(T, name)
    for name in ("TransformerEncoderLayer", "PositionwiseFeedForward", "LinearNoSubsampling", "Conv2dSubsampling4", "PositionalEncoding", "NoPositionalEncoding"):
        assert hasattr(T, name) and not hasattr(nnet, name)                  # the reference's `import *` does not bring them either
    model = helpers.build_model(TC.BLUEPRINT, SMALL % ("", ""))
    assert model.embedding_dim() == 256 and callable(model.extract_embedding_whole) and type(model).extract_embedding.max_chunk == 300
    with pytest.raises(NotImplementedError, match="eager forward"):
        model.transformer(torch.zeros(1, 40, 20))
    with pytest.raises(NotImplementedError, match="eager forward"):
        model.stats(torch.zeros(1, 1536, 20))
    for cls in (nnet.ConformerEncoder, nnet.ReConformerEncoder):
        with pytest.raises(NotImplementedError, match=cls.__name__):
            cls(40)


def test_create_model_from_py_through_a_nnet_config_line(tmp_path):
    import libs.support.utils as utils
    creation = TC.CASES["transformer_conv_small"]["creation"]
    cfg = tmp_path / "nnet.config"
    utils.write_nnet_config(os.path.join(helpers.MODEL_DIR, TC.BLUEPRINT), creation, str(cfg))
    rows = dict(line.split(";", 1) for line in cfg.read_text().splitlines())
    model = utils.create_model_from_py(rows["model_blueprint"], rows["model_creation"])
    assert type(model).__name__ == "TransformerXvector" and model.get_model_creation().startswith("TransformerXvector(40,10")
    assert "self_attention" in [op.kind for op in _trace(model, 40).ops]


# ------------------------------------------------------------------------------------------ the traced program

def test_traced_programs_have_the_expected_ops(traced):
    kinds = lambda name: [op.kind for op in traced[name][3].ops]
    layer = ["rowop", "tdnn", "self_attention", "tdnn", "rowop", "tdnn", "tdnn"]              # LN, [q|k|v], attention, linear_out + x, LN, w_1 (relu), w_2 + x
    tail = ["rowop", "tdnn", "rowop", "tdnn", "rowop", "tdnn", "attpool", "rowop", "tdnn", "rowop"]
    assert kinds("transformer_lin_small") == ["tdnn"] + 2 * layer + tail
    swish = ["rowop", "tdnn", "self_attention", "tdnn", "rowop", "tdnn", "rowop", "tdnn"]       # a row-op activation between w_1 and w_2
    conv = kinds("transformer_conv_small")
    assert conv[:6] == ["front_conv", "im2col", "tdnn", "flatten", "tdnn", "posenc"] and conv[6:22] == 2 * swish and conv.count("pool") == 1
    assert kinds("transformer_default").count("self_attention") == 6 and kinds("transformer_default")[:6] == conv[:6]
    g = traced["transformer_conv_small"][3]
    assert g.domains == [("frames",), ("utts",), ("vgrid", 1, 19, 20), ("vgrid", 2, 9, 10), ("vseq", 2)] and g.min_frames() == 7
    assert traced["transformer_lin_small"][3].domains == [("frames",), ("utts",)] and traced["transformer_lin_small"][3].min_frames() == 1
    for op in g.ops:
        if op.kind == "self_attention":                                   # three slices of the merged projection
            assert op.q.tid == op.k.tid == op.v.tid and (op.q.ch_off, op.k.ch_off, op.v.ch_off) == (0, 64, 128) and (op.heads, op.d_k) == (2, 32)
        if op.kind == "im2col":
            assert op.stride == 2 and op.taps == [(i, j) for i in range(3) for j in range(3)]
        if op.kind == "posenc":
            assert op.scale == 8.0 and op.pe.shape == (5000, 64)
    far = traced["transformer_far"][3]
    assert far.ops[-1].kind == "tdnn" and far.ops[-1].act1 is None and far.output.channels == 64


def test_qkv_merge_leaves_other_projections_alone():
    """three 1-tap affines are merged only when nothing but the attention op reads them"""
    from libs.amd import ir
    g = ir.Graph(16)
    w = lambda: np.random.RandomState(0).randn(32, 16, 1).astype(np.float32)
    q, k, v = (g.tdnn(g.full_view(0), w(), np.zeros(32, np.float32), [0], 0) for _ in range(3))
    att = g.self_attention(q, k, v, 2, 16)
    both = g.eltwise(att, b=q)                                              # q has a second reader
    g.output = g.pool(both)
    g.optimize()
    assert [op.kind for op in g.ops].count("tdnn") == 3


@pytest.mark.parametrize("name", FIXTURES)
def test_numpy_interpreter_of_the_traced_program_reproduces_the_reference(name, traced):
    g, _, model, graph = traced[name]
    assert float(g["max_activation"]) * TC.RANGE_MARGIN < TC.RANGE_LIMIT and np.isfinite(g["embeddings"]).all()
    for i, m in enumerate(helpers.golden_feats(g)):
        got = TI.extract(graph, m)
        assert helpers.rel_err(got, g["embeddings"][i]) < 1e-5, (name, m.shape[0], helpers.rel_err(got, g["embeddings"][i]))


def test_positions_restart_in_every_chunk(traced):
    """T = 650 runs as chunks of 216 / 216 / 218 frames: evaluated as ONE chunk (positions running on, attention across the whole
    utterance) the same program gives another embedding"""
    g, _, model, graph = traced["transformer_conv_small"]
    m = helpers.golden_feats(g)[5]
    assert helpers.rel_err(TI.extract(graph, m, max_chunk=300), g["embeddings"][5]) < 1e-5
    assert helpers.rel_err(TI.extract(graph, m, max_chunk=10000), g["embeddings"][5]) > 1e-3


@pytest.mark.parametrize("F", FC.WIDTHS)
def test_front_program_equals_torch_convolutions(F):
    """front_conv -> im2col(valid) -> K = 9 d layer -> flatten -> Linear, interpreted, against torch's unpadded Conv2d pair in float64,
    on every length of the GPU test; row counts L(T)"""
    graph = FC.build(F)
    for m in FC.features(F):
        assert np.abs(TI.run_graph(graph, m) - FC.reference_torch64(m, F)).max() < 1e-12
        assert TI.valid_len(m.shape[0], 2) == FC.rows_of(m.shape[0])
    assert [FC.rows_of(T) for T in FC.LENGTHS] == [1, 1, 1, 1, 2, 15, 15] and FC.rows_of(6) == 0


# ------------------------------------------------------------------------------------------ the refusals

REFUSED_ENCODER = [
    ("pos_enc_type", "'pos_enc_type':'rel_pos'"), ("pos_enc_type", "'pos_enc_type':'rot_pos'"), ("att_type", "'att_type':'gau'"),
    ("positionwise_layer_type", "'positionwise_layer_type':'conv1d'"), ("positionwise_layer_type", "'positionwise_layer_type':'gau'"),
    ("norm_method", "'attention_norm_args':{'norm_method':'relu_plus'}"), ("norm_method", "'attention_norm_args':{'norm_method':'softmax_plus'}"),
    ("scale_adapt", "'attention_norm_args':{'scale_adapt':True}"), ("diag_mask", "'attention_norm_args':{'diag_mask':True}"),
    ("g_sa", "'attention_norm_args':{'g_sa':True}"),
    ("input_layer", "'input_layer':'conv2d2'"), ("input_layer", "'input_layer':'re_conv2d'"), ("input_layer", "'input_layer':'conv2d6'"),
    ("input_layer", "'input_layer':'conv2d8'"), ("combiner_type", "'combiner_type':'mfa'"), ("convfnn_blocks", "'convfnn_blocks':1"),
    ("mlp_head", "'mlp_head':True"), ("add_t5rel_bias", "'add_t5rel_bias':True"), ("attention_conv_out", "'attention_conv_out':True"),
    ("re_scale", "'re_scale':True"), ("activation_balancer", "'activation_balancer':True"), ("concat_after", "'concat_after':True"),
    ("normalize_before", "'normalize_before':False"), ("norm_type", "'norm_type':'batch_norm'"), ("norm_type", "'norm_type':'basic_norm'"),
    ("static_chunk_size", "'static_chunk_size':16"), ("left_chunk_size", "'left_chunk_size':4"), ("use_dynamic_chunk", "'use_dynamic_chunk':True"),
    ("use_dynamic_left_chunk", "'use_dynamic_left_chunk':True"),
]


@pytest.mark.parametrize("option,text", REFUSED_ENCODER)
def test_refused_encoder_options_name_the_option(option, text):
    with pytest.raises(NotImplementedError, match=option):
        helpers.build_model(TC.BLUEPRINT, SMALL % ("," + text, ""))


def test_other_refusals_and_accepted_options():
    for kind in ("conformer", "re_conformer"):
        with pytest.raises(NotImplementedError, match="transformer_type='%s'" % kind):
            helpers.build_model(TC.BLUEPRINT, "TransformerXvector(40,10,training=False,transformer_type='%s')" % kind)
    with pytest.raises(NotImplementedError, match="transformer_type='conformer'"):
        helpers.build_model(TC.BLUEPRINT, "TransformerXvector(40,10,training=False)")                  # the reference's default type
    with pytest.raises(NotImplementedError, match="stddev"):
        helpers.build_model(TC.BLUEPRINT, SMALL % ("", ",pooling_params={'stddev':False}"))
    with pytest.raises(NotImplementedError, match="training"):
        helpers.build_model(TC.BLUEPRINT, "TransformerXvector(40,10,transformer_type='transformer')")
    with pytest.raises(NotImplementedError, match="multiple of 16"):
        helpers.build_model(TC.BLUEPRINT, SMALL % (",'attention_heads':8", ""))                         # d_k = 8
    with pytest.raises(ValueError, match="unknown input_layer"):
        helpers.build_model(TC.BLUEPRINT, SMALL % (",'input_layer':'conv3d'", ""))
    from libs.nnet import MQMHASP_Linear
    with pytest.raises(NotImplementedError):
        MQMHASP_Linear(64)
    # accepted: the eval-identity combiners, train_len, every activation of the layer factory, both positions
    for text in ("'combiner_type':'random_frame'", "'combiner_type':'random_layer'", "'attention_norm_args':{'norm_method':'softmax','train_len':512.}",
                 "'activation_type':'gelu'", "'activation_type':'tanh'", "'input_layer':'linear','pos_enc_type':'abs_pos'", "'pos_enc_type':'no_pos'"):
        model = helpers.build_model(TC.BLUEPRINT, SMALL % ("," + text, ""))
        assert "self_attention" in [op.kind for op in _trace(model, 40).ops]


def test_short_chunks_are_a_value_error_before_the_library_is_asked(traced):
    """T = 6 behind the conv2d front: Engine.check_chunk_lengths is what extract_device runs first"""
    from libs.amd.engine import Engine
    stub = Engine.__new__(Engine)
    stub.graph = traced["transformer_conv_small"][3]
    stub.check_chunk_lengths(np.array([0, 7, 307], np.int32), 300)
    stub.check_chunk_lengths(np.array([0, 14], np.int32), 7)                      # 7 + 7
    for offsets, mc in (([0, 6], 300), ([0, 100, 106], 300), ([0, 13], 7), ([0, 305], 60)):      # 305 = 5 x 50 + 55: fine; 13 = 6 + 7: not
        if offsets == [0, 305]:
            stub.check_chunk_lengths(np.array(offsets, np.int32), mc)
            continue
        with pytest.raises(ValueError, match="at least 7"):
            stub.check_chunk_lengths(np.array(offsets, np.int32), mc)
    stub.graph = traced["transformer_lin_small"][3]
    stub.check_chunk_lengths(np.array([0, 1, 3], np.int32), 300)                 # no unpadded front: nothing to refuse


# ------------------------------------------------------------------------------------------ the ABI

def test_new_ops_abi(tmp_path):
    from libs.amd import capi
    header = open(os.path.join(helpers.REPO, "include", "asv_amd.h")).read()
    for sym in ("asv_net_define_grid_valid", "asv_net_add_front_conv", "asv_net_add_posenc", "asv_net_add_self_attention"):
        assert sym in capi.SYMBOLS and re.search(r"int\s+%s\(" % sym, header) and getattr(capi.lib(), sym) is not None
    for name, value in (("ATTENTION", capi.KERNEL_ATTENTION), ("POSENC", capi.KERNEL_POSENC), ("FRONT_CONV", capi.KERNEL_FRONT_CONV)):
        assert re.search(r"#define ASV_KERNEL_%s %d\b" % (name, value), header)
    assert capi.KERNEL_ATTENTION == capi.KERNEL_CONV_TAPS + 1
    structs = (("asv_self_attention_desc_t", capi.SelfAttentionDesc, "out_ch_off"), ("asv_posenc_desc_t", capi.PosencDesc, "pe_rows"),
               ("asv_front_conv_desc_t", capi.FrontConvDesc, "bias"))
    body = "".join('  printf("%%zu %%zu ", sizeof(%s), offsetof(%s, %s));\n' % (c, c, f) for c, _, f in structs)
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "asv_amd.h"\nint main(void) {\n%s  return 0;\n}\n' % body)
    exe = tmp_path / "size"
    subprocess.run(["cc", "-I", os.path.join(helpers.REPO, "include"), "-o", str(exe), str(src)], check=True)
    nums = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    for i, (_, cls, field) in enumerate(structs):
        assert nums[2 * i] == C.sizeof(cls) and nums[2 * i + 1] == getattr(cls, field).offset, cls.__name__


# ------------------------------------------------------------------------------------------ the yardsticks of the GPU tests

@pytest.mark.parametrize("name", FIXTURES)
def test_16bit_format_loss_is_what_the_gpu_test_allows_twice(name, traced):
    """tests/test_gpu_transformer.py holds the device's bf16 / f16 cosines to twice the loss the number format alone causes; that loss
    is re-measured here (float64 arithmetic, the mode's roundings) and must be the figure written there, to 5 %"""
    from test_gpu_transformer import H16_LOSS
    g, _, model, graph = traced[name]
    mats, ref = helpers.golden_feats(g), np.asarray(g["embeddings"], dtype=np.float64)
    for et in ("bf16", "f16"):
        got = np.stack([TI.extract(graph, m, et=et) for m in mats])
        loss = float((1.0 - (got * ref).sum(1) / np.linalg.norm(got, axis=1) / np.linalg.norm(ref, axis=1)).max())
        print("[transformer] %-24s %-4s format-alone cosine loss %.3g" % (name, et, loss))
        assert abs(loss - H16_LOSS[(name, et)]) <= 0.05 * H16_LOSS[(name, et)], (name, et, loss)


def test_attention_yardstick_is_what_the_gpu_test_allows_four_times():
    """tests/test_gpu_attention_kernel.py allows the device 4 x the error of the float32 torch restatement against float64; those
    errors are re-measured here.  The 16-bit figures are roundings of exact inputs and reproduce exactly (5 %); the float32 ones
    depend on the summation order of the host's matrix product: the documented figure must be no smaller than half of, and no larger
    than twice, what this host measures."""
    from test_gpu_attention_kernel import YARDSTICK
    mats = AC.features()
    for heads in AC.HEADS:
        for d_k in AC.D_KS:
            ref = np.stack([AC.reference64(m, heads, d_k) for m in mats])
            for et in AC.ELEM_TYPES:
                err = AC.block_err(np.stack([AC.yardstick32(m, heads, d_k, et) for m in mats]), ref)
                doc = YARDSTICK[(heads, d_k)][et]
                print("[attention] heads %d d_k %3d %-4s yardstick %.3g (documented %.3g)" % (heads, d_k, et, err, doc))
                assert (0.5 * err <= doc <= 2.0 * err) if et == "f32" else abs(err - doc) <= 0.05 * doc, (heads, d_k, et, err, doc)
    m = mats[5]
    for et in AC.ELEM_TYPES:
        err = AC.block_err(AC.yardstick32(m, 4, 64, et, 65), AC.reference64(m, 4, 64, 65))
        doc = YARDSTICK["chunked"][et]
        assert (0.5 * err <= doc <= 2.0 * err) if et == "f32" else abs(err - doc) <= 0.05 * doc, ("chunked", et, err, doc)
    # the q, k and v values of the cases are exact in every element type, as the cases' docstring claims
    from rowop_cases import round_to
    qkv = mats[5] @ AC.weights(4, 128).T
    assert np.array_equal(round_to(qkv, "bf16"), qkv) and np.abs(qkv).max() <= 4
