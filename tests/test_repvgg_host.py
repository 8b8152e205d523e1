"""RepVGG / RepSPK x-vector extraction, host side (no GPU): the drop-in surface (state_dict keys and shapes of both forms), the
float64 fold of a block's branches, the lowering of the traced program, a numpy interpreter of that program against the
reference's outputs (tests/golden/repvgg_*.npz), the ABI of the new op, and the refusals."""

import ctypes as C
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import helpers
import repvgg_cases as RC
import repvgg_interp as RI

FIXTURES = sorted(RC.CASES)


def _trace(model, dim):
    from libs.amd import ir
    return ir.trace(model, type(model).extract_embedding.__wrapped_body__, int(dim))


@pytest.fixture(scope="module")
def traced():
    """{fixture name: (fixture, model, graph)}, traced once and shared; leave them unchanged."""
    out = {}
    for name in FIXTURES:
        g, model = RC.golden_model(name)
        out[name] = (g, model, _trace(model, g["dim"]))
    return out


# ------------------------------------------------------------------------------------------ the drop-in surface

@pytest.mark.parametrize("name", FIXTURES)
def test_state_dict_has_the_reference_keys_and_shapes(name):
    """strict load of the reference's key list (the fixture recorded it from the reference's own model), training and deploy form"""
    g, shapes = helpers.load_golden(name)
    creation = str(g["training_creation"]) if int(g["from_training"]) else str(g["creation"])
    model = helpers.build_model(RC.BLUEPRINT, creation)
    ours = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert list(ours) == list(shapes) and ours == shapes
    model.load_state_dict({k: torch.zeros(s) for k, s in shapes.items()}, strict=True)
    if int(g["from_training"]):
        want = {str(k): tuple(int(d) for d in str(v).split(",")) if str(v) else () for k, v in zip(g["deploy_keys"], g["deploy_shapes"])}
        deploy = helpers.build_model(RC.BLUEPRINT, str(g["creation"]))
        got = {k: tuple(v.shape) for k, v in deploy.state_dict().items()}
        assert list(got) == list(want) and got == want
        assert any(k.endswith("rbr_reparam.weight") for k in got) and not any("rbr_dense" in k for k in got)
        from libs.nnet.repvgg import repvgg_model_convert
        conv = repvgg_model_convert(model)
        assert {k: tuple(v.shape) for k, v in conv.state_dict().items()} == want and conv.deploy and not model.deploy


def test_eager_forward_raises_and_surface_is_there():
    model = helpers.build_model(RC.BLUEPRINT, "RepVggXvector(40,10,training=False,repvgg_config={'repvgg_params':{'num_blocks':[1,1,1,1]}})")
    with pytest.raises(NotImplementedError, match="eager forward"):
        model.repvgg(torch.zeros(1, 1, 40, 8))
    with pytest.raises(NotImplementedError, match="eager forward"):
        model.repvgg.stage0(torch.zeros(1, 1, 40, 8))
    assert model.embedding_dim() == 256 and callable(model.extract_embedding_whole)
    from libs import nnet
    for name in ("RepVGGBlock", "RepSPKBlock", "RepVGG", "repvgg_model_convert"):
        assert hasattr(nnet, name)
    auto = helpers.build_model(RC.BLUEPRINT, "RepVggXvector(40,10,training=False,repvgg_config={'auto_model':True,'auto_model_name':'RepVGG_A0','block':'RepVGG'})")
    assert auto.repvgg.stage1[0].rbr_dense.conv.out_channels == 48 and len(auto.repvgg.stage3) == 14


# ------------------------------------------------------------------------------------------ the fold

def _reference_fold64(block):
    """get_equivalent_kernel_bias of the reference (repvgg.py:112-152, 226-275) restated in float64 torch: fuse each branch's
    BatchNorm, pad the 3 x 3 / 1 x 1 to K x K, spread the dilated 3 x 3 over every other position, add."""
    import torch.nn.functional as F
    K = block.K

    def fuse(branch):
        if branch is None:
            return 0, 0
        if isinstance(branch, torch.nn.Sequential):
            kernel, bn = branch.conv.weight.double(), branch.bn
        else:
            bn = branch
            n = block.in_channels
            kernel = torch.zeros(n, n, K, K, dtype=torch.float64)
            kernel[torch.arange(n), torch.arange(n), K // 2, K // 2] = 1
        std = (bn.running_var.double() + bn.eps).sqrt()
        t = (bn.weight.double() / std).reshape(-1, 1, 1, 1)
        return kernel * t, bn.bias.double() - bn.running_mean.double() * bn.weight.double() / std

    k3, b3 = fuse(block.rbr_dense)
    ki, bi = fuse(block.rbr_identity)
    if K == 3:
        k1, b1 = fuse(block.rbr_1x1)
        return k3 + F.pad(k1, [1, 1, 1, 1]) + ki, b3 + b1 + bi
    kd, bd = fuse(block.rbr_dense_dilation)
    spread = torch.zeros(kd.shape[0], kd.shape[1], 5, 5, dtype=torch.float64)
    spread[:, :, ::2, ::2] = kd
    return spread + F.pad(k3, [1, 1, 1, 1]) + ki, b3 + bd + bi


@pytest.mark.parametrize("name,n_taps", [("repvgg_spk_small", 17), ("repvgg_vgg_small", 9)])
def test_fold_equals_get_equivalent_kernel_bias(name, n_taps):
    g, model = RC.golden_model(name)
    blocks = [m for m in model.repvgg.modules() if hasattr(m, "folded_taps")]
    assert len(blocks) == 7
    with torch.no_grad():
        for b in blocks:
            kernel, bias = b.folded_kernel_bias()
            rk, rb = _reference_fold64(b)
            assert kernel.dtype == np.float64 and np.abs(kernel - rk.numpy()).max() <= 1e-12 * max(1.0, np.abs(rk.numpy()).max())
            assert np.abs(bias - rb.numpy()).max() <= 1e-12 * max(1.0, np.abs(rb.numpy()).max())
            taps, w, _ = b.folded_taps()
            assert len(taps) == n_taps and w.shape == kernel.shape[:2] + (n_taps,)
            c = b.K // 2
            for k, (dt, df) in enumerate(taps):
                assert np.array_equal(w[:, :, k], kernel[:, :, df + c, dt + c])
            if b.K == 5:
                from conv_taps_cases import SPK17
                assert sorted(taps) == SPK17


def test_training_form_and_deploy_form_trace_to_the_same_tap_tables(traced):
    """the same ops, the same tap tables, weights and biases equal to float32 rounding (the deploy checkpoint holds the merged
    kernel rounded to float32; the training form is merged in float64 and rounded once)"""
    a, b = traced["repvgg_spk_small"][2], traced["repvgg_spk_deploy"][2]
    assert [op.kind for op in a.ops] == [op.kind for op in b.ops] and a.domains == b.domains
    n = 0
    for x, y in zip(a.ops, b.ops):
        if x.kind in ("grid_conv", "tdnn"):
            assert x.taps == y.taps and x.weight.shape == y.weight.shape
            scale = np.abs(x.weight).max()
            assert np.abs(x.weight - y.weight).max() <= 4 * np.finfo(np.float32).eps * scale
            assert np.abs(x.bias - y.bias).max() <= 4 * np.finfo(np.float32).eps * max(1.0, np.abs(x.bias).max())
            n += x.kind == "grid_conv"
    assert n == 4


# ------------------------------------------------------------------------------------------ the lowering

def test_traced_programs_have_the_op_kinds_of_the_lowering_table(traced):
    kinds = lambda name: [op.kind for op in traced[name][2].ops]
    # RepSPK [1, 2, 2, 1], strides 1, 1, 2, 2, 2: stage0 + stage1 (stride 1: the new op), stage2 = gather + 9-tap layer, then a stride-1 block, ...
    assert kinds("repvgg_spk_small") == ["grid_input", "grid_conv", "grid_conv", "im2col", "tdnn", "grid_conv", "im2col", "tdnn", "grid_conv", "im2col", "tdnn",
                                         "pool", "tdnn"]
    assert kinds("repvgg_spk_deploy") == kinds("repvgg_spk_small")
    g = traced["repvgg_spk_small"][2]
    for op in g.ops:
        if op.kind == "grid_conv":
            assert len(op.taps) == 17 and op.act == "relu" and g.grid_reach(op.inp.tid) == 2
        if op.kind == "im2col":
            assert op.stride == 2 and len(op.taps) == 4
        if op.kind == "tdnn" and g.grid_spec(op.inp.tid) is not None:
            assert len(op.taps) == 9 and op.inp.channels % 4 == 0 and abs(op.alg_fraction - 17 / 36.0) < 1e-12
    live = {g.tensors[op.out.tid][0] for op in g.ops}
    assert all(len(g.domains[d]) == 5 and g.domains[d][3] == g.domains[d][2] + 2 for d in live if g.domains[d][0] == "grid")
    # the default depth: 18 stride-1 blocks + stage0 on the new op, 3 + 1 (fc2) layers on existing kernels
    d = kinds("repvgg_spk_default")
    assert d.count("grid_conv") == 19 and d.count("im2col") == 3 and d.count("tdnn") == 4
    # RepVGG blocks fold to 3 x 3: existing ops on reach-1 grids only
    v = traced["repvgg_vgg_small"][2]
    assert "grid_conv" not in kinds("repvgg_vgg_small") and all(len(s) == 4 for s in v.domains if s[0] == "grid")
    assert all(len(op.taps) in (9, 4, 1) for op in v.ops if op.kind == "tdnn")
    # a frame-weighting pooling: the trunk's output flattened onto the sequence domain
    assert "flatten" in kinds("repvgg_spk_attentive") and "attpool" in kinds("repvgg_spk_attentive")


@pytest.mark.parametrize("name", FIXTURES)
def test_numpy_interpreter_of_the_traced_program_reproduces_the_reference(name, traced):
    g, model, graph = traced[name]
    assert float(g["max_activation"]) * RC.RANGE_MARGIN < RC.RANGE_LIMIT
    for i, m in enumerate(helpers.golden_feats(g)):
        got = RI.extract(graph, m)
        assert helpers.rel_err(got, g["embeddings"][i]) < 1e-4, (name, m.shape[0])


def test_every_pooling_of_the_reference_blueprint_traces():
    small = "repvgg_config={'repvgg_params':{'num_blocks':[1,1,1,1]}}"
    for pooling, params in (("lde", "{'num_head':8}"), ("multi-head", "{'num_head':4,'share':True,'affine_layers':1}"),
                            ("multi-resolution", "{'num_head':4,'share':True,'affine_layers':2,'hidden_size':32,'temperature':True}")):
        model = helpers.build_model(RC.BLUEPRINT, "RepVggXvector(40,10,training=False,pooling='%s',pooling_params=%s,%s)" % (pooling, params, small))
        kinds = [op.kind for op in _trace(model, 40).ops]
        assert "flatten" in kinds and kinds.count("grid_conv") == 2


RESNET_PROGRAMS = {        # sha256 of describe() + the domain list, recorded on the commit before reach-2 grids existed
    "resnet34se_c5": "2e176598ed0f06eeca79479fb4490f97d52296e4cdafded96760b1a57d465d76",
    "resnet_attentive": "cfe530a719665d592c7d2bf24631b6ea0a5d3d92735a7e8197b222c07804272b",
}


def _program_digest(graph):
    return hashlib.sha256((graph.describe() + repr(graph.domains)).encode()).hexdigest()


@pytest.mark.parametrize("name", sorted(RESNET_PROGRAMS))
def test_reach_1_resnet_programs_are_what_they_were(name):
    g, sd, model = helpers.golden_model(name)
    graph = _trace(model, g["dim"])
    assert all(len(s) == 4 and s[3] == s[2] + 1 for s in graph.domains if s[0] == "grid")
    assert not any(op.kind == "grid_conv" for op in graph.ops)
    assert _program_digest(graph) == RESNET_PROGRAMS[name]


# ------------------------------------------------------------------------------------------ the ABI

def test_grid_conv_abi(tmp_path):
    from libs.amd import capi
    header = open(os.path.join(helpers.REPO, "include", "asv_amd.h")).read()
    for sym in ("asv_net_add_grid_conv", "asv_net_define_grid_reach"):
        assert sym in capi.SYMBOLS and re.search(r"int\s+%s\(" % sym, header) and getattr(capi.lib(), sym) is not None
    assert re.search(r"#define ASV_MAX_TAPS 9\b", header) and re.search(r"#define ASV_GRID_CONV_MAX_TAPS 25\b", header)
    assert re.search(r"#define ASV_KERNEL_CONV_TAPS %d\b" % capi.KERNEL_CONV_TAPS, header) and capi.KERNEL_CONV_TAPS == capi.KERNEL_ROWOP + 1
    assert capi.MAX_TAPS == 9 and capi.GRID_CONV_MAX_TAPS == 25
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "asv_amd.h"\nint main(void) {\n  printf("%zu %zu %zu", sizeof(asv_grid_conv_desc_t), '
                   'offsetof(asv_grid_conv_desc_t, weight), offsetof(asv_grid_conv_desc_t, act));\n  return 0;\n}\n')
    exe = tmp_path / "size"
    subprocess.run(["cc", "-I", os.path.join(helpers.REPO, "include"), "-o", str(exe), str(src)], check=True)
    size, off_w, off_act = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert size == C.sizeof(capi.GridConvDesc) and off_w == capi.GridConvDesc.weight.offset and off_act == capi.GridConvDesc.act.offset


# ------------------------------------------------------------------------------------------ the refusals

def test_refusals_name_the_option():
    base = "RepVggXvector(%d,10,training=False,repvgg_config={'repvgg_params':{'num_blocks':[1,1,1,1]%s}%s})"
    with pytest.raises(NotImplementedError, match="use_se"):
        helpers.build_model(RC.BLUEPRINT, base % (40, ",'use_se':True", ""))
    with pytest.raises(NotImplementedError, match="override_groups_map"):
        helpers.build_model(RC.BLUEPRINT, base % (40, ",'override_groups_map':{2:2}", ""))
    from libs.nnet.repvgg import RepSPKBlock, RepVGGBlock
    for cls in (RepSPKBlock, RepVGGBlock):
        with pytest.raises(NotImplementedError, match="groups"):
            cls(32, 32, 3, padding=1, groups=2)
    from libs.amd import ir
    wide = helpers.build_model(RC.BLUEPRINT, base % (82, "", ""))
    with pytest.raises(ir.TraceError, match="82 frequency bins"):
        _trace(wide, 82)
    _trace(helpers.build_model(RC.BLUEPRINT, base % (81, "", "")), 81)            # width + 2 = 83: the widest
    _trace(helpers.build_model(RC.BLUEPRINT, base % (82, "", ",'block':'RepVGG'")), 82)      # 3 x 3 blocks keep the ResNet trunk's limit
    g = ir.Graph(8)
    v = g.grid_input()                                                            # reach 1
    with pytest.raises(ir.TraceError, match="reach-1"):
        g.grid_conv(v, np.zeros((16, 1, 1), np.float32), None, [(2, 0)])


# ------------------------------------------------------------------------------------------ the 16-bit yardstick

@pytest.mark.parametrize("name", ["repvgg_spk_small", "repvgg_vgg_small", "repvgg_spk_default"])
def test_16bit_format_loss_is_what_the_gpu_test_allows_twice(name, traced):
    """tests/test_gpu_repvgg.py holds the device's bf16 / f16 cosines to twice the loss the number format alone causes; that loss is
    re-measured here (float64 arithmetic, the mode's roundings) and must be the figure written there, to 5 %.  Without roundings the
    same evaluation reproduces the reference."""
    from test_gpu_repvgg import H16_LOSS
    g, model, graph = traced[name]
    mats, ref = helpers.golden_feats(g), np.asarray(g["embeddings"], dtype=np.float64)
    for i, m in enumerate(mats[:2]):
        assert helpers.rel_err(RI.run_graph_rounded(graph, m, "f64"), ref[i]) < 1e-4
    for et in ("bf16", "f16"):
        got = np.stack([RI.run_graph_rounded(graph, m, et) for m in mats])
        loss = float((1.0 - (got * ref).sum(1) / np.linalg.norm(got, axis=1) / np.linalg.norm(ref, axis=1)).max())
        assert abs(loss - H16_LOSS[(name, et)]) <= 0.05 * H16_LOSS[(name, et)], (name, et, loss)
