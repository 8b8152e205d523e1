"""The activations beyond relu / tanh / sigmoid and `ln_replace` (LayerNorm) on the host: the layer factory builds them with the
reference's parameter names, the traced programs hold the row ops the layers stand for and reproduce the embeddings the
reference itself produced (tests/gen_rowop_golden.py), the numpy model of the op equals torch's own modules, graphs of the
built-in activations are untouched, and the C ABI of the new entry point agrees with its ctypes binding."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
import rowop_cases as RC
import rowop_interp
from helpers import rel_err

FIXTURES, golden_model = RC.FIXTURES, RC.golden_model
INTERPRETED = sorted(n for n in FIXTURES if "ecapa" not in n)          # rowop_interp runs tdnn / pool / rowop programs
_traced = {}


def _trace(name):
    if name not in _traced:
        from libs.amd import ir
        g, sd, model = golden_model(name)                                # strict load: the reference's parameter names and shapes
        _traced[name] = (g, model, ir.trace(model, type(model).extract_embedding.__wrapped_body__, int(g["dim"])))
    return _traced[name]


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_blueprint_takes_the_reference_checkpoint(name):
    g, model, _ = _trace(name)
    _, shapes = helpers.load_golden(name)
    mine = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert list(mine) == list(shapes) and mine == shapes
    if any(spec[2] for spec in FIXTURES[name]):                          # LayerNorm: weight / bias under the BatchNorm's name, no statistics
        assert not any(k.startswith("tdnn7.batchnorm.running") for k in mine)
        assert ("tdnn6.batchnorm.weight" in mine) == FIXTURES[name][-2][3] and ("tdnn7.batchnorm.bias" in mine) == FIXTURES[name][-1][3]


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_traced_program_holds_the_row_ops(name):
    g, model, graph = _trace(name)
    got = [(op.act0, op.slope0, op.ln, op.gamma is not None, op.act1, op.scale1 is not None, graph.is_utts(op.inp.tid))
           for op in graph.ops if op.kind == "rowop"]
    assert [(t[0], round(t[1], 6)) + t[2:] for t in got] == [(t[0], round(t[1], 6)) + t[2:] for t in FIXTURES[name]]
    for i, op in enumerate(graph.ops):
        if op.kind != "rowop":
            continue
        prev = graph.ops[i - 1]
        assert prev.kind == "tdnn" and prev.out == op.inp and op.scale0 is None and (op.eps == 1e-5 or not op.ln)
        assert op.gamma is None or (op.gamma.shape == op.beta.shape == (op.inp.channels,))
        if name == "rowop_lx_leaky02_bnfirst":                            # BN -> act: the BatchNorm stays in the GEMM epilogue
            assert prev.scale is not None and prev.act1 is None
        elif name == "rowop_lx_head_ln" and not graph.is_utts(op.inp.tid):  # ReLU in front of a LayerNorm stays there too
            assert prev.act1 == "relu" and prev.scale is None
        else:
            assert prev.act1 is None and prev.scale is None


@pytest.mark.parametrize("name", INTERPRETED)
def test_traced_program_reproduces_the_reference_on_cpu(name):
    g, model, graph = _trace(name)
    assert {op.kind for op in graph.ops} == {"tdnn", "pool", "rowop"}
    for (T, _), x, ref in zip(g["utts"], helpers.golden_feats(g), g["embeddings"]):
        err = rel_err(rowop_interp.extract(graph, x), ref)
        print("%s T=%d: rel err %.3g" % (name, T, err))
        assert err < 1e-4, (name, int(T), err)


@pytest.mark.parametrize("layout", [l[0] for l in RC.LAYOUTS if l[0] in ("c16", "c1500", "c3000_utts")])
def test_numpy_model_equals_the_torch_modules_in_float64(layout):
    """LeakyReLU, SELU, SiLU, F.gelu, x tanh(softplus x), x sigmoid(x - 1), F.layer_norm in float64 on the GPU test's inputs."""
    import torch
    for case in RC.all_cases():
        if case.lname != layout:
            continue
        x = RC.inputs(case, "f32")[:, case.ch_off:case.ch_off + case.channels]
        want = RC.rowop_torch(x, torch.float64, **RC.fields(case))
        got = RC.reference64(case, "f32")
        assert np.isfinite(got).all() and np.isfinite(want).all()
        err = rel_err(got, want)
        print("%s: model vs torch float64 %.3g" % (case.name, err))
        assert err < 1e-13, (case.name, err)


def test_every_new_activation_is_constructible_and_named():
    import torch
    from libs.nnet import activation as A
    for name in A.ROWOP_ACTIVATIONS + A.HIP_ACTIVATIONS:
        assert A.activation_name(A.Nonlinearity(name)) == name
    assert isinstance(A.Nonlinearity("swish"), torch.nn.SiLU) and isinstance(A.Nonlinearity("gelu"), torch.nn.GELU)
    assert A.Nonlinearity("gelu").approximate == "none"
    assert A.Nonlinearity("leaky_relu", negative_slope=0.3).negative_slope == 0.3
    assert A.Nonlinearity("") is None and A.activation_name(None) is None
    with pytest.raises(ValueError):
        A.Nonlinearity("softsign")
    with pytest.raises(NotImplementedError, match="eager forward"):
        A.Mish()(torch.zeros(3))


def test_layer_norm_follows_the_reference_options():
    from libs.nnet import components as K
    bn_off = {"momentum": 0.1, "affine": False, "track_running_stats": True}
    a = K.ReluBatchNormTdnnLayer(8, 16, ln_replace=True, bn_params=bn_off)
    assert isinstance(a.batchnorm, K.LayerNorm) and not a.batchnorm.elementwise_affine and a.batchnorm.eps == 1e-5 and a.batchnorm.dim == 1
    b = K.ReluBatchNormTdnnLayer(8, 16, ln_replace=True, bn_params=bn_off, **{"bn-relu": True})
    assert b.batchnorm.elementwise_affine and list(b.state_dict()) == ["affine.weight", "affine.bias", "batchnorm.weight", "batchnorm.bias"]
    assert list(K.ReluBatchNormTdnnLayer(8, 16, ln_replace=True, bn=False).state_dict()) == ["affine.weight", "affine.bias"]


@pytest.mark.parametrize("name", ["xvector_c1", "snowdar_default", "ecapa_c512_fc1_far", "extended_far", "factored_far", "resnet34_plain"])
def test_graphs_of_the_built_in_activations_hold_no_row_op(name):
    from libs.amd import ir
    g, sd, model = helpers.golden_model(name)
    graph = ir.trace(model, type(model).extract_embedding.__wrapped_body__, int(g["dim"]))
    assert "rowop" not in [op.kind for op in graph.ops]


def test_abi_entry_and_struct_layout(tmp_path):
    from libs.amd import capi
    header = open(os.path.join(helpers.REPO, "include", "asv_amd.h")).read()
    for sym in ("asv_net_add_rowop", "asv_rowop_forward"):
        assert sym in capi.SYMBOLS and re.search(r"int\s+%s\(" % sym, header) and getattr(capi.lib(), sym) is not None
    assert capi.KERNEL_ROWOP == 14 == int(re.search(r"#define\s+ASV_KERNEL_ROWOP\s+(\d+)", header).group(1))
    acts = {n: int(v) for n, v in re.findall(r"#define\s+ASV_ACT_([A-Z_]+)\s+(\d+)", header)}
    assert [acts[k] for k in ("NONE", "RELU", "TANH", "SIGMOID")] == [0, 1, 2, 3]                      # not renumbered
    assert {k.lower(): v for k, v in acts.items() if v >= 4} == {k: v for k, v in capi.ROWOP_ACT_BY_NAME.items() if k and v >= 4}
    assert set(capi.ACT_BY_NAME.values()) == {0, 1, 2, 3}                                               # the other entry points' table
    fields = [n for n, _ in capi.RowopDesc._fields_]
    src = tmp_path / "rowop_sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "asv_amd.h"\nint main(void) {\n  printf("%zu", sizeof(asv_rowop_desc_t));\n'
                   + "".join('  printf(" %%zu", offsetof(asv_rowop_desc_t, %s));\n' % f for f in fields)
                   + '  printf(" %zu %zu %zu\\n", sizeof(asv_tdnn_desc_t), sizeof(asv_eltwise_desc_t), sizeof(asv_pool_desc_t));\n  return 0;\n}\n')
    exe = tmp_path / "rowop_sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(helpers.REPO, "include"), str(src), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert vals[0] == C.sizeof(capi.RowopDesc)
    assert vals[1:1 + len(fields)] == [getattr(capi.RowopDesc, f).offset for f in fields]
    assert vals[-3:] == [C.sizeof(capi.TdnnDesc), C.sizeof(capi.EltwiseDesc), C.sizeof(capi.PoolDesc)] == [152, 96, 44]       # the existing structs keep their sizes
    assert capi.lib().asv_kernel_launch_count(capi.KERNEL_ROWOP) >= 0
