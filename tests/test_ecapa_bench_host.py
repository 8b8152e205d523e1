"""The reference's benchmark ECAPA-TDNN blueprint (model/ecapa-tdnn-xvector.py, the file launcher/runEcapaXvector.py trains) on the
host: our blueprint takes the reference's checkpoints, the traced program reproduces the embeddings the reference itself produced
(tests/gen_ecapa_bench_golden.py), the reference's own file traces to the same program, the late graph pass turns each Res2 chain
into one op, and the plumbing of that op (tests/res2n_cases.py, kernel resources, C ABI) is in place."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
import ir_interp
import res2n_cases as RC
from helpers import rel_err
from test_kernel_resources import HIPCC, device_asm

# name -> (channels, Res2 group width)
FIXTURES = {"ecapa_bench_default": (512, 64), "ecapa_bench_launcher": (512, 64), "ecapa_bench_c1024_far": (1024, 128), "ecapa_bench_stats": (512, 64),
            "ecapa_bench_multihead": (512, 64)}
REF_FILE = "/root/reference/pytorch/model/ecapa-tdnn-xvector.py"
_traced = {}


def _trace(name):
    if name not in _traced:
        from libs.amd import ir
        g, sd, model = helpers.golden_model(name)                      # strict load: the reference's parameter names and shapes
        _traced[name] = (g, sd, model, ir.trace(model, type(model).extract_embedding.__wrapped_body__, int(g["dim"])))
    return _traced[name]


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_blueprint_takes_the_reference_checkpoint(name):
    g, sd, model, _ = _trace(name)
    assert str(g["blueprint"]) == "ecapa-tdnn-xvector.py"
    _, shapes = helpers.load_golden(name)
    mine = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert list(mine) == list(shapes) and mine == shapes
    for key in ("layer2.0.conv.weight", "layer2.1.convs.3.weight", "layer2.1.bns.3.running_var", "layer2.3.linear1.weight", "conv.bias", "bn_conv.running_mean"):
        assert key in mine, key
    assert "layer2.0.conv.bias" not in mine and "layer2.1.convs.0.bias" not in mine


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_program_has_three_chains_and_the_pass_fuses_the_64_wide_ones(name):
    from libs.amd import ir
    g, sd, model, graph = _trace(name)
    C_, Wd = FIXTURES[name]
    chain = [op for op in graph.ops if op.kind == "tdnn" and len(op.taps) == 3]
    assert len(chain) == 21 and all(op.inp.channels == Wd and op.out.channels == Wd and op.bias is None for op in chain)
    assert sorted({op.taps[2] for op in chain}) == [2, 3, 4]
    for blk in range(3):                                                # dependent: branch k reads branch k - 1's slice and group k of the input
        ops = chain[7 * blk:7 * blk + 7]
        assert ops[0].inp2 is None and ops[0].inp.ch_off == 0
        for k in range(1, 7):
            assert ops[k].inp == ops[k - 1].out and ops[k].inp2 == ir.View(ops[0].inp.tid, k * Wd, Wd)
    assert not any(op.kind == "cat" for op in graph.ops)
    copies = [op for op in graph.ops if op.kind == "eltwise" and op.b is None and op.seg_scale is None and op.scale is None and getattr(op, "act", None) is None]
    assert len(copies) == 3 and all(op.a.channels == Wd and op.a.ch_off == 7 * Wd for op in copies)     # the three pass-through groups, nothing else
    before = list(graph.ops)
    fused = graph.fused_res2n_ops()
    assert graph.ops == before                                          # a late pass: the graph keeps its own list
    kinds = [op.kind for op in fused]
    assert graph.fused_res2_ops() == before and "res2" not in kinds    # the 128-wide pass finds nothing here
    if Wd == 64:
        assert kinds.count("res2n") == 3 and len(fused) == len(before) - 3 * 7
        for op, d in zip([o for o in fused if o.kind == "res2n"], (2, 3, 4)):
            assert (op.width, op.groups, op.pass_group, op.dilation, op.bias) == (64, 8, 7, d, None)
            assert op.weight.shape == (7, 64, 64, 2 * d + 1) and op.scale.shape == op.shift.shape == (7, 64)
            assert op.inp.channels == op.out.channels == 512 and op.inp.ch_off == op.out.ch_off == 0
        assert [o for o in fused if o.kind != "res2n"] == [o for o in before if o not in chain and o not in copies]
    else:                                                               # channels = 1024: groups of 128 stay one layer per branch
        assert fused == before


def test_the_pass_leaves_the_other_blueprint_and_broken_chains_alone():
    from libs.amd import ir
    g, sd, model = helpers.golden_model("ecapa_c512_near_affine")       # model/ecapa_tdnn_xvector.py at C = 512: group 0 passes through
    graph = ir.trace(model, type(model).extract_embedding.__wrapped_body__, int(g["dim"]))
    assert graph.fused_res2n_ops() == graph.ops
    both = graph.fused_res2n_ops(pass_groups=("last", "first"))         # the kernel covers that wiring; only on request
    assert [op.kind for op in both].count("res2n") == 3 and all(op.pass_group == 0 and op.bias is not None for op in both if op.kind == "res2n")
    _, _, _, mine = _trace("ecapa_bench_default")
    ops = list(mine.ops)
    idx = [i for i, op in enumerate(ops) if op.kind == "tdnn" and len(op.taps) == 3]
    cut = ops[:idx[3]] + ops[idx[3] + 1:]                               # one branch missing: not the pattern
    assert [op.kind for op in mine.fused_res2n_ops(cut)].count("res2n") == 2


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_traced_program_reproduces_the_reference_in_float64(name):
    g, sd, model, graph = _trace(name)
    assert all(op.kind in ("tdnn", "pool", "attpool", "eltwise") for op in graph.ops)          # the unfused program: existing op kinds only
    for (T, _), x, ref in zip(g["utts"], helpers.golden_feats(g), g["embeddings"]):
        err = rel_err(ir_interp.extract(graph, x, dtype=np.float64), ref)
        print("%s T=%d: rel err %.3g" % (name, T, err))
        assert err < 1e-4, (name, int(T), err)


@pytest.mark.skipif(not os.path.exists(REF_FILE), reason="needs the reference tree (build container only)")
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_the_references_own_file_traces_to_the_same_program(name):
    import torch
    import libs.support.utils as utils
    from libs.amd import ir
    g, sd, model, graph = _trace(name)
    ref = utils.create_model_from_py(REF_FILE, str(g["creation"]))
    ref.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    ref.eval()
    assert type(ref.layer2[3]).__name__ == "SE_Connect" and not hasattr(ref.layer2[3], "se")
    traced = ir.trace(ref, type(ref).extract_embedding.__wrapped_body__, int(g["dim"]))
    assert traced.describe() == graph.describe()
    assert "forward" not in ref.layer2[3].__dict__                      # the recorder put the module back as it found it


def test_unsupported_layers_raise_with_a_message():
    import torch
    from libs.amd import ir
    g = ir.Graph(64)
    x = ir.Sym(g, g.full_view(0), 3)
    model = helpers.build_model("ecapa-tdnn-xvector.py", "ECAPA_TDNN(64,10,training=False)")
    blk = type(model.layer1)
    for kw in (dict(kernel_size=4, padding=2), dict(kernel_size=3, padding=0), dict(kernel_size=3, padding=1, stride=2)):
        with pytest.raises(ir.TraceError, match="odd kernel, stride 1"):
            blk(64, 64, **kw)(x)
    with pytest.raises(ir.TraceError, match="halo"):
        blk(64, 64, kernel_size=3, padding=5, dilation=5)(x)
    with pytest.raises(ir.TraceError, match="relu, conv1d"):
        torch.nn.functional.gelu(x)
    with pytest.raises(NotImplementedError, match="eager forward"):
        model.layer1(torch.zeros(1, 64, 10))


def test_relu_behind_a_shared_affine_stays_an_elementwise_pass():
    """F.relu folds into the affine in front of it only when nobody else reads that affine; a BatchNorm only behind such a fold."""
    import torch
    import torch.nn.functional as F
    from libs.amd import ir

    class Two(torch.nn.Module):
        def __init__(self):
            super(Two, self).__init__()
            self.conv = torch.nn.Conv1d(16, 16, 1)
            self.bn = torch.nn.BatchNorm1d(16)
            self.pool = helpers.build_model("ecapa-tdnn-xvector.py", "ECAPA_TDNN(16,10,training=False,pooling='statistics')").stats.__class__(16)

    m = Two()
    folded = ir.trace(m, lambda self, x: self.pool(self.bn(F.relu(self.conv(x)))), 16)
    assert [op.kind for op in folded.ops] == ["tdnn", "pool"] and folded.ops[0].act1 == "relu" and folded.ops[0].scale is not None

    def shared(self, x):
        y = self.conv(x)
        return self.pool(F.relu(y) + y)
    kept = ir.trace(m, shared, 16)
    assert [op.kind for op in kept.ops] == ["tdnn", "eltwise", "eltwise", "pool"] and kept.ops[0].act1 is None and kept.ops[1].act == "relu"


# ---- the one-op cases of tests/res2n_cases.py

def test_case_batches_put_segment_ends_around_tile_edges():
    from libs.amd import capi
    assert RC.M == capi.RES2N_TILE_ROWS
    rep = RC.seam_report(RC.RAGGED)
    assert all(v >= 1 for v in rep.values()), rep
    assert set((1, 2, 3, 27, 28, 29, RC.M - 1, RC.M, RC.M + 1, 2 * RC.M + 5)) <= set(RC.RAGGED) and len(RC.RAGGED) <= 16
    assert RC.row_layout(RC.SMALL)[0][-1] + RC.SMALL[-1] < RC.M
    cases = RC.all_cases(True)
    assert {(c.d, c.first, c.n, c.bias) for c in cases} == {(d, f, n, b) for d in (2, 3, 4) for f in (True, False) for n in (1, 7) for b in (True, False)}
    assert {c.in_off for c in cases} == {c.out_off for c in cases} == {0, 64}


@pytest.mark.parametrize("case", RC.all_cases(True)[::5] + RC.all_cases(False)[2::7], ids=lambda c: c.name)
def test_case_reference_reproduces_the_interpreter_on_the_unfused_chain(case):
    """Without its roundings the reference of tests/res2n_cases.py is the program tests/ir_interp.py runs over the per-branch ops."""
    graph, feats = RC.unfused_graph(case, "bf16", RC.SMALL)
    ref = RC.evaluate(case, "bf16", RC.SMALL, rounding=False)
    for i, f in enumerate(feats):
        got = ir_interp.run_graph(graph, f, dtype=np.float64)
        assert rel_err(got, ref[i]) < 1e-12, (case, i)
    fused, _ = RC.fused_graph(case, "bf16", RC.SMALL)
    assert [op.kind for op in fused.ops] == ["res2n", "pool"]
    op = fused.ops[0]
    assert (op.inp.ch_off, op.out.ch_off, op.pass_group, op.groups, op.dilation, op.bias is None) == (case.in_off, case.out_off, case.pass_group, case.n + 1, case.d, not case.bias)


def test_exact_family_cannot_round_and_the_rounded_reference_sees_a_fault():
    for case in RC.all_cases(True)[::3]:
        feats, c = RC.plan(case, "bf16")
        assert np.array_equal(RC.evaluate(case, "bf16"), RC.evaluate(case, "bf16", rounding=False))      # rounding to bf16 changes nothing
        y = RC.chain(case, feats[4][:, case.in_off:case.in_off + case.channels], c, None)
        assert np.array_equal(y, np.round(y)) and np.abs(y).max() <= 196 and np.abs(y).max() >= (8 if case.n == 7 else 3)
        assert sorted(set(np.unique(c["weight"]))) == [-1.0, 0.0, 1.0]
    case = RC.all_cases(False)[5]
    a, b = RC.evaluate(case, "bf16", RC.SMALL), RC.evaluate(case, "bf16", RC.SMALL, order=1)
    errs = RC.errors(case, a, b)
    assert max(errs.values()) < 2.0 ** -6                                # another summation order: a few roundings on the other side at most
    assert max(RC.errors(case, RC.evaluate(case, "bf16", RC.SMALL, rounding=False), a).values()) > 1e-4    # the roundings are part of the contract


# ---- the kernel's resources and the C ABI

@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_res2n_chain_kernel_fits_its_registers_and_lds(tmp_path):
    """res2n_chain_kernel<ET> (kernels_res2n.hip): 4 accumulators, one branch's 12 weight fragments and the next group's 16 pieces per
    lane, designed for two waves per SIMD (at most 256 registers, no scratch); one 33 KiB image: several workgroups per CU."""
    blocks = re.split(r"remark: [^\n]*Function Name: ", device_asm("kernels_res2n", tmp_path / "res2n.s"))[1:]
    assert len(blocks) == 2 and all("res2n_chain_kernel" in b.split()[0] for b in blocks)
    for b in blocks:
        name = b.split()[0]
        assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, name
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, name
        assert int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1)) == 2, name
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        assert lds == (256 + 8) * 128 and lds <= 163840, name


def test_abi_entry_and_kernel_id_exist_in_binding_and_header(tmp_path):
    from libs.amd import capi
    header = open(os.path.join(helpers.REPO, "include", "asv_amd.h")).read()
    assert "asv_net_add_res2n" in capi.SYMBOLS and re.search(r"int\s+asv_net_add_res2n\(", header)
    assert capi.KERNEL_RES2N == 13 == int(re.search(r"#define\s+ASV_KERNEL_RES2N\s+(\d+)", header).group(1))
    assert capi.RES2N_TILE_ROWS == int(re.search(r"#define\s+ASV_RES2N_TILE_ROWS\s+(\d+)", header).group(1))
    body = re.search(r"typedef struct asv_res2n_desc \{(.*?)\} asv_res2n_desc_t;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in (d.strip() for d in body.split(";") if d.strip()):
        names = re.sub(r"^(const\s+)?\w+\s+", "", decl)                  # drop the type
        fields += [n.strip().lstrip("*") for n in names.split(",")]
    assert fields == [n for n, _ in capi.Res2nDesc._fields_]
    # sizeof(asv_res2n_desc_t) as the C compiler lays it out
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "asv_amd.h"\nint main(void) { printf("%zu\\n", sizeof(asv_res2n_desc_t)); return 0; }\n')
    exe = tmp_path / "sz"
    r = subprocess.run(["cc", "-I", os.path.join(helpers.REPO, "include"), "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert int(subprocess.run([str(exe)], capture_output=True, text=True).stdout) == C.sizeof(capi.Res2nDesc) == 72
    lib = capi.lib()
    assert hasattr(lib, "asv_net_add_res2n") and lib.asv_kernel_launch_count(capi.KERNEL_RES2N) >= 0
