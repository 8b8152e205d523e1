"""Multi-query multi-head attentive pooling (MQMHASP, reference libs/nnet/pooling.py:590-701) under ECAPA-TDNN, on the host: the
blueprint takes the reference's checkpoints, the traced program reproduces the embeddings the reference itself produced
(tests/gen_mqmha_golden.py), and the late graph pass turns the (head, query) poolings into one op - and nothing else."""

import os
import re

import numpy as np
import pytest

import helpers
import ir_interp
from helpers import rel_err

FIXTURES = {"ecapa_mqmha_roadmap": (2, 2, False), "ecapa_mqmha_shared": (4, 3, True), "ecapa_mqmha_q1": (1, 1, False)}   # heads, queries, shared
_traced = {}


def _trace(name):
    if name not in _traced:
        from libs.amd import ir
        g, sd, model = helpers.golden_model(name)                      # strict load: the reference's parameter names and shapes
        _traced[name] = (g, model, ir.trace(model, type(model).extract_embedding.__wrapped_body__, int(g["dim"])))
    return _traced[name]


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_blueprint_takes_the_reference_checkpoint(name):
    g, model, _ = _trace(name)
    _, shapes = helpers.load_golden(name)
    mine = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert list(mine) == list(shapes) and mine == shapes
    H, Q, shared = FIXTURES[name]
    mfa = model.mfa.affine.weight.shape[0]
    assert model.stats.get_output_dim() == 2 * Q * mfa == model.bn_stats.num_features
    assert any(k.startswith("stats.attention.0.") for k in mine)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_traced_program_reproduces_the_reference_on_cpu(name):
    g, model, graph = _trace(name)
    H, Q, shared = FIXTURES[name]
    att = [op for op in graph.ops if op.kind == "attpool"]
    assert len(att) == H * Q and all(op.shared == shared and op.eps == 1e-5 for op in att)
    assert all(op.logits.channels == (1 if shared else op.x.channels) for op in att)
    for (T, _), x, ref in zip(g["utts"], helpers.golden_feats(g), g["embeddings"]):
        err = rel_err(ir_interp.extract(graph, x), ref)
        print("%s T=%d: rel err %.3g" % (name, T, err))
        assert err < 1e-4, (name, int(T), err)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fused_pass_leaves_one_op(name):
    g, model, graph = _trace(name)
    H, Q, shared = FIXTURES[name]
    before = list(graph.ops)
    ops = graph.fused_mqpool_ops()
    assert graph.ops == before                                          # a late pass: the graph keeps its own list
    kinds = [op.kind for op in ops]
    assert kinds.count("mqattpool") == 1 and "attpool" not in kinds and "cat" not in kinds
    assert len(ops) == len(before) - H * Q + 1
    mq = ops[kinds.index("mqattpool")]
    Ch = mq.x.channels // H
    assert (mq.heads, mq.queries, mq.shared) == (H, Q, shared) and mq.logits.channels == H * Q * (1 if shared else Ch)
    assert mq.out.channels == 2 * Q * mq.x.channels and (mq.pair_stride, mq.std_off) == (2 * Ch, Ch)
    # every other op is the same object, in the same order
    assert [o for o in ops if o.kind != "mqattpool"] == [o for o in before if o.kind != "attpool"]
    if Q > 1:                                                           # more queries than the kernel is instantiated for: left alone
        assert graph.fused_mqpool_ops(max_queries=Q - 1) == before


def test_other_poolings_are_left_alone():
    from libs.amd import ir
    for name in ("snowdar_multires", "ecapa_c512_near_affine"):          # global heads; ECAPA's own per-channel attentive pooling
        g, sd, model = helpers.golden_model(name)
        graph = ir.trace(model, type(model).extract_embedding.__wrapped_body__, int(g["dim"]))
        assert any(op.kind == "attpool" for op in graph.ops)
        assert graph.fused_mqpool_ops() == graph.ops


def test_a_broken_set_is_left_alone():
    """One pair reading other logit columns, or one pair missing: not the pattern, nothing is fused."""
    from libs.amd import ir
    g, model, graph = _trace("ecapa_mqmha_roadmap")
    ops = list(graph.ops)
    idx = [i for i, op in enumerate(ops) if op.kind == "attpool"]
    assert graph.fused_mqpool_ops(ops[:idx[-1]] + ops[idx[-1] + 1:]) == ops[:idx[-1]] + ops[idx[-1] + 1:]
    o = ops[idx[1]]
    moved = ir.Op("attpool", o.out, **{k: v for k, v in o.__dict__.items() if k not in ("kind", "out")})
    moved.logits = ir.View(o.logits.tid, o.logits.ch_off + 16, o.logits.channels)
    swapped = ops[:idx[1]] + [moved] + ops[idx[1] + 1:]
    assert graph.fused_mqpool_ops(swapped) == swapped


def test_unsupported_configurations_raise_with_a_message():
    from libs.amd import ir
    from libs.nnet import pooling
    with pytest.raises(NotImplementedError, match="layer_norm"):
        pooling.MQMHASP(1536, num_head=2, norm_type="layer_norm")
    with pytest.raises(NotImplementedError, match="MQMHASP_Linear"):
        pooling.MQMHASP_Linear(1536)
    # 768 channels in 32 heads: heads of 24 channels are not 16-aligned views
    model = helpers.build_model("ecapa_tdnn_xvector.py", "ECAPA_TDNN(40,10,training=False,pooling='mqmha',pooling_params={'num_head':32,'hidden_size':8},"
                                "ecapa_params={'channels':512,'embd_dim':64,'mfa_conv':768})")
    with pytest.raises(ir.TraceError, match="multiple of 16"):
        ir.trace(model, type(model).extract_embedding.__wrapped_body__, 40)
    with pytest.raises(NotImplementedError, match="eager forward"):
        import torch
        pooling.MQMHASP(64, num_head=2)(torch.zeros(1, 64, 10))


def test_ecapa_passes_its_own_defaults_to_the_pooling():
    """ECAPA_TDNN.init pops `stddev` before it builds the pooling and supplies hidden_size 128 / time_attention True
    (reference ecapa_tdnn_xvector.py:213-217, 274, 290); num_head 4, num_q 2, share=True, two layers are MQMHASP's own."""
    model = helpers.build_model("ecapa_tdnn_xvector.py", "ECAPA_TDNN(40,10,training=False,pooling='mqmha',pooling_params={'stddev':False},"
                                "ecapa_params={'channels':512,'embd_dim':64,'mfa_conv':768})")
    s = model.stats
    assert (s.stddev, s.num_head, s.num_q, s.share, s.time_attention, s.hidden_size) == (True, 4, 2, True, True, 128)
    assert s.attention[0].weight.shape == (128 * 8, 3 * 768 // 4, 1) and s.attention[0].groups == 4
    assert s.attention[4].weight.shape == (8, 128, 1) and s.attention[4].groups == 8
    assert model.bn_stats.num_features == 4 * 768 and model.fc2.affine.weight.shape[1] == 4 * 768


def test_abi_entry_and_kernel_id_exist_in_binding_and_header():
    import ctypes as C
    from libs.amd import capi
    header = open(os.path.join(helpers.REPO, "include", "asv_amd.h")).read()
    assert "asv_net_add_mq_attentive_pool" in capi.SYMBOLS and re.search(r"int\s+asv_net_add_mq_attentive_pool\(", header)
    assert capi.KERNEL_MQ_ATTPOOL == 7 == int(re.search(r"#define\s+ASV_KERNEL_MQ_ATTPOOL\s+(\d+)", header).group(1))
    body = re.search(r"typedef struct asv_mq_attpool_desc \{(.*?)\} asv_mq_attpool_desc_t;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert fields == [n for n, _ in capi.MqAttPoolDesc._fields_]
    assert C.sizeof(capi.MqAttPoolDesc) == 4 * len(fields)              # 13 x int32 / uint32 + one float, no padding
    lib = capi.lib()
    assert lib.asv_kernel_launch_count(capi.KERNEL_MQ_ATTPOOL) >= 0 and lib.asv_kernel_launch_count(1 << 20) == 0     # no such id (8 - 12 are the grid convolutions')
