"""numpy interpreter of the programs the x-vector family records once its layers use the row op (TEST INFRASTRUCTURE): the op
kinds those graphs contain - 'tdnn', the plain 'pool' and 'rowop' - and nothing else.  The TDNN and pooling arithmetic is
tests/ir_interp.py's (imported, not edited); the row op is tests/rowop_cases.py's model."""

import numpy as np

import ir_interp
import rowop_cases as RC
from oracle import np_oracle as O

ROWOP_FIELDS = ("act0", "slope0", "ln", "eps", "gamma", "beta", "act1", "slope1", "scale0", "shift0", "scale1", "shift1")


def run_graph(graph, feats, dtype=np.float32):
    """feats [T, D] -> embedding [E] for one utterance segment."""
    feats = np.asarray(feats, dtype=dtype)
    T = feats.shape[0]
    bufs = {0: feats}

    def get(v):
        return bufs[v.tid][:, v.ch_off:v.ch_off + v.channels]

    def put(v, val):
        if v.tid not in bufs:
            bufs[v.tid] = np.zeros((T if graph.domain(v.tid) == 0 else 1, graph.tensors[v.tid][1]), dtype=dtype)
        bufs[v.tid][:, v.ch_off:v.ch_off + v.channels] = val

    for op in graph.ops:
        if op.kind == "tdnn":
            assert op.inp2 is None and op.seg_bias is None and op.seg_scale is None and op.res is None and op.act2 is None
            z = ir_interp._tdnn_general(get(op.inp), op, dtype)
            s = 1 if op.scale is None else op.scale.astype(dtype)
            t = 0 if op.shift is None else op.shift.astype(dtype)
            z = ir_interp._act(z * s + t, op.act1) if op.affine_first else ir_interp._act(z, op.act1) * s + t
            put(op.out, z.astype(dtype))
        elif op.kind == "pool":
            assert not getattr(op, "per_bin", False) and op.stddev
            x = get(op.inp)
            mean = x.mean(axis=0, dtype=dtype)
            n = x.shape[0]
            counts = n - 1 if (op.unbiased == 2 or (op.unbiased == 1 and n > 1)) else n
            var = ((x - mean) ** 2).sum(axis=0, dtype=dtype) / dtype(counts)
            std = np.sqrt(var + dtype(op.eps)) if op.var_mode == 1 else np.sqrt(np.maximum(var, dtype(op.eps)))
            put(op.out, np.concatenate([mean, std])[None, :])
        elif op.kind == "rowop":
            put(op.out, RC.rowop_model(get(op.inp), dtype, **{k: getattr(op, k) for k in ROWOP_FIELDS}))
        else:
            raise AssertionError("unexpected op %s" % op.kind)
    return get(graph.output)[0]


def extract(graph, feats, max_chunk=10000, dtype=np.float32):
    return O.extract_embedding(lambda c: run_graph(graph, c, dtype), feats, max_chunk, dtype)
