"""numpy interpreter of a traced transformer x-vector program (TEST INFRASTRUCTURE), float64, one chunk at a time.

It knows the ops such a program consists of - front_conv, the unpadded im2col, 1-tap tdnn layers on grids / sequences / pooled
rows, flatten, posenc, rowop, self_attention, pool, attpool - on its own tensor forms: a grid tensor is a map [T', W, C] (no pitch
rows), a frames / sequence tensor [T', C], a pooled tensor [1, C].  tests/ir_interp.py cannot run these programs: its grids follow
the ceil(T / 2) rule, the unpadded front's follow (T - 1) // 2.

`et` = 'bf16' | 'f16' restates what a 16-bit precision mode rounds, in float64 arithmetic: the features and every grid / frames /
sequence tensor are stored in the element type (ties to even), the weights of the layers on those tensors are rounded to it once
(biases, the first front stage's nine weights per channel and the positional table stay f32, as on the device), the attention
probabilities exp(s - max) are rounded for the second product while their sum is not; products are exact, sums f32-or-better, and
the pooled tail (statistics, norm_stats, the embedding layers) is f32 on the device and left unrounded here.  The cosine between
this evaluation and the reference's embeddings is the loss the number format alone causes on a fixture: the yardstick of the
device's 16-bit results (tests/test_gpu_transformer.py)."""

import numpy as np

from oracle import np_oracle as O
from rowop_cases import act_model, round_to, rowop_model


def valid_len(n, stages):
    for _ in range(stages):
        n = (n - 1) // 2
    return n


def attention64(q, k, v, heads, d_k, rnd=None):
    """[T, heads * d_k] each -> [T, heads * d_k]: per head softmax(q k^T / sqrt(d_k)) v in float64."""
    out = np.zeros_like(q)
    for h in range(heads):
        sl = slice(h * d_k, (h + 1) * d_k)
        s = (q[:, sl] @ k[:, sl].T) / np.sqrt(np.float64(d_k))
        p = np.exp(s - s.max(axis=1, keepdims=True))
        out[:, sl] = ((p if rnd is None else rnd(p)) @ v[:, sl]) / p.sum(axis=1, keepdims=True)
    return out


def run_graph(graph, feats, et="f64", ops=None):
    """feats [T, D] -> embedding [E] for ONE chunk."""
    rnd = (lambda a: np.asarray(a, dtype=np.float64)) if et in ("f64", "f32") else (lambda a: round_to(a, et).astype(np.float64))
    f64 = lambda a: None if a is None else np.asarray(a, dtype=np.float64)
    bufs = {0: rnd(feats)}
    utts = lambda tid: graph.is_utts(tid)
    store = lambda tid, val: val if utts(tid) else rnd(val)

    def get(v):
        return bufs[v.tid][..., v.ch_off:v.ch_off + v.channels]

    def put(v, val):
        if v.tid not in bufs:
            bufs[v.tid] = np.zeros(val.shape[:-1] + (graph.tensors[v.tid][1],), dtype=np.float64)
        bufs[v.tid][..., v.ch_off:v.ch_off + v.channels] = store(v.tid, val)

    for op in (graph.ops if ops is None else ops):
        if op.kind == "front_conv":
            x = get(op.inp)
            T1, F1 = valid_len(x.shape[0], 1), valid_len(x.shape[1], 1)
            z = np.zeros((T1, F1, op.weight.shape[0])) + f64(op.bias)
            for i in range(3):
                for j in range(3):
                    z += x[i:i + 2 * T1:2, j:j + 2 * F1:2, None] * f64(op.weight[:, 3 * i + j])
            put(op.out, np.maximum(z, 0))
        elif op.kind == "im2col":
            assert graph.is_valid_domain(op.inp.tid) and op.stride == 2 and getattr(op, "b", None) is None
            x = get(op.inp)
            T2, F2 = valid_len(x.shape[0], 1), valid_len(x.shape[1], 1)
            put(op.out, np.concatenate([x[dt:dt + 2 * T2:2, df:df + 2 * F2:2] for dt, df in op.taps], axis=2))
        elif op.kind == "flatten":
            x = get(op.inp)                                            # [T', W, C] -> column c * W + f
            put(op.out, x.transpose(0, 2, 1).reshape(x.shape[0], -1))
        elif op.kind == "tdnn":
            assert op.taps == [0] and op.inp2 is None
            w = f64(op.weight[:, :, 0 - op.w_left])
            z = get(op.inp) @ (w if utts(op.out.tid) else rnd(w)).T
            if op.bias is not None:
                z = z + f64(op.bias)
            if op.seg_bias is not None:
                z = z + get(op.seg_bias)
            s, t = (1, 0) if op.scale is None else (f64(op.scale), f64(op.shift))
            z = act_model(z * s + t, op.act1) if op.affine_first else act_model(z, op.act1) * s + t
            z = act_model(z, op.act2)
            if op.seg_scale is not None:
                z = z * get(op.seg_scale)
            if op.res is not None:
                z = z + get(op.res)
            put(op.out, z)
        elif op.kind == "posenc":
            x = get(op.inp)
            assert x.shape[0] < op.pe.shape[0]
            put(op.out, x * np.float64(op.scale) + f64(op.pe[:x.shape[0]]))
        elif op.kind == "rowop":
            put(op.out, rowop_model(get(op.inp), np.float64, act0=op.act0, slope0=op.slope0, ln=op.ln, eps=op.eps, gamma=op.gamma, beta=op.beta, act1=op.act1,
                                    slope1=op.slope1, scale0=op.scale0, shift0=op.shift0, scale1=op.scale1, shift1=op.shift1))
        elif op.kind == "self_attention":
            put(op.out, attention64(get(op.q), get(op.k), get(op.v), op.heads, op.d_k, None if et in ("f64", "f32") else rnd))
        elif op.kind == "pool":
            assert not getattr(op, "per_bin", False)
            x = get(op.inp)
            mean = x.mean(axis=0)
            if op.stddev:
                n = x.shape[0]
                with np.errstate(divide="ignore", invalid="ignore"):
                    var = ((x - mean) ** 2).sum(axis=0) / float(n - 1 if (op.unbiased == 2 or (op.unbiased == 1 and n > 1)) else n)
                std = np.sqrt(var + op.eps) if op.var_mode == 1 else np.sqrt(np.maximum(var, op.eps))
                put(op.out, np.concatenate([mean, std])[None, :])
            else:
                put(op.out, mean[None, :])
        elif op.kind == "attpool":
            assert not op.shared and op.group <= 1 and not op.softplus2 and op.prior_logit is None
            x, e = get(op.x), get(op.logits)
            a = np.exp(e - e.max(axis=0, keepdims=True))
            a = a / a.sum(axis=0, keepdims=True)
            mean = (a * x).sum(axis=0)
            put(op.out, np.concatenate([mean, np.sqrt(np.maximum((a * x * x).sum(axis=0) - mean * mean, op.eps))])[None, :])
        else:
            raise AssertionError("transformer_interp: unexpected op %s" % op.kind)
    return get(graph.output)[0]


def extract(graph, feats, max_chunk=300, et="f64", ops=None):
    """The chunked extraction of one utterance: ceil(T / max_chunk) near-equal chunks, frame-weighted mean (framework.py:34-47)."""
    return O.extract_embedding(lambda c: run_graph(graph, c, et, ops), feats, max_chunk, np.float64)
