"""The cases of tests/test_gpu_attention_kernel.py: the self-attention op alone (TEST INFRASTRUCTURE, shared with the host test).

Program: features -> ONE 1-tap layer producing [q | k | v] -> self_attention -> statistics pooling (mean | std over the rows of a
segment, biased variance, floor 1e-10), run through Engine.  The features are integers in {-1, 0, 1} on 8 channels, the
projection weights integers / 2 (q, k) and / 4 (v), no bias: every q, k and v value is a multiple of 1/4 of magnitude <= 4, exact in
bf16, f16 and f32, and the layer that produces them cannot round in any mode.  What is measured is therefore the attention kernel
(and the pooling kernel's f32 sums, which have their own test) and nothing in front of it.  Scores q.k / sqrt(d_k) have a standard
deviation near 1: a softmax that is neither uniform nor one-hot.

Reference: the same program in float64 (numpy).  Yardstick: the same computation in float32 torch on CPU - softmax(q k^T /
sqrt(d_k)) v, then the statistics - and, for a 16-bit mode, with what that mode rounds besides: the probabilities to the element
type in front of the second product and the attention output where it is stored.  The error of the yardstick against float64 is
what the number formats cost; the device is allowed 4 x that for its different summation order and its exp."""

import zlib

import numpy as np

LENGTHS = [1, 2, 63, 64, 65, 130]
FEAT_DIM = 8
POOL_EPS = 1e-10
HEADS = (1, 4)
D_KS = (16, 64, 128)
ELEM_TYPES = ("bf16", "f16", "f32")


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def features(lengths=LENGTHS, seed=0):
    return [_rng("attn-x", T, i, seed).randint(-1, 2, size=(T, FEAT_DIM)).astype(np.float32) for i, T in enumerate(lengths)]


def weights(heads, d_k):
    n = heads * d_k
    r = _rng("attn-w", heads, d_k)
    w = r.randint(-1, 2, size=(3 * n, FEAT_DIM)).astype(np.float32)
    w[:2 * n] /= 2.0
    w[2 * n:] /= 4.0
    return w


def build(heads, d_k):
    """The traced program (libs.amd.ir.Graph) of one case."""
    from libs.amd import ir
    n = heads * d_k
    g = ir.Graph(FEAT_DIM)
    qkv = g.tdnn(g.full_view(0), weights(heads, d_k)[:, :, None], None, [0], 0)
    att = g.self_attention(ir.View(qkv.tid, 0, n), ir.View(qkv.tid, n, n), ir.View(qkv.tid, 2 * n, n), heads, d_k)
    g.output = g.pool(att, stddev=True, unbiased=0, var_mode=0, eps=POOL_EPS)
    return g


def _chunks(x, max_chunk):
    T = x.shape[0]
    n = -(-T // max_chunk)
    split = T // n
    return [x[i * split:(i + 1) * split if i < n - 1 else T] for i in range(n)]


def reference64(x, heads, d_k, max_chunk=1 << 30):
    """[T, 8] -> [2 heads d_k] in float64, chunked like the library (frame-weighted mean of the chunks)."""
    import transformer_interp as TI
    w = weights(heads, d_k).astype(np.float64)
    n = heads * d_k
    out, tot = 0.0, 0
    for c in _chunks(np.asarray(x, np.float64), max_chunk):
        qkv = c @ w.T
        o = TI.attention64(qkv[:, :n], qkv[:, n:2 * n], qkv[:, 2 * n:], heads, d_k)
        mean = o.mean(0)
        std = np.sqrt(np.maximum(((o - mean) ** 2).mean(0), POOL_EPS))
        out, tot = out + c.shape[0] * np.concatenate([mean, std]), tot + c.shape[0]
    return out / tot


def yardstick32(x, heads, d_k, et, max_chunk=1 << 30):
    """The same in float32 torch on CPU, with the roundings of the 16-bit mode `et` ('f32': none)."""
    import torch
    dt = {"bf16": torch.bfloat16, "f16": torch.float16}.get(et)
    rnd = (lambda t: t) if dt is None else (lambda t: t.to(dt).float())
    w = torch.from_numpy(weights(heads, d_k))
    n = heads * d_k
    out, tot = 0.0, 0
    for c in _chunks(np.asarray(x, np.float32), max_chunk):
        qkv = torch.from_numpy(c) @ w.T                                # exact: see the module docstring
        o = torch.zeros(c.shape[0], n)
        for h in range(heads):
            sl = slice(h * d_k, (h + 1) * d_k)
            p = torch.softmax((qkv[:, sl] @ qkv[:, n:2 * n][:, sl].T) / torch.sqrt(torch.tensor(float(d_k))), dim=1)
            o[:, sl] = rnd(p) @ qkv[:, 2 * n:][:, sl]
        o = rnd(o)
        mean = o.mean(0)
        std = torch.sqrt(torch.clamp(((o - mean) ** 2).mean(0), min=POOL_EPS))
        out, tot = out + c.shape[0] * torch.cat([mean, std]).double().numpy(), tot + c.shape[0]
    return out / tot


def block_err(got, ref):
    """Largest error of the mean block and of the std block, each relative to the block's largest reference value; over all rows."""
    got, ref = np.atleast_2d(np.asarray(got, np.float64)), np.atleast_2d(np.asarray(ref, np.float64))
    n = ref.shape[1] // 2
    return max(float(np.abs(got[:, s] - ref[:, s]).max() / max(np.abs(ref[:, s]).max(), 1e-30)) for s in (slice(0, n), slice(n, 2 * n)))
