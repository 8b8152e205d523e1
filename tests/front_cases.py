"""The cases of tests/test_gpu_subsample_front.py: the unpadded stride-2 front alone, on an exact-input family (TEST INFRASTRUCTURE).

Program: features [T, F] -> front_conv (1 -> 16 channels, 3 x 3, stride 2, unpadded, ReLU) -> im2col(valid) -> 1-tap layer with
K = 144 + ReLU (the second convolution) -> flatten -> 1-tap layer (the front's Linear, 64 outputs) -> posenc -> statistics pooling.

Exact inputs, as in conv_taps_cases.py: features, weights and biases are integers in {-1, 0, 1}; the second convolution has at
most two non-zero weights per (output channel, tap), the Linear one non-zero weight per output channel.  Stage-1 values are
integers in [0, 10], stage-2 values integers in [0, 181], the Linear's integers of magnitude <= 182: all exact in bf16 (8
significant bits), f16 and f32, and no f32 operation on the way can round.  Only the pooling rounds, so the bound is
conv_cases.TOL_EXACT.

The last 16 outputs of the Linear have no weights and no bias; the positional table adds the row's position t' to them (and
nothing to the others; scale 1).  Their pooled mean is (L - 1) / 2 and their std sqrt((L^2 - 1) / 12) for a segment of L rows:
the row count of every segment - L(T) = ((T - 1) // 2 - 1) // 2 - and the restart of the positions at every segment are read off
the output."""

import zlib

import numpy as np

WIDTHS = (7, 8, 11, 40, 80)
LENGTHS = [7, 8, 9, 10, 11, 64, 65]
CH = 16
OUT = 64
POS = 16                       # the last POS outputs carry the position
POOL_EPS = 1e-10


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def rows_of(T):
    return ((T - 1) // 2 - 1) // 2


def features(F, lengths=LENGTHS):
    return [_rng("front-x", F, T, i).randint(-1, 2, size=(T, F)).astype(np.float32) for i, T in enumerate(lengths)]


def weights(F):
    """(w1 [16, 9], b1 [16], w2 [16, 16, 3, 3] (out, in, time, frequency), b2 [16], w3 [64, 16 * F2], b3 [64])."""
    r = _rng("front-w", F)
    F2 = ((F - 1) // 2 - 1) // 2
    w1 = r.randint(-1, 2, size=(CH, 9)).astype(np.float32)
    b1 = r.randint(-1, 2, size=CH).astype(np.float32)
    w2 = np.zeros((CH, CH, 3, 3), dtype=np.float32)
    for co in range(CH):
        for i in range(3):
            for j in range(3):
                w2[co, r.choice(CH, size=2, replace=False), i, j] = r.choice([-1.0, 1.0], size=2)
    b2 = r.randint(-1, 2, size=CH).astype(np.float32)
    w3 = np.zeros((OUT, CH * F2), dtype=np.float32)
    b3 = np.zeros(OUT, dtype=np.float32)
    for o in range(OUT - POS):
        w3[o, r.randint(CH * F2)] = r.choice([-1.0, 1.0])
        b3[o] = r.randint(-1, 2)
    return w1, b1, w2, b2, w3, b3


def position_table(rows=32):
    pe = np.zeros((rows, OUT), dtype=np.float32)
    pe[:, OUT - POS:] = np.arange(rows, dtype=np.float32)[:, None]
    return pe


def build(F):
    from libs.amd import ir
    w1, b1, w2, b2, w3, b3 = weights(F)
    g = ir.Graph(F)
    y = g.front_conv(w1, b1)
    cols = g.im2col(y, [(i, j) for i in range(3) for j in range(3)], 2, valid=True)
    y = g.tdnn(cols, np.ascontiguousarray(w2.transpose(0, 2, 3, 1).reshape(CH, 9 * CH))[:, :, None], b2, [0], 0, act1="relu")
    y = g.tdnn(g.flatten_grid(y), w3[:, :, None], b3, [0], 0)
    y = g.posenc(y, 1.0, position_table())
    g.output = g.pool(y, stddev=True, unbiased=0, var_mode=0, eps=POOL_EPS)
    return g


def reference_torch64(x, F):
    """The same front written with torch's own unpadded convolutions in float64 (the reference's Conv2dSubsampling4 forward), then
    the positions and the statistics: [T, F] -> [2 * 64]."""
    import torch
    import torch.nn.functional as Fn
    w1, b1, w2, b2, w3, b3 = (torch.from_numpy(a).double() for a in weights(F))
    y = torch.from_numpy(np.asarray(x, np.float64))[None, None]                    # (b, c, t, f)
    y = torch.relu(Fn.conv2d(y, w1.reshape(CH, 1, 3, 3), b1, stride=2))
    y = torch.relu(Fn.conv2d(y, w2, b2, stride=2))
    b, c, t, f = y.shape
    y = y.transpose(1, 2).contiguous().view(t, c * f) @ w3.T + b3
    y = y + torch.from_numpy(position_table()).double()[:t]
    mean = y.mean(0)
    std = torch.sqrt(torch.clamp(((y - mean) ** 2).mean(0), min=POOL_EPS))
    return torch.cat([mean, std]).numpy()
