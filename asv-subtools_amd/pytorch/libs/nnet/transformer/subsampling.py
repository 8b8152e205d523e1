# -*- coding:utf-8 -*-
"""Input layers of the encoder (reference libs/nnet/transformer/subsampling.py:39-88, 91-141).

LinearNoSubsampling   Linear(idim, odim) per frame, then the positional encoding: one 1-tap layer on the frames domain.
Conv2dSubsampling4    the [T, F] features as a one-channel (time, frequency) image through Conv2d(1, d, 3, stride 2) -> ReLU ->
                      Conv2d(d, d, 3, stride 2) -> ReLU without padding, [B, d, T2, F2] -> [B, T2, d * F2] (column c * F2 + f),
                      Linear(d * F2, d), the positional encoding.  On the device: the first stage straight from the feature rows
                      (Graph.front_conv), the second as the unpadded stride-2 gather + a 1-tap layer with K = 9 d on the matrix
                      cores, then the grid flatten and a 1-tap layer on the sequence domain.  A chunk of T frames owns
                      T2 = ((T - 1) // 2 - 1) // 2 rows; T < 7 is refused (ValueError) before anything is launched.
"""

import numpy as np
import torch

from libs.amd import ir as _ir


def _np(t):
    return t.detach().cpu().numpy()


def _refuse_mlp_head(mlp_head):
    if mlp_head:
        raise NotImplementedError("mlp_head=True (a class token in front of the sequence) is not implemented on the MI355X path")


class LinearNoSubsampling(torch.nn.Module):
    def __init__(self, idim, odim, dropout_rate, mlp_head, pos_enc_class):
        super(LinearNoSubsampling, self).__init__()
        _refuse_mlp_head(mlp_head)
        self.out = torch.nn.Sequential(torch.nn.Linear(idim, odim))
        self.pos_enc = pos_enc_class
        self.subsampling_rate = 1
        self.mlp_head = mlp_head

    def forward(self, x, x_mask=None):
        if not isinstance(x, _ir.Sym):
            raise NotImplementedError("LinearNoSubsampling.forward() on a torch tensor: eager forward is not part of asv-subtools_amd")
        lin = self.out[0]
        if x.view.channels != lin.in_features:
            raise _ir.TraceError("LinearNoSubsampling expects %d input channels, got %d" % (lin.in_features, x.view.channels))
        y = _ir.Sym(x.graph, x.graph.tdnn(x.view, _np(lin.weight)[:, :, None], _np(lin.bias), [0], 0), 3)
        y, pos_emb = self.pos_enc(y)
        return y, pos_emb, x_mask


class Conv2dSubsampling4(torch.nn.Module):
    def __init__(self, idim, odim, dropout_rate, mlp_head, pos_enc_class):
        super(Conv2dSubsampling4, self).__init__()
        _refuse_mlp_head(mlp_head)
        self.conv = torch.nn.Sequential(torch.nn.Conv2d(1, odim, 3, 2), torch.nn.ReLU(), torch.nn.Conv2d(odim, odim, 3, 2), torch.nn.ReLU())
        self.out = torch.nn.Sequential(torch.nn.Linear(odim * (((idim - 1) // 2 - 1) // 2), odim))
        self.pos_enc = pos_enc_class
        self.subsampling_rate = 4
        self.mlp_head = mlp_head
        self.idim, self.odim = idim, odim

    def forward(self, x, x_mask=None):
        if not isinstance(x, _ir.Sym):
            raise NotImplementedError("Conv2dSubsampling4.forward() on a torch tensor: eager forward is not part of asv-subtools_amd")
        g = x.graph
        if x.view.tid != 0 or x.view.channels != self.idim or self.idim != g.feat_dim:
            raise _ir.TraceError("Conv2dSubsampling4 reads the feature matrix itself (%d bins), got %r" % (self.idim, x.view))
        d = self.odim
        if ((self.idim - 1) // 2 - 1) // 2 < 1:
            raise _ir.TraceError("Conv2dSubsampling4 over %d frequency bins: at least 7" % self.idim)
        c1, c2, lin = self.conv[0], self.conv[2], self.out[0]
        # Conv2d weights are [out, in, time, frequency] (the image is (time, frequency))
        y = g.front_conv(_np(c1.weight).reshape(d, 9), _np(c1.bias))
        taps = [(i, j) for i in range(3) for j in range(3)]
        cols = g.im2col(y, taps, 2, valid=True)                                  # column (3 i + j) * d + c
        w2 = np.ascontiguousarray(_np(c2.weight).transpose(0, 2, 3, 1).reshape(d, 9 * d))      # [out][(i, j, c)]
        y = g.tdnn(cols, w2[:, :, None], _np(c2.bias), [0], 0, act1="relu")
        y = g.flatten_grid(y)                                                    # [T2][c * F2 + f]
        y = _ir.Sym(g, g.tdnn(y, _np(lin.weight)[:, :, None], _np(lin.bias), [0], 0), 3)
        y, pos_emb = self.pos_enc(y)
        return y, pos_emb, x_mask
