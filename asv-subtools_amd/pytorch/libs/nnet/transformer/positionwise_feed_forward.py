# -*- coding:utf-8 -*-
"""Position-wise feed-forward of the encoder layers (reference libs/nnet/transformer/positionwise_feed_forward.py:11-35):
w_2(act(w_1(x))).  relu / tanh / sigmoid run in w_1's GEMM epilogue, the other activations in the row op."""

import torch

from libs.amd import ir as _ir
from libs.nnet.activation import Nonlinearity, activation_name, HIP_ACTIVATIONS


class PositionwiseFeedForward(torch.nn.Module):
    def __init__(self, idim, hidden_units, dropout_rate, activation_type="relu", activation_balancer=False, re_scale=False):
        super(PositionwiseFeedForward, self).__init__()
        for name, value in (("activation_balancer", activation_balancer), ("re_scale", re_scale)):
            if value:
                raise NotImplementedError("%s=True is not implemented on the MI355X path" % name)
        self.w_1 = torch.nn.Linear(idim, hidden_units)
        self.w_2 = torch.nn.Linear(hidden_units, idim)
        self.dropout = torch.nn.Dropout(dropout_rate)
        self.activation = Nonlinearity(activation_type)
        self.balancer = None
        assert self.activation is not None

    def forward(self, x, residual=None):
        """`residual`: a traced tensor added to w_2's result in its epilogue."""
        if not isinstance(x, _ir.Sym):
            raise NotImplementedError("PositionwiseFeedForward.forward() on a torch tensor: eager forward is not part of asv-subtools_amd")
        g = x.graph
        act = activation_name(self.activation)
        if act == "gelu" and getattr(self.activation, "approximate", "none") != "none":
            raise _ir.TraceError("GELU(approximate=%r): the row op has the exact erf form only" % self.activation.approximate)
        np_ = lambda t: t.detach().cpu().numpy()
        h = g.tdnn(x.view, np_(self.w_1.weight)[:, :, None], np_(self.w_1.bias), [0], 0, act1=act if act in HIP_ACTIVATIONS else None)
        if act not in HIP_ACTIVATIONS:
            h = g.rowop(h, act0=act, slope0=float(getattr(self.activation, "negative_slope", 0.01)))
        out = g.tdnn(h, np_(self.w_2.weight)[:, :, None], np_(self.w_2.bias), [0], 0, res=None if residual is None else residual.view)
        return _ir.Sym(g, out, x.rank)
