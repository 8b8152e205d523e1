# -*- coding:utf-8 -*-
"""LayerNorm of the encoder (reference libs/nnet/transformer/layer_norm.py:57-80): the holder libs.nnet.components already has
(weight / bias, eps 1e-5, biased variance), normalised by the row op."""

from libs.amd import ir as _ir
from libs.nnet.components import LayerNorm  # noqa: F401


def emit_layer_norm(norm, x):
    """LayerNorm over the channels of the traced tensor `x` as one row op."""
    kw = dict(ln=True, eps=float(norm.eps))
    if norm.elementwise_affine:
        kw.update(gamma=norm.weight.detach().cpu().numpy(), beta=norm.bias.detach().cpu().numpy())
    return _ir.Sym(x.graph, x.graph.rowop(x.view, **kw), x.rank)
