# -*- coding:utf-8 -*-
"""Pre-norm encoder layer (reference libs/nnet/transformer/encoder_layer.py:11-138; eval: alpha = 1, the dropouts are identities):
    x = x + self_attn(norm1(x));   x = x + feed_forward(norm2(x))
The two residual additions run in the epilogues of linear_out and w_2; the LayerNorms are row ops."""

import torch

from libs.amd import ir as _ir
from .layer_norm import LayerNorm, emit_layer_norm


class TransformerEncoderLayer(torch.nn.Module):
    def __init__(self, size, self_attn, feed_forward, dropout_rate=0.1, layer_dropout=0., normalize_before=True, norm_type="layer_norm",
                 positionwise_layer_type="linear", concat_after=False):
        super(TransformerEncoderLayer, self).__init__()
        if norm_type != "layer_norm":
            raise NotImplementedError("norm_type=%r is not implemented on the MI355X path ('layer_norm' only)" % (norm_type,))
        if not normalize_before:
            raise NotImplementedError("normalize_before=False (post-norm layers) is not implemented on the MI355X path")
        if concat_after:
            raise NotImplementedError("concat_after=True is not implemented on the MI355X path")
        if positionwise_layer_type != "linear":
            raise NotImplementedError("positionwise_layer_type=%r is not implemented on the MI355X path ('linear' only)" % (positionwise_layer_type,))
        self.self_attn = self_attn
        self.feed_forward = feed_forward
        self.norm1 = LayerNorm(size)
        self.norm2 = LayerNorm(size)
        self.dropout = torch.nn.Dropout(dropout_rate)
        self.layer_dropout = layer_dropout
        self.size = size
        self.normalize_before = normalize_before
        self.concat_after = concat_after
        self.concat_linear = None
        self.positionwise_layer_type = positionwise_layer_type

    def forward(self, x, mask=None, pos_emb=None, mask_pad=None, warmup=1.0):
        if not isinstance(x, _ir.Sym):
            raise NotImplementedError("TransformerEncoderLayer.forward() on a torch tensor: eager forward is not part of asv-subtools_amd")
        n = emit_layer_norm(self.norm1, x)
        x = self.self_attn(n, n, n, mask, pos_emb, residual=x)
        x = self.feed_forward(emit_layer_norm(self.norm2, x), residual=x)
        return x, mask
