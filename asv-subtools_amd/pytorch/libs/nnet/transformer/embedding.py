# -*- coding:utf-8 -*-
"""Positional encodings of the encoder front (reference libs/nnet/transformer/embedding.py:24-76, 129-150).  Neither has
parameters or buffers in the state dict: the sinusoid table is an attribute, rebuilt here on the host exactly as the reference
builds it (float32 torch, max_len 5000) and uploaded with the program."""

import math

import torch

from libs.amd import ir as _ir


class PositionalEncoding(torch.nn.Module):
    """x * sqrt(d_model) + pe[t]; pe[t, 2i] = sin(t * exp(-2i ln(10000) / d)), pe[t, 2i + 1] = cos(same).  Positions restart at 0 in
    every chunk; a chunk must have fewer than max_len rows (the reference asserts it; the library refuses the batch)."""

    def __init__(self, d_model, dropout_rate, att_h=4, rope_abs_plus=False, max_len=5000, reverse=False):
        super(PositionalEncoding, self).__init__()
        self.d_model = d_model
        self.xscale = math.sqrt(self.d_model)
        self.dropout = torch.nn.Dropout(p=dropout_rate)
        self.max_len = max_len
        pe = torch.zeros(self.max_len, self.d_model)
        position = torch.arange(0, self.max_len, dtype=torch.float32).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, self.d_model, 2, dtype=torch.float32) * -(math.log(10000.0) / self.d_model))
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        self.pe = pe.unsqueeze(0)

    def forward(self, x, offset=0):
        if not isinstance(x, _ir.Sym):
            raise NotImplementedError("PositionalEncoding.forward() on a torch tensor: eager forward is not part of asv-subtools_amd")
        if offset != 0:
            raise NotImplementedError("PositionalEncoding(offset=%r): streaming offsets are not implemented on the MI355X path" % (offset,))
        out = x.graph.posenc(x.view, self.xscale, self.pe[0].numpy())
        return _ir.Sym(x.graph, out, x.rank), None


class NoPositionalEncoding(torch.nn.Module):
    """The input as it is - unscaled, as in the reference."""

    def __init__(self, d_model, dropout_rate, att_h=4, rope_abs_plus=False):
        super(NoPositionalEncoding, self).__init__()
        self.d_model = d_model
        self.dropout = torch.nn.Dropout(p=dropout_rate)

    def forward(self, x, offset=0):
        if not isinstance(x, _ir.Sym):
            raise NotImplementedError("NoPositionalEncoding.forward() on a torch tensor: eager forward is not part of asv-subtools_amd")
        return x, None
