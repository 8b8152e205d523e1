# -*- coding:utf-8 -*-
"""Multi-head self-attention of the encoder layers (reference libs/nnet/transformer/attention.py:16-154; its score normalisation
AttentionNormalize, 640-716, with norm_method 'softmax'): q, k, v = Linear(x) with bias, head h = columns [h d_k, (h + 1) d_k),
softmax(q k^T / sqrt(d_k)) over the keys of the same chunk, the heads concatenated in that column order, linear_out.  A single
unpadded sequence has an all-ones mask, so the reference's -1e4 fill never acts.  On the device: the three projections as one GEMM
(Graph._merge_qkv_projections), the ragged attention kernel (kernels_attention.hip), linear_out with the layer's residual added in
its epilogue."""

import torch

from libs.amd import ir as _ir


def check_attention_norm_args(args):
    """The options of AttentionNormalize this path has: norm_method 'softmax' (`train_len` is accepted and unused, as in the reference)."""
    args = dict(args or {})
    method = args.get("norm_method", "softmax")
    if method != "softmax":
        raise NotImplementedError("attention_norm_args['norm_method']=%r is not implemented on the MI355X path ('softmax' only)" % (method,))
    for name in ("scale_adapt", "diag_mask", "g_sa"):
        if args.get(name, False):
            raise NotImplementedError("attention_norm_args[%r]=True is not implemented on the MI355X path" % name)
    unknown = sorted(set(args) - {"norm_method", "train_len", "scale_adapt", "diag_mask", "g_sa", "dim"})
    if unknown:
        raise TypeError("attention_norm_args: unknown option(s) %s" % unknown)
    if args.get("dim", -1) != -1:
        raise NotImplementedError("attention_norm_args['dim']=%r is not implemented on the MI355X path" % (args["dim"],))


class MultiHeadedAttention(torch.nn.Module):
    def __init__(self, n_head, n_feat, dropout_rate, add_t5rel_bias=False, conv_out=False, attention_norm_args={}, re_scale=False):
        super(MultiHeadedAttention, self).__init__()
        assert n_feat % n_head == 0
        for name, value in (("add_t5rel_bias", add_t5rel_bias), ("attention_conv_out", conv_out), ("re_scale", re_scale)):
            if value:
                raise NotImplementedError("%s=True is not implemented on the MI355X path" % name)
        check_attention_norm_args(attention_norm_args)
        self.d_k = n_feat // n_head
        self.h = n_head
        if self.d_k % 16 != 0 or self.d_k > 128:
            raise NotImplementedError("attention_dim / attention_heads = %d: the attention kernel takes head widths that are a multiple of 16 up to 128" % self.d_k)
        self.linear_q = torch.nn.Linear(n_feat, n_feat)
        self.linear_k = torch.nn.Linear(n_feat, n_feat)
        self.linear_v = torch.nn.Linear(n_feat, n_feat)
        self.linear_out = torch.nn.Linear(n_feat, n_feat)
        self.dropout = torch.nn.Dropout(p=dropout_rate)

    def forward(self, query, key, value, mask=None, pos_emb=None, residual=None):
        """`residual`: a traced tensor added to linear_out's result in its epilogue (the encoder layer's x + attention)."""
        if not isinstance(query, _ir.Sym):
            raise NotImplementedError("MultiHeadedAttention.forward() on a torch tensor: eager forward is not part of asv-subtools_amd")
        if key is not query or value is not query:
            raise _ir.TraceError("MultiHeadedAttention: self-attention only (query, key and value are one tensor)")
        g = query.graph
        def linear(m, x, res=None):
            return g.tdnn(x, m.weight.detach().cpu().numpy()[:, :, None], m.bias.detach().cpu().numpy(), [0], 0, res=res)

        q, k, v = (linear(m, query.view) for m in (self.linear_q, self.linear_k, self.linear_v))
        ctx = g.self_attention(q, k, v, self.h, self.d_k)
        return _ir.Sym(g, linear(self.linear_out, ctx, None if residual is None else residual.view), query.rank)
