# -*- coding:utf-8 -*-
"""Encoders of the transformer x-vector family (reference libs/nnet/transformer/encoder.py: BaseEncoder 48-420, TransformerEncoder
423-533, ConformerEncoder 536-, ReConformerEncoder 684-).  TransformerEncoder is built for the options listed in its docstring;
everything else raises NotImplementedError naming the option, in the constructor."""

import torch

from libs.amd import ir as _ir
from .attention import MultiHeadedAttention, check_attention_norm_args
from .embedding import PositionalEncoding, NoPositionalEncoding
from .encoder_layer import TransformerEncoderLayer
from .layer_norm import LayerNorm, emit_layer_norm
from .positionwise_feed_forward import PositionwiseFeedForward
from .subsampling import LinearNoSubsampling, Conv2dSubsampling4


def _refuse(name, value, why=""):
    raise NotImplementedError("%s=%r is not implemented on the MI355X path%s" % (name, value, why))


class TransformerEncoder(torch.nn.Module):
    """embed -> num_blocks pre-norm layers -> after_norm.  Implemented: input_layer 'linear' | 'conv2d'; pos_enc_type 'abs_pos' |
    'no_pos'; att_type 'multi' with softmax scores; positionwise_layer_type 'linear' with any activation of the layer factory;
    normalize_before=True; norm_type 'layer_norm'; combiner_type 'norm' | 'random_frame' | 'random_layer' (in eval all three return
    the last layer's output, encoder.py:917-918, 932-933, 975-976: no parameters, nothing to run)."""

    def __init__(self, idim, attention_dim=256, attention_heads=4, linear_units=2048, mlp_head=False, num_blocks=6, aux_layer_period=3, aux_layer_start=1,
                 dropout_rate=0.1, layer_dropout=0., positional_dropout_rate=0.1, attention_dropout_rate=0.0, attention_conv_out=False, attention_norm_args={},
                 input_layer="conv2d", pos_enc_type="abs_pos", rotary_value=True, rope_abs_plus=False, add_t5rel_bias=False, att_type="multi", gau_units=512,
                 gau_key=64, normalize_before=True, norm_type="layer_norm", concat_after=False, positionwise_layer_type="linear",
                 positionwise_conv_kernel_size=1, activation_type="relu", activation_balancer=False, static_chunk_size=0, left_chunk_size=-1,
                 use_dynamic_chunk=False, use_dynamic_left_chunk=False, combiner_type="norm", re_scale=False, convfnn_blocks=0, **args):
        super(TransformerEncoder, self).__init__()
        if pos_enc_type == "abs_pos":
            pos_enc = PositionalEncoding(attention_dim, positional_dropout_rate)
        elif pos_enc_type == "no_pos":
            pos_enc = NoPositionalEncoding(attention_dim, positional_dropout_rate)
        elif pos_enc_type in ("rel_pos", "rot_pos"):
            _refuse("pos_enc_type", pos_enc_type, " ('abs_pos' and 'no_pos' are)")
        else:
            raise ValueError("unknown pos_enc_layer: " + pos_enc_type)
        if input_layer in ("conv2d2", "re_conv2d", "conv2d6", "conv2d8"):
            _refuse("input_layer", input_layer, " ('linear' and 'conv2d' are)")
        if input_layer not in ("linear", "conv2d"):
            raise ValueError("unknown input_layer: " + input_layer)
        if att_type != "multi":
            _refuse("att_type", att_type, " ('multi' only)")
        if positionwise_layer_type != "linear":
            _refuse("positionwise_layer_type", positionwise_layer_type, " ('linear' only)")
        check_attention_norm_args(attention_norm_args)
        if combiner_type == "mfa":
            _refuse("combiner_type", combiner_type, " ('norm', 'random_frame' and 'random_layer' are: the last layer's output in eval)")
        assert combiner_type in ("norm", "random_frame", "random_layer"), "unknown combiner_type {}".format(combiner_type)
        if convfnn_blocks > 0:
            _refuse("convfnn_blocks", convfnn_blocks)
        for name, value in (("mlp_head", mlp_head), ("add_t5rel_bias", add_t5rel_bias), ("attention_conv_out", attention_conv_out), ("re_scale", re_scale),
                            ("activation_balancer", activation_balancer), ("concat_after", concat_after), ("use_dynamic_chunk", use_dynamic_chunk),
                            ("use_dynamic_left_chunk", use_dynamic_left_chunk)):
            if value:
                _refuse(name, value)
        if not normalize_before:
            _refuse("normalize_before", normalize_before)
        if norm_type != "layer_norm":
            _refuse("norm_type", norm_type, " ('layer_norm' only)")
        if static_chunk_size != 0:
            _refuse("static_chunk_size", static_chunk_size, " (full attention inside a chunk only)")
        if left_chunk_size != -1:
            _refuse("left_chunk_size", left_chunk_size, " (full attention inside a chunk only)")
        assert num_blocks > 0
        self.att_type, self.mlp_head, self.pos_enc_type = att_type, mlp_head, pos_enc_type
        front = LinearNoSubsampling if input_layer == "linear" else Conv2dSubsampling4
        self.embed = front(idim, attention_dim, dropout_rate, mlp_head, pos_enc)
        self.normalize_before = normalize_before
        self._output_size = attention_dim
        self.use_layer_norm = True
        self.after_norm = LayerNorm(attention_dim, eps=1e-5)
        self.static_chunk_size, self.left_chunk_size = static_chunk_size, left_chunk_size
        self.use_dynamic_chunk, self.use_dynamic_left_chunk = use_dynamic_chunk, use_dynamic_left_chunk
        self.encoders = torch.nn.ModuleList([
            TransformerEncoderLayer(attention_dim,
                                    MultiHeadedAttention(attention_heads, attention_dim, attention_dropout_rate, add_t5rel_bias, attention_conv_out,
                                                         attention_norm_args, re_scale),
                                    PositionwiseFeedForward(attention_dim, linear_units, dropout_rate, activation_type, activation_balancer, re_scale),
                                    dropout_rate, layer_dropout, normalize_before, norm_type, positionwise_layer_type, concat_after)
            for _ in range(num_blocks)])

    def output_size(self):
        return self._output_size

    def forward(self, xs, xs_lens=None, decoding_chunk_size=-1, decoding_left_chunk_size=-2, warmup=1.0):
        """xs: the traced [1, F, T] feature tensor (rows are frames: the reference's transposes are no-ops in the row layout).
        Returns (encoded [1, attention_dim, T'], None)."""
        if not isinstance(xs, _ir.Sym):
            raise NotImplementedError("TransformerEncoder.forward() on a torch tensor: eager forward is not part of asv-subtools_amd")
        xs, pos_emb, _ = self.embed(xs, None)
        for layer in self.encoders:
            xs, _ = layer(xs, None, pos_emb)
        return emit_layer_norm(self.after_norm, xs), None


def _not_built(name, where):
    class _Refusing(torch.nn.Module):
        def __init__(self, *args, **kwargs):
            raise NotImplementedError("%s (reference libs/nnet/transformer/%s) is not implemented on the MI355X path: transformer_type='transformer' "
                                      "(TransformerEncoder) is" % (name, where))
    _Refusing.__name__ = _Refusing.__qualname__ = name
    return _Refusing


ConformerEncoder = _not_built("ConformerEncoder", "encoder.py:536-681")
ReConformerEncoder = _not_built("ReConformerEncoder", "encoder.py:684-831")
