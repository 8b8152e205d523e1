# -*- coding:utf-8 -*-
"""Transformer x-vector blueprint for the MI355X extraction path: an encoder over the frames of a chunk (libs/nnet/transformer/), a
swish + LayerNorm output layer, LayerNorm attentive statistics pooling and the embedding layers.

Public surface of the reference blueprint (pytorch/model/transformer_xvector.py:12-407 of the reference): class names, `init`
arguments and defaults, sub-module names (state_dict keys `transformer.*`, `transform_out.*`, `stats.*`, `fc1.*`, `fc2.*`), the
`extract_embedding` positions with the decorator's maxChunk=300, `extract_embedding_whole` and `embedding_dim`.  Built:
transformer_type="transformer" with the encoder options TransformerEncoder lists; "conformer" and "re_conformer" (the reference's
default!) are refused in the constructor, as is pooling stddev=False.  Training, forward(), wenet_transfer and
load_transform_state_dict's renaming are outside this package, as for every other blueprint.

The reference calls the model once per chunk, so the subsampling, the positions (they restart at 0), the attention and the pooling
all work per chunk: the engine's chunks are the segments every op here takes its rows from.
"""

import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, "subtools/pytorch")

import libs.support.utils as utils
from libs.amd import ir as _ir
from libs.nnet import *  # noqa: F401,F403
from libs.nnet.transformer.layer_norm import emit_layer_norm


class AttentiveStatsPool(nn.Module):
    """alpha = Conv1d(hidden -> C)(tanh(LayerNorm(relu(Conv1d(in -> hidden)(x_in))))), softmax over the frames per channel,
    mean = sum alpha x, std = sqrt(clamp(sum alpha x^2 - mean^2, 1e-5)), then norm_stats = LayerNorm(2 C) over [mean ; std]
    (reference transformer_xvector.py:12-90).  time_attention: x_in = [x ; m ; s] with m the time mean and
    s = sqrt(clamp(mean(x^2) - m^2, 1e-5)) - constant over the chunk, so that part of the first convolution is a per-chunk bias."""
    _asv_amd_native = True           # records itself: not one of ir.MODULE_HANDLERS' classes of this name

    def __init__(self, in_dim, hidden_size=128, time_attention=False, stddev=True):
        super(AttentiveStatsPool, self).__init__()
        if not stddev:
            raise NotImplementedError("pooling_params['stddev']=False is not implemented on the MI355X path")
        self.stddev = stddev
        self.output_dim = in_dim * 2
        self.time_attention = time_attention
        accept_dim = in_dim * 3 if time_attention else in_dim
        self.attention = nn.Sequential(
            nn.Conv1d(accept_dim, hidden_size, kernel_size=1),
            nn.ReLU(),
            LayerNorm(hidden_size, dim=1, eps=1e-5),
            nn.Tanh(),
            nn.Conv1d(hidden_size, in_dim, kernel_size=1),
        )
        self.norm_stats = LayerNorm(self.output_dim, dim=1)

    def forward(self, x, mask=None):
        if not isinstance(x, _ir.Sym):
            raise NotImplementedError("AttentiveStatsPool.forward() on a torch tensor: eager forward is not part of asv-subtools_amd")
        g, C = x.graph, x.view.channels
        conv1, norm, conv2 = self.attention[0], self.attention[2], self.attention[4]
        w1, b1 = conv1.weight.detach().cpu().numpy(), conv1.bias.detach().cpu().numpy()
        if self.time_attention:
            assert w1.shape[1] == 3 * C
            stats = g.pool(x.view, stddev=True, unbiased=0, var_mode=0, eps=1e-5)          # [m ; s], biased variance, clamped
            ctx = g.tdnn(stats, w1[:, C:, :], b1, [0], 0)                                   # W_m m + W_s s + b
            h = g.tdnn(x.view, w1[:, :C, :], None, [0], 0, seg_bias=ctx, act1="relu")
        else:
            h = g.tdnn(x.view, w1, b1, [0], 0, act1="relu")
        h = g.rowop(h, ln=True, eps=float(norm.eps), gamma=norm.weight.detach().cpu().numpy(), beta=norm.bias.detach().cpu().numpy(), act1="tanh")
        e = g.tdnn(h, conv2.weight.detach().cpu().numpy(), conv2.bias.detach().cpu().numpy(), [0], 0)
        pooled = _ir.Sym(g, g.attpool(x.view, e, eps=1e-5), 3)
        return emit_layer_norm(self.norm_stats, pooled)

    def get_output_dim(self):
        return self.output_dim


class TransformerXvector(TopVirtualNnet):
    """A transformer x-vector framework"""

    def init(self, inputs_dim, num_targets, embd_dim=256, training=True, extracted_embedding="near", mixup=False, mixup_alpha=1.0,
             pooling="ecpa-attentive", pooling_params={}, transformer_type="conformer", transformer_params={}, tansformer_out={}, fc1=False,
             fc1_params={}, fc2_params={}, margin_loss=True, margin_loss_params={}, lsm_weight=0.0, use_step=False, step_params={},
             transfer_from="softmax_loss", wenet_transfer=False):
        default_transformer_params = {
            "attention_dim": 256, "att_type": "multi", "attention_heads": 4, "gau_key": 64, "gau_units": 512, "num_blocks": 6,
            "dropout_rate": 0.1, "layer_dropout": 0., "positionwise_layer_type": "linear", "positional_dropout_rate": 0.1, "linear_units": 2048,
            "positionwise_conv_kernel_size": 3, "attention_dropout_rate": 0.0,
            "attention_norm_args": {"norm_method": "softmax", "train_len": 300.},
            "input_layer": "conv2d", "pos_enc_type": "abs_pos", "cnn_module_kernel": 15, "use_cnn_module": True, "cnn_module_norm": "layer_norm",
            "static_chunk_size": 0, "left_chunk_size": -1, "use_dynamic_chunk": False, "use_dynamic_left_chunk": False, "combiner_type": "norm",
            "convfnn_blocks": 0,
        }
        default_tansformer_out = {
            "out_dim": 1536, "nonlinearity": "swish", "nonlinearity_params": {"inplace": True}, "bn-relu": False, "bn": True, "ln_replace": True,
            "bn_params": {"momentum": 0.5, "affine": True, "track_running_stats": True},
        }
        default_pooling_params = {"hidden_size": 128, "time_attention": False, "stddev": True}
        default_fc_params = {
            "nonlinearity": "relu", "nonlinearity_params": {"inplace": True}, "bn-relu": False, "bn": True, "ln_replace": True,
            "bn_params": {"momentum": 0.5, "affine": True, "track_running_stats": True},
        }
        if training:
            raise NotImplementedError("TransformerXvector(training=True): training is outside asv-subtools_amd; construct with training=False")
        self.use_step = use_step
        self.step_params = step_params
        self.extracted_embedding = extracted_embedding
        self.inputs_dim = inputs_dim
        transformer_params = utils.assign_params_dict(default_transformer_params, transformer_params, support_unknow=True)
        tansformer_out = utils.assign_params_dict(default_tansformer_out, tansformer_out)
        pooling_params = utils.assign_params_dict(default_pooling_params, pooling_params)
        fc1_params = utils.assign_params_dict(default_fc_params, fc1_params)
        fc2_params = utils.assign_params_dict(default_fc_params, fc2_params)
        self.embd_dim = embd_dim

        if transformer_type == "transformer":
            transformer_backbone = TransformerEncoder
        elif transformer_type == "conformer":
            transformer_backbone = ConformerEncoder          # refuses (NotImplementedError): not built on this path
        elif transformer_type == "re_conformer":
            transformer_backbone = ReConformerEncoder        # likewise
        else:
            raise ValueError("unknown transformer_type: " + transformer_type)
        try:
            self.transformer = transformer_backbone(inputs_dim, **transformer_params)
        except NotImplementedError as e:
            if transformer_type != "transformer":
                raise NotImplementedError("transformer_type=%r: %s" % (transformer_type, e))
            raise

        out_dim = tansformer_out.pop("out_dim")
        self.transform_out = ReluBatchNormTdnnLayer(self.transformer.output_size(), out_dim, **tansformer_out)
        stddev = pooling_params.pop("stddev")
        if pooling != "ecpa-attentive":
            raise ValueError("Only supoort asp for conformer now.")
        self.stats = AttentiveStatsPool(out_dim, stddev=stddev, **pooling_params)
        self.fc1 = ReluBatchNormTdnnLayer(self.stats.get_output_dim(), embd_dim, **fc1_params) if fc1 else None
        self.fc2 = ReluBatchNormTdnnLayer(embd_dim if fc1 else self.stats.get_output_dim(), embd_dim, **fc2_params)

    def _embed(self, x, position):
        x, _ = self.transformer(x, None)               # rows are frames: the reference's transposes around the encoder are no-ops here
        x = self.transform_out(x)
        x = self.stats(x)
        if position == "far":
            assert self.fc1 is not None
            return self.fc1.affine(x)
        x = self.auto(self.fc1, x)
        if position == "near_affine":
            return self.fc2.affine(x)
        if position == "near":
            return self.fc2(x)
        raise TypeError("Expected far or near position, but got {}".format(position))

    @for_extract_embedding(maxChunk=300, isMatrix=True)
    def extract_embedding(self, x):
        return self._embed(x, self.extracted_embedding)

    def extract_embedding_whole(self, input, position="near", maxChunk=4000, isMatrix=True):
        """The reference's export interface (transformer_xvector.py:379-401): `position` in place of the model's
        extracted_embedding, chunks of at most maxChunk frames averaged by length.  Returns a 1-D CPU float32 tensor."""
        from libs.nnet.framework import _to_frames_matrix
        function = _WHOLE_BODIES.get(position)
        if function is None:
            raise TypeError("Expected far or near position, but got {}".format(position))
        was = self.extracted_embedding
        self.extracted_embedding = position                           # part of the engine cache key (framework.py)
        try:
            emb = self._amd_engine(function).extract_batch([_to_frames_matrix(input, isMatrix)], max_chunk=maxChunk)
        finally:
            self.extracted_embedding = was
        return emb[0]

    def embedding_dim(self):
        return self.embd_dim


# one body per position: the engine cache is keyed on the body
_WHOLE_BODIES = {
    "far": lambda self, x: self._embed(x, "far"),
    "near_affine": lambda self, x: self._embed(x, "near_affine"),
    "near": lambda self, x: self._embed(x, "near"),
}
