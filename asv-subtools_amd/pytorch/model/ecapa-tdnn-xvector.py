# -*- coding:utf-8 -*-
"""The ECAPA-TDNN blueprint of the reference's benchmark recipe (launcher/runEcapaXvector.py) for the MI355X extraction path.

Mirrors the public surface of the reference's model/ecapa-tdnn-xvector.py - class names, `ECAPA_TDNN.init` arguments and defaults,
sub-module names (hence state_dict keys: `layer2.0.conv.weight`, `layer2.1.convs.3.weight`, `layer2.1.bns.3.running_var`,
`layer2.3.linear1.weight`, ...), `extract_embedding` positions - so an `nnet.config` written by that recipe and its `*.params`
work unchanged.  It differs from model/ecapa_tdnn_xvector.py in every block:

  * raw Conv1d (no bias) -> ReLU -> BatchNorm1d bricks, C = 512 by default;
  * Res2 block: of the eight channel groups the first seven are convolved, y_i = BN(ReLU(conv_i(y_{i-1} + x_i))), the LAST passes through;
  * SE over two Linear layers (C -> C/4 -> C); the residual sums live in the top model;
  * a 3C -> 3C 1x1 convolution WITH bias -> ReLU -> BN in front of the pooling;
  * "ecpa-attentive" = tanh(linear1 x) -> linear2 -> softmax over frames, no global context, std = sqrt(clamp(., 1e-9)).

Poolings: "ecpa-attentive" (default), "attentive", "multi-head", "global-multi", "multi-resolution" through the libs.nnet classes
(whatever their constructors refuse with the reference's pooling defaults they refuse here), anything else = statistics pooling.

All modules are parameter holders whose forward() records fused ops for libasv_amd.so (libs/amd/ir.py holds the lowering: the
reference's own file traces to the same program through the handlers of the same names).
"""

import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, "subtools/pytorch")

import libs.support.utils as utils
from libs.nnet import *  # noqa: F401,F403
from libs.amd import ir as _ir


def _only_symbolic(x, who):
    if not isinstance(x, _ir.Sym):
        raise NotImplementedError("%s.forward() on a torch tensor: eager forward is not part of asv-subtools_amd" % who)


class Res2Conv1dReluBn(nn.Module):
    """`scale` channel groups of `width` channels: group i < scale - 1 feeds Conv1d (no bias) -> ReLU -> BN with the previous
    group's output added, the last group passes through.  inputs_dim == out_channels == channels."""
    _asv_amd_native = True

    def __init__(self, channels, kernel_size=1, stride=1, padding=0, dilation=1, bias=False, scale=4):
        super(Res2Conv1dReluBn, self).__init__()
        assert channels % scale == 0, "{} % {} != 0".format(channels, scale)
        self.scale = scale
        self.width = channels // scale
        self.nums = scale if scale == 1 else scale - 1
        self.convs = nn.ModuleList([nn.Conv1d(self.width, self.width, kernel_size, stride, padding, dilation, bias=bias) for _ in range(self.nums)])
        self.bns = nn.ModuleList([nn.BatchNorm1d(self.width) for _ in range(self.nums)])

    def forward(self, x):
        _only_symbolic(x, "Res2Conv1dReluBn")
        return _ir.MODULE_HANDLERS["Res2Conv1dReluBn"](self, x)


class Conv1dReluBn(nn.Module):
    """Conv1d (no bias by default) -> ReLU -> BatchNorm1d."""
    _asv_amd_native = True

    def __init__(self, inputs_dim, out_channels, kernel_size=1, stride=1, padding=0, dilation=1, bias=False):
        super(Conv1dReluBn, self).__init__()
        self.conv = nn.Conv1d(inputs_dim, out_channels, kernel_size, stride, padding, dilation, bias=bias)
        self.bn = nn.BatchNorm1d(out_channels)

    def forward(self, x):
        _only_symbolic(x, "Conv1dReluBn")
        return _ir.MODULE_HANDLERS["Conv1dReluBn"](self, x)


class SE_Connect(nn.Module):
    """Squeeze-excitation: time mean -> Linear -> ReLU -> Linear -> sigmoid -> channel scale."""
    _asv_amd_native = True

    def __init__(self, channels, s=4):
        super(SE_Connect, self).__init__()
        assert channels % s == 0, "{} % {} != 0".format(channels, s)
        self.linear1 = nn.Linear(channels, channels // s)
        self.linear2 = nn.Linear(channels // s, channels)

    def forward(self, x):
        _only_symbolic(x, "SE_Connect")
        return _ir.MODULE_HANDLERS["SE_Connect"](self, x)


def SE_Res2Block(channels, kernel_size, stride, padding, dilation, scale):
    """1x1 -> Res2 -> 1x1 -> SE; the residual connection is made by ECAPA_TDNN, not here."""
    return nn.Sequential(
        Conv1dReluBn(channels, channels, kernel_size=1, stride=1, padding=0),
        Res2Conv1dReluBn(channels, kernel_size, stride, padding, dilation, scale=scale),
        Conv1dReluBn(channels, channels, kernel_size=1, stride=1, padding=0),
        SE_Connect(channels))


class AttentiveStatsPool(nn.Module):
    """Attentive weighted mean and standard deviation pooling with per-channel weights."""
    _asv_amd_native = True

    def __init__(self, in_dim, bottleneck_dim):
        super(AttentiveStatsPool, self).__init__()
        self.linear1 = nn.Conv1d(in_dim, bottleneck_dim, kernel_size=1)
        self.linear2 = nn.Conv1d(bottleneck_dim, in_dim, kernel_size=1)

    def forward(self, x):
        _only_symbolic(x, "AttentiveStatsPool")
        return _ir.MODULE_HANDLERS["AttentiveStatsPool"](self, x)


class ECAPA_TDNN(TopVirtualNnet):
    def init(self, inputs_dim, num_targets, channels=512, embd_dim=192, aug_dropout=0., tail_dropout=0., training=True,
             extracted_embedding="near", mixup=False, mixup_alpha=1.0, pooling="ecpa-attentive", pooling_params={}, fc1=False,
             fc1_params={}, fc2_params={}, margin_loss=True, margin_loss_params={}, use_step=False, step_params={},
             transfer_from="softmax_loss"):
        default_pooling_params = {"num_head": 1, "hidden_size": 64, "share": True, "affine_layers": 1, "context": [0], "stddev": True,
                                  "temperature": False, "fixed": True}
        default_fc_params = {"nonlinearity": "relu", "nonlinearity_params": {"inplace": True}, "bn-relu": False, "bn": True,
                             "bn_params": {"momentum": 0.5, "affine": True, "track_running_stats": True}}
        pooling_params = utils.assign_params_dict(default_pooling_params, pooling_params)
        fc1_params = utils.assign_params_dict(default_fc_params, fc1_params)
        fc2_params = utils.assign_params_dict(default_fc_params, fc2_params)

        # training-only arguments (dropout, mixup, margin loss, step) are accepted and have no extraction counterpart
        self.use_step, self.step_params = use_step, step_params
        self.extracted_embedding = extracted_embedding
        self.inputs_dim = inputs_dim
        self.embd_dim = embd_dim

        self.layer1 = Conv1dReluBn(inputs_dim, channels, kernel_size=5, padding=2)
        self.layer2 = SE_Res2Block(channels, kernel_size=3, stride=1, padding=2, dilation=2, scale=8)
        self.layer3 = SE_Res2Block(channels, kernel_size=3, stride=1, padding=3, dilation=3, scale=8)
        self.layer4 = SE_Res2Block(channels, kernel_size=3, stride=1, padding=4, dilation=4, scale=8)
        cat_channels = channels * 3
        self.conv = nn.Conv1d(cat_channels, cat_channels, kernel_size=1)
        self.bn_conv = nn.BatchNorm1d(cat_channels)

        stddev = pooling_params.pop("stddev")
        stats_dim = cat_channels * 2
        if pooling == "attentive":
            self.stats = AttentiveStatisticsPooling(cat_channels, hidden_size=pooling_params["hidden_size"], context=pooling_params["context"], stddev=stddev)
        elif pooling == "ecpa-attentive":
            self.stats = AttentiveStatsPool(cat_channels, 128)
        elif pooling == "multi-head":
            self.stats = MultiHeadAttentionPooling(cat_channels, stddev=stddev, **pooling_params)
        elif pooling == "global-multi":
            self.stats = GlobalMultiHeadAttentionPooling(cat_channels, stddev=stddev, **pooling_params)
            stats_dim = cat_channels * 2 * pooling_params["num_head"]
        elif pooling == "multi-resolution":
            self.stats = MultiResolutionMultiHeadAttentionPooling(cat_channels, **pooling_params)
            stats_dim = cat_channels * 2 * pooling_params["num_head"]
        else:
            self.stats = StatisticsPooling(cat_channels, stddev=stddev)
        self.bn_stats = nn.BatchNorm1d(stats_dim)
        self.fc1 = ReluBatchNormTdnnLayer(stats_dim, embd_dim, **fc1_params) if fc1 else None
        self.fc2 = ReluBatchNormTdnnLayer(embd_dim if fc1 else cat_channels * 2, embd_dim, **fc2_params)
        self.tail_dropout = None
        if training:
            self.loss = MarginSoftmaxLoss(embd_dim, num_targets, **margin_loss_params) if margin_loss else SoftmaxLoss(embd_dim, num_targets)

    def _embed(self, x, position):
        out1 = self.layer1(x)
        out2 = self.layer2(out1) + out1
        out3 = self.layer3(out1 + out2) + out1 + out2
        out4 = self.layer4(out1 + out2 + out3) + out1 + out2 + out3
        out = torch.cat([out2, out3, out4], dim=1)
        out = self.bn_conv(F.relu(self.conv(out)))
        x = self.bn_stats(self.stats(out))
        if len(x.shape) != 3:
            x = x.unsqueeze(dim=2)
        if position == "far":
            assert self.fc1 is not None
            return self.fc1.affine(x)
        x = self.auto(self.fc1, x)
        if position == "near_affine":
            return self.fc2.affine(x)
        if position == "near":
            return self.fc2(x)
        raise TypeError("Expected far or near position, but got {}".format(position))

    @for_extract_embedding(maxChunk=10000, isMatrix=True)
    def extract_embedding(self, x):
        return self._embed(x, self.extracted_embedding)

    def embedding_dim(self):
        return self.embd_dim
