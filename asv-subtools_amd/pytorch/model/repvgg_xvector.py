# -*- coding:utf-8 -*-
"""RepVGG / RepSPK x-vector blueprint (a re-parameterised VGG-style 2-D trunk over fbank) for the MI355X extraction path.

Public surface of the reference blueprint (/root/reference/pytorch/model/repvgg_xvector.py:14-345): class name, `init` arguments and
defaults (RepSPK blocks [2, 4, 14, 1], base width 32), sub-module names (state_dict keys `repvgg.*`, `stats.*`, `fc1.*`, `fc2.*`) in
the training form and with `deploy=True`, the `extract_embedding` positions, `extract_embedding_whole`, `embedding_dim`,
`repvgg_model_convert` and the `auto_model` presets.  Every pooling the reference's constructor selects (repvgg_xvector.py:100-111):
statistics (pooled per frequency bin straight from the grid) and - over the [B, C*F', T'] reshape materialised once on the device -
attentive, multi-head, multi-resolution and LDE, routed as in resnet_xvector.py.
"""

import sys

import torch

sys.path.insert(0, "subtools/pytorch")

import libs.support.utils as utils
from libs.nnet import *  # noqa: F401,F403
from libs.nnet.repvgg import repvgg_model_convert  # noqa: F401  (the reference defines it in this file as well)


class RepVggXvector(TopVirtualNnet):
    """A repvgg vector framework"""

    def init(self, inputs_dim, num_targets, embd_dim=256, aug_dropout=0., tail_dropout=0., training=True, extracted_embedding="near",
             deploy=False, repvgg_config={}, pooling="statistics", pooling_params={}, fc1=False, fc1_params={}, fc2_params={}, margin_loss=False,
             margin_loss_params={}, use_step=False, step_params={}, adacos=False, transfer_from="softmax_loss"):
        default_repvgg_config = {
            "auto_model": False,
            "auto_model_name": "RepVGG_A1",
            "block": "RepSPK",
            "repvgg_params": {
                "num_blocks": [2, 4, 14, 1],
                "strides": [1, 1, 2, 2, 2],
                "base_width": 32,
                "width_multiplier": [1, 1, 1, 2.5],
                "norm_layer_params": {"momentum": 0.5, "affine": True},
                "override_groups_map": None,
                "use_se": False,
            }
        }
        fc_defaults = {"nonlinearity": "relu", "nonlinearity_params": {"inplace": True}, "bn-relu": False, "bn": True,
                       "bn_params": {"momentum": 0.5, "affine": True, "track_running_stats": True}}
        repvgg_config = utils.assign_params_dict(default_repvgg_config, repvgg_config)
        repvgg_params = dict(auto_model(repvgg_config["auto_model_name"]) if repvgg_config["auto_model"] else repvgg_config["repvgg_params"])
        repvgg_params["deploy"] = deploy
        repvgg_params["block"] = repvgg_config["block"]
        pooling_params = utils.assign_params_dict({"num_head": 1, "hidden_size": 64, "share": True, "affine_layers": 1, "context": [0],
                                                   "stddev": True, "temperature": False, "fixed": True}, pooling_params)
        fc1_params = utils.assign_params_dict(fc_defaults, fc1_params)
        fc2_params = utils.assign_params_dict(fc_defaults, fc2_params)

        self.extracted_embedding = extracted_embedding
        self.inputs_dim = inputs_dim
        self.repvgg = RepVGG(1, **repvgg_params)
        mult = self.repvgg.get_downsample_multiple()
        trunk_dim = (inputs_dim + mult - 1) // mult * self.repvgg.get_output_planes()
        stddev = pooling_params.pop("stddev")                            # the reference's selection, repvgg_xvector.py:100-111
        if pooling == "lde":
            self.stats = LDEPooling(trunk_dim, c_num=pooling_params["num_head"])
        elif pooling == "attentive":
            self.stats = AttentiveStatisticsPooling(trunk_dim, hidden_size=pooling_params["hidden_size"], context=pooling_params["context"], stddev=stddev)
        elif pooling == "multi-head":
            self.stats = MultiHeadAttentionPooling(trunk_dim, stddev=stddev, **pooling_params)
        elif pooling == "multi-resolution":
            self.stats = MultiResolutionMultiHeadAttentionPooling(trunk_dim, **pooling_params)
        else:
            self.stats = StatisticsPooling(trunk_dim, stddev=stddev)
        self.fc1 = ReluBatchNormTdnnLayer(self.stats.get_output_dim(), embd_dim, **fc1_params) if fc1 else None
        self.fc2 = ReluBatchNormTdnnLayer(embd_dim if fc1 else self.stats.get_output_dim(), embd_dim, **fc2_params)
        self.embd_dim = embd_dim
        self.deploy = deploy
        if training:
            self.loss = MarginSoftmaxLoss(embd_dim, num_targets, **margin_loss_params) if margin_loss else SoftmaxLoss(embd_dim, num_targets)

    def _embed(self, x, position):
        x = x.unsqueeze(1)                                            # [B, F, T] -> [B, 1, F, T]
        x = self.repvgg(x)
        x = x.reshape(x.shape[0], x.shape[1] * x.shape[2], x.shape[3])  # channel index c*F' + f
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

    @for_extract_embedding(maxChunk=10000, isMatrix=True)
    def extract_embedding(self, x):
        return self._embed(x, self.extracted_embedding)

    def extract_embedding_whole(self, input, position="near", maxChunk=4000, isMatrix=True):
        """The reference's export interface (repvgg_xvector.py:239-261): `position` in place of the model's extracted_embedding, chunks
        of at most maxChunk frames averaged by length.  Returns a 1-D CPU float32 tensor."""
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


def auto_model(model_name):
    """The reference's presets (repvgg_xvector.py:350-481).  The grouped (g2 / g4) and SE presets name options this path refuses."""
    optional_groupwise_layers = [2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 26]
    g2_map = {l: 2 for l in optional_groupwise_layers}
    g4_map = {l: 4 for l in optional_groupwise_layers}
    norm = {"momentum": 0.5, "affine": True}

    def preset(num_blocks, width_multiplier, groups=None, **extra):
        return dict({"num_blocks": num_blocks, "strides": [1, 1, 2, 2, 2], "base_width": 64, "width_multiplier": width_multiplier,
                     "norm_layer_params": dict(norm), "override_groups_map": groups}, **extra)

    a, b = [2, 4, 14, 1], [4, 6, 16, 1]
    model_params_dict = {
        "RepVGG_A0": preset(a, [0.75, 0.75, 0.75, 2.5]),
        "RepVGG_A1": preset(a, [1, 1, 1, 2.5]),
        "RepVGG_A2": preset(a, [1.5, 1.5, 1.5, 2.75]),
        "RepVGG_B0": preset(b, [1, 1, 1, 2.5], use_se=False),
        "RepVGG_B1": preset(b, [2, 2, 2, 4]),
        "RepVGG_B1g2": preset(b, [2, 2, 2, 4], g2_map),
        "RepVGG_B1g4": preset(b, [2, 2, 2, 4], g4_map),
        "RepVGG_B2": preset(b, [2.5, 2.5, 2.5, 5]),
        "RepVGG_B2g2": preset(b, [2.5, 2.5, 2.5, 5], g2_map),
        "RepVGG_B2g4": preset(b, [2.5, 2.5, 2.5, 5], g4_map),
        "RepVGG_B3": preset(b, [3, 3, 3, 5]),
        "RepVGG_B3g2": preset(b, [3, 3, 3, 5], g2_map),
        "RepVGG_B3g4": preset(b, [3, 3, 3, 5], g4_map),
        "RepVGG_D2se": preset([8, 14, 24, 1], [2.5, 2.5, 2.5, 5], use_se=True),
    }
    return model_params_dict[model_name]
