# -*- coding:utf-8 -*-
"""A small x-vector blueprint whose layer options reach ReluBatchNormTdnnLayer UNFILTERED (TEST INFRASTRUCTURE).

The shipped snowdar / ECAPA / ResNet blueprints - the reference's and this package's alike - pass their layer options through
`assign_params_dict(defaults, options)`, whose defaults have no `ln_replace` key (and, in the snowdar blueprint, no
`negative_slope`): such options are dropped there without a word and never reach the layer.  Only the reference's Conformer
blueprint names `ln_replace` in its defaults.  This blueprint hands the dictionaries to the layers as they are, so that
LayerNorm in both orders, with and without its elementwise affine, on frame-level and on pooled tensors, can be recorded from
the reference's own layer classes (tests/gen_rowop_golden.py runs this file against the reference's libs.nnet) and from this
package's (tests/test_rowop_host.py, tests/test_gpu_rowop_models.py)."""

from libs.nnet import *  # noqa: F401,F403


class RowopXvector(TopVirtualNnet):
    """tdnn1-3 -> mean/std pooling -> tdnn6 -> tdnn7; the embedding is the output of the WHOLE tdnn7 layer."""

    def init(self, inputs_dim, num_targets, layer_params={}, tdnn6_params=None, tdnn7_params=None, training=False):
        self.inputs_dim = inputs_dim
        tdnn6_params = layer_params if tdnn6_params is None else tdnn6_params
        tdnn7_params = layer_params if tdnn7_params is None else tdnn7_params
        self.tdnn1 = ReluBatchNormTdnnLayer(inputs_dim, 512, [-2, -1, 0, 1, 2], **layer_params)
        self.tdnn2 = ReluBatchNormTdnnLayer(512, 512, [-2, 0, 2], **layer_params)
        self.tdnn3 = ReluBatchNormTdnnLayer(512, 1500, **layer_params)
        self.stats = StatisticsPooling(1500, stddev=True)
        self.tdnn6 = ReluBatchNormTdnnLayer(self.stats.get_output_dim(), 512, **tdnn6_params)
        self.tdnn7 = ReluBatchNormTdnnLayer(512, 192, **tdnn7_params)

    @for_extract_embedding(maxChunk=10000, isMatrix=True)
    def extract_embedding(self, inputs):
        x = self.tdnn3(self.tdnn2(self.tdnn1(inputs)))
        return self.tdnn7(self.tdnn6(self.stats(x)))
