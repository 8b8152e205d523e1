# -*- coding:utf-8 -*-
"""RepVGG / RepSPK 2-D trunk of RepVggXvector: same class names, constructor arguments and state_dict keys as the reference
(/root/reference/pytorch/libs/nnet/repvgg.py: conv_bn 20-25, RepVGGBlock 29-171, RepSPKBlock 173-294, RepVGG 297-376,
repvgg_model_convert 378-386), in both forms - the training form (`rbr_dense.conv/bn`, `rbr_1x1.*` or `rbr_dense_dilation.*`,
`rbr_identity.*`) and `deploy=True` (`rbr_reparam.weight/bias`) - as parameter holders whose forward() records the trunk for
libasv_amd.so.

Every block is ONE convolution + bias + ReLU on the device: at trace time the eval BatchNorm of each branch is folded into its
kernel, and the branches - 3 x 3, 1 x 1 (RepVGG) or 3 x 3 at dilation 2 (RepSPK), identity BatchNorm - are merged into one K x K
kernel (K = 3 | 5) and one bias, in float64 (the reference's get_equivalent_kernel_bias, there in float32).  Taps whose weights are
all exactly zero are dropped: a RepSPK block keeps 17 of its 25 (the 3 x 3 at the centre, the 3 x 3 at dilation 2, one shared
centre tap).  The deploy form holds the merged kernel already; the same taps drop out, so both forms of a checkpoint give the same
program with weights equal to float32 rounding.

Lowering:
  K = 3 (RepVGG), stride 1 | 2    resnet.emit_conv_folded: the 9-tap layer / space-to-depth gather + 4-tap layer / im2col + GEMM of the
                                  ResNet trunk, on reach-1 grids (pitch = width + 1): existing kernels, every precision mode
  K = 5 (RepSPK), stride 1        Graph.grid_conv on a reach-2 grid (pitch = width + 2): the tap-table kernel, kernels_conv_taps.hip
  K = 5 (RepSPK), stride 2        the four-phase gather (Graph.im2col) + a 3 x 3 layer over 4 Cin channels on the output grid: input offset
                                  d in -2 .. 2 is phase (d & 1) of output offset (d - (d & 1)) / 2 = -1, -1, 0, 0, +1

Not implemented (raise): use_se, grouped convolutions (override_groups_map), more than 81 frequency bins with RepSPK blocks.
"""

import copy

import numpy as np
import torch
import torch.nn as nn

from libs.amd import ir as _ir
from libs.nnet import resnet as _resnet


def conv_bn(in_channels, out_channels, kernel_size, stride, padding, dilation=1, groups=1, norm_layer_params={}):
    result = nn.Sequential()
    result.add_module("conv", nn.Conv2d(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, stride=stride, padding=padding,
                                        dilation=dilation, groups=groups, bias=False))
    result.add_module("bn", nn.BatchNorm2d(num_features=out_channels, **norm_layer_params))
    return result


def _np64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _bn_scale_shift64(bn):
    """eval BatchNorm -> (scale, shift) in float64."""
    std = np.sqrt(_np64(bn.running_var) + float(bn.eps))
    gamma = _np64(bn.weight) if bn.affine else np.ones_like(std)
    beta = _np64(bn.bias) if bn.affine else np.zeros_like(std)
    return gamma / std, beta - _np64(bn.running_mean) * gamma / std


def _refuse(use_se, groups):
    if use_se:
        raise NotImplementedError("use_se=True: SE blocks in the RepVGG / RepSPK trunk are not implemented on the MI355X path")
    if groups != 1:
        raise NotImplementedError("override_groups_map / groups=%r: grouped convolutions in the RepVGG / RepSPK trunk are not implemented "
                                  "on the MI355X path (groups=1 only)" % (groups,))


class _RepBlock(nn.Module):
    """What RepVGGBlock and RepSPKBlock share: the fold and the lowering.  Subclasses set K (merged kernel size) and build the branches."""
    K = 3

    def folded_kernel_bias(self):
        """(kernel [Cout, Cin, K, K], bias [Cout]) in float64: get_equivalent_kernel_bias of the reference (repvgg.py:112-116, 226-230)."""
        K = self.K
        if self.rbr_reparam is not None:
            return _np64(self.rbr_reparam.weight), _np64(self.rbr_reparam.bias)
        dense = self.rbr_dense
        cout, cin = dense.conv.out_channels, dense.conv.in_channels
        kernel, bias = np.zeros((cout, cin, K, K), dtype=np.float64), np.zeros(cout, dtype=np.float64)
        c = K // 2
        s, t = _bn_scale_shift64(dense.bn)
        kernel[:, :, c - 1:c + 2, c - 1:c + 2] += _np64(dense.conv.weight) * s[:, None, None, None]
        bias += t
        second = self._second_branch()
        s, t = _bn_scale_shift64(second.bn)
        w2 = _np64(second.conv.weight) * s[:, None, None, None]
        if w2.shape[2] == 1:                             # RepVGG's 1 x 1
            kernel[:, :, c:c + 1, c:c + 1] += w2
        else:                                            # RepSPK's 3 x 3 at dilation 2: every other position of the 5 x 5
            kernel[:, :, ::2, ::2] += w2
        bias += t
        if self.rbr_identity is not None:
            s, t = _bn_scale_shift64(self.rbr_identity)
            kernel[np.arange(cout), np.arange(cin), c, c] += s
            bias += t
        return kernel, bias

    def folded_taps(self):
        """([(dt, df)], weight [Cout, Cin, taps] float64, bias [Cout] float64): the merged kernel without the taps whose weights are
        all exactly zero, frequency-major as the kernel's own index order.  Kernel axes: [.., frequency, time] (the input is [B, C, F, T])."""
        kernel, bias = self.folded_kernel_bias()
        c = self.K // 2
        live = [(j - c, i - c) for i in range(self.K) for j in range(self.K) if np.any(kernel[:, :, i, j] != 0.0)]
        if not live:
            live = [(0, 0)]
        w = np.stack([kernel[:, :, df + c, dt + c] for dt, df in live], axis=2)
        return live, w, bias

    def get_equivalent_kernel_bias(self):
        kernel, bias = self.folded_kernel_bias()
        return torch.from_numpy(kernel.astype(np.float32)), torch.from_numpy(bias.astype(np.float32))

    def switch_to_deploy(self):
        if self.rbr_reparam is not None:
            return
        kernel, bias = self.get_equivalent_kernel_bias()
        conv = self.rbr_dense.conv
        self.rbr_reparam = nn.Conv2d(in_channels=conv.in_channels, out_channels=conv.out_channels, kernel_size=self.K, stride=conv.stride,
                                     padding=self.K // 2, groups=conv.groups, bias=True)
        self.rbr_reparam.weight.data = kernel.to(conv.weight.device)
        self.rbr_reparam.bias.data = bias.to(conv.weight.device)
        for para in self.parameters():
            para.detach_()
        self.rbr_dense = None
        self._drop_second_branch()
        self.rbr_identity = None
        self.deploy = True

    def _stride(self):
        conv = self.rbr_reparam if self.rbr_reparam is not None else self.rbr_dense.conv
        if conv.stride[0] != conv.stride[1] or conv.stride[0] not in (1, 2):
            raise _ir.TraceError("%s: stride %r (1 or 2 in both axes)" % (type(self).__name__, conv.stride))
        return conv.stride[0]

    def forward(self, x):
        if not isinstance(x, _ir.Sym):
            raise NotImplementedError("%s.forward() on a torch tensor: eager forward is not part of asv-subtools_amd" % type(self).__name__)
        g = x.graph
        if g.grid_spec(x.view.tid) is None or x.rank != 4:
            raise _ir.TraceError("%s applied to a tensor that is not a [B, C, F, T] grid" % type(self).__name__)
        stride = self._stride()
        if self.K == 3:
            kernel, bias = self.folded_kernel_bias()
            return _resnet.emit_conv_folded(x, kernel, bias.astype(np.float32), stride, relu=True)
        if g.grid_reach(x.view.tid) < 2:
            raise _ir.TraceError("RepSPKBlock needs a reach-2 grid (pitch >= width + 2); RepVGG.forward() makes one from the input features")
        taps, w, bias = self.folded_taps()
        if stride == 1:
            return _ir.Sym(g, g.grid_conv(x.view, w.astype(np.float32), bias.astype(np.float32), taps, act="relu"), 4)
        # stride 2: the four phases (2 t' + pt, 2 f' + pf) side by side on the output grid ([rows'][(pt * 2 + pf) * Cin + c], one gather),
        # then input offset d = 2 a + p (a in -1 .. 1, p in 0 .. 1) is phase p of output offset a: a 3 x 3 layer over 4 Cin channels
        cout, cin = w.shape[0], w.shape[1]
        cols = g.im2col(x.view, [(0, 0), (0, 1), (1, 0), (1, 1)], 2)
        pitch = g.grid_spec(cols.tid)[3]
        offs = sorted(a * pitch + b for a in (-1, 0, 1) for b in (-1, 0, 1))
        dense = np.zeros((cout, 4 * cin, offs[-1] - offs[0] + 1), dtype=np.float64)
        used = set()
        for k, (dt, df) in enumerate(taps):
            pt, pf = dt & 1, df & 1
            a, b = (dt - pt) // 2, (df - pf) // 2
            ph = pt * 2 + pf
            dense[:, ph * cin:(ph + 1) * cin, a * pitch + b - offs[0]] = w[:, :, k]
            used.add(a * pitch + b)
        live = [o for o in offs if o in used]
        out = g.tdnn(cols, dense.astype(np.float32), bias.astype(np.float32), live, offs[0], act1="relu")
        g.ops[-1].alg_fraction = len(taps) / float(4 * len(live))      # (tap, phase) blocks that carry weights: FLOP accounting
        return _ir.Sym(g, out, 4)


class RepVGGBlock(_RepBlock):
    K = 3

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, padding_mode="zeros", deploy=False,
                 use_se=False, norm_layer_params={}):
        super(RepVGGBlock, self).__init__()
        _refuse(use_se, groups)
        assert kernel_size == 3 and padding == 1
        if dilation != 1 or padding_mode != "zeros":
            raise NotImplementedError("RepVGGBlock: dilation=%r / padding_mode=%r are not implemented on the MI355X path" % (dilation, padding_mode))
        self.deploy, self.groups, self.in_channels = deploy, groups, in_channels
        self.nonlinearity = nn.ReLU(inplace=True)
        self.se = nn.Identity()
        self.rbr_reparam = self.rbr_identity = self.rbr_dense = self.rbr_1x1 = None
        if deploy:
            self.rbr_reparam = nn.Conv2d(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, stride=stride, padding=padding,
                                         dilation=dilation, groups=groups, bias=True, padding_mode=padding_mode)
        else:
            self.rbr_identity = nn.BatchNorm2d(num_features=in_channels, **norm_layer_params) if out_channels == in_channels and stride == 1 else None
            self.rbr_dense = conv_bn(in_channels, out_channels, kernel_size, stride, padding, groups=groups, norm_layer_params=norm_layer_params)
            self.rbr_1x1 = conv_bn(in_channels, out_channels, 1, stride, padding - kernel_size // 2, groups=groups, norm_layer_params=norm_layer_params)

    def _second_branch(self):
        return self.rbr_1x1

    def _drop_second_branch(self):
        self.rbr_1x1 = None


class RepSPKBlock(_RepBlock):
    K = 5

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, branch_dilation=2, groups=1, padding_mode="zeros",
                 deploy=False, use_se=False, norm_layer_params={}):
        super(RepSPKBlock, self).__init__()
        _refuse(use_se, groups)
        assert kernel_size == 3 and padding == 1 and dilation == 1 and branch_dilation == 2
        if padding_mode != "zeros":
            raise NotImplementedError("RepSPKBlock: padding_mode=%r is not implemented on the MI355X path" % (padding_mode,))
        self.branch_dilation = branch_dilation
        self.depoly_kernel_size = (kernel_size - 1) * (branch_dilation - 1) + kernel_size
        self.deploy, self.groups, self.in_channels = deploy, groups, in_channels
        self.nonlinearity = nn.ReLU(inplace=True)
        self.se = nn.Identity()
        self.rbr_reparam = self.rbr_identity = self.rbr_dense = self.rbr_dense_dilation = None
        if deploy:
            self.rbr_reparam = nn.Conv2d(in_channels=in_channels, out_channels=out_channels, kernel_size=self.depoly_kernel_size, stride=stride,
                                         padding=self.branch_dilation, groups=groups, bias=True, padding_mode=padding_mode)
        else:
            self.rbr_identity = nn.BatchNorm2d(num_features=in_channels, **norm_layer_params) if out_channels == in_channels and stride == 1 else None
            self.rbr_dense = conv_bn(in_channels, out_channels, kernel_size, stride, padding, groups=groups, norm_layer_params=norm_layer_params)
            self.rbr_dense_dilation = conv_bn(in_channels, out_channels, kernel_size, stride, self.branch_dilation, dilation=self.branch_dilation,
                                              groups=groups, norm_layer_params=norm_layer_params)

    def _second_branch(self):
        return self.rbr_dense_dilation

    def _drop_second_branch(self):
        self.rbr_dense_dilation = None


class RepVGG(nn.Module):
    """stage0 + four stages of blocks (reference repvgg.py:297-376)."""

    def __init__(self, head_inplanes, block="RepVGG", num_blocks=[2, 4, 14, 1], strides=[1, 1, 2, 2, 2], base_width=64, width_multiplier=None,
                 override_groups_map=None, deploy=False, use_se=False, norm_layer_params={}):
        super(RepVGG, self).__init__()
        assert len(width_multiplier) == 4 and len(num_blocks) == 4 and len(strides) == 5
        if override_groups_map:
            raise NotImplementedError("override_groups_map=%r: grouped convolutions in the RepVGG / RepSPK trunk are not implemented on the "
                                      "MI355X path" % (override_groups_map,))
        _refuse(use_se, 1)
        width_multiplier = [w * (base_width / 64.) for w in width_multiplier]
        self.deploy, self.use_se, self.norm_layer_params = deploy, use_se, norm_layer_params
        self.override_groups_map = dict()
        self.block_name = block
        if block == "RepVGG":
            used_block = RepVGGBlock
        elif block == "RepSPK":
            used_block = RepSPKBlock
        else:
            raise TypeError("Do not support {} block.".format(block))
        self.downsample_multiple = 1
        for s in strides:
            self.downsample_multiple *= s
        self.in_planes = min(64, int(64 * width_multiplier[0]))
        self.stage0 = used_block(head_inplanes, out_channels=self.in_planes, kernel_size=3, stride=strides[0], padding=1, deploy=deploy, use_se=use_se,
                                 norm_layer_params=norm_layer_params)
        self.cur_layer_idx = 1
        self.stage1 = self._make_stage(used_block, int(64 * width_multiplier[0]), num_blocks[0], strides[1])
        self.stage2 = self._make_stage(used_block, int(128 * width_multiplier[1]), num_blocks[1], strides[2])
        self.stage3 = self._make_stage(used_block, int(256 * width_multiplier[2]), num_blocks[2], strides[3])
        self.stage4 = self._make_stage(used_block, int(512 * width_multiplier[3]), num_blocks[3], strides[4])
        self.output_planes = self.in_planes

    def _make_stage(self, block, planes, num_blocks, stride):
        blocks = []
        for s in [stride] + [1] * (num_blocks - 1):
            blocks.append(block(in_channels=self.in_planes, out_channels=planes, kernel_size=3, stride=s, padding=1, groups=1, deploy=self.deploy,
                                use_se=self.use_se, norm_layer_params=self.norm_layer_params))
            self.in_planes = planes
            self.cur_layer_idx += 1
        return nn.Sequential(*blocks)

    def get_downsample_multiple(self):
        return self.downsample_multiple

    def get_output_planes(self):
        return self.output_planes

    def forward(self, x):
        if not isinstance(x, _ir.Sym):
            raise NotImplementedError("RepVGG.forward() on a torch tensor: eager forward is not part of asv-subtools_amd")
        g = x.graph
        spec = g.grid_spec(x.view.tid)
        if spec is None or x.rank != 4:
            raise _ir.TraceError("RepVGG applied to a tensor that is not a [B, C, F, T] grid")
        if self.block_name == "RepSPK" and g.grid_reach(x.view.tid) < 2:
            # `x.unsqueeze(1)` made the one-channel grid of the ResNet trunk (pitch = width + 1); the 5 x 5 kernels need two zero
            # rows behind the bins of a frame and wider gaps: the same features on a reach-2 grid (the first grid has no reader left
            # and is dropped with its op by Graph.optimize)
            if spec[2] + 2 > 83:
                raise _ir.TraceError("RepSPK blocks over %d frequency bins: at most 81 (width + 2 <= 83, the widest window the tap-table "
                                     "kernel stages)" % spec[2])
            src = [op for op in g.ops if op.kind == "grid_input" and op.out.tid == x.view.tid]
            if not src:
                raise _ir.TraceError("RepVGG(block='RepSPK') must read the grid that x.unsqueeze(1) makes of the input features")
            x = _ir.Sym(g, g.grid_input(src[0].inp, reach=2), 4)
        for stage in (self.stage0, self.stage1, self.stage2, self.stage3, self.stage4):
            x = stage(x)
        return x


def repvgg_model_convert(model, save_path=None, do_copy=True):
    """The training form -> the deploy form (reference repvgg.py:378-386): every block's branches merged into `rbr_reparam`."""
    if do_copy:
        engines = model.__dict__.pop("_amd_engines", None)          # compiled engines hold device handles: not part of the copy
        try:
            new = copy.deepcopy(model)
        finally:
            if engines is not None:
                model.__dict__["_amd_engines"] = engines
        if engines is not None:
            new.__dict__["_amd_engines"] = {}
        model = new
    elif hasattr(model, "_invalidate_engines"):
        model._invalidate_engines()
    for module in model.modules():
        if hasattr(module, "switch_to_deploy"):
            module.switch_to_deploy()
    if hasattr(model, "deploy"):
        model.deploy = True
    if save_path is not None:
        torch.save(model.state_dict(), save_path)
    return model
