# -*- coding:utf-8 -*-
"""Activation factory (reference libs/nnet/activation.py:69-94).  relu / tanh / sigmoid run inside the GEMM epilogues;
the other six run in the row op (csrc/kernels_rowop.hip, asv_net_add_rowop)."""

import torch

HIP_ACTIVATIONS = ("relu", "tanh", "sigmoid")                                              # the GEMM epilogues'
ROWOP_ACTIVATIONS = ("leaky_relu", "selu", "mish", "swish", "gelu", "double_swish")        # the row op's


def _eager_unsupported(name):
    raise NotImplementedError("%s.forward() on a torch tensor: eager forward is not part of asv-subtools_amd; the module is a "
                              "marker for the recorder (model.extract_embedding runs the HIP row op)" % name)


class Mish(torch.nn.Module):
    """x * tanh(softplus(x)) (reference activation.py:13-21).  Marker module: no parameters, no eager forward."""

    def forward(self, inputs):
        _eager_unsupported("Mish")


class DoubleSwish(torch.nn.Module):
    """x * sigmoid(x - 1) (reference activation.py:58-66).  Marker module: no parameters, no eager forward."""

    def forward(self, x):
        _eager_unsupported("DoubleSwish")


def Nonlinearity(nonlinearity="relu", inplace=True, negative_slope=0.01):
    """Returns a torch module used as a *marker* (its class tells the recorder which activation to emit) or None for
    '' / None / False.  'gelu': the reference calls torch.nn.GELU(inplace=...), which torch rejects (TypeError), so the
    reference cannot build it; here it is torch.nn.GELU(), the exact erf form (the row op)."""
    if nonlinearity == "relu":
        return torch.nn.ReLU(inplace=inplace)
    if nonlinearity == "leaky_relu":
        return torch.nn.LeakyReLU(inplace=inplace, negative_slope=negative_slope)
    if nonlinearity == "selu":
        return torch.nn.SELU(inplace=inplace)
    if nonlinearity == "mish":
        return Mish()
    if nonlinearity == "tanh":
        return torch.nn.Tanh()
    if nonlinearity == "sigmoid":
        return torch.nn.Sigmoid()
    if nonlinearity == "swish":
        return torch.nn.SiLU()
    if nonlinearity == "gelu":
        return torch.nn.GELU()
    if nonlinearity == "double_swish":
        return DoubleSwish()
    if nonlinearity == "" or nonlinearity is None or nonlinearity is False:
        return None
    raise ValueError("Do not support {0} nonlinearity now.".format(nonlinearity))


def activation_name(module):
    """Marker module -> activation name (HIP_ACTIVATIONS: an epilogue's; ROWOP_ACTIVATIONS: the row op's)."""
    if module is None:
        return None
    for cls, name in ((torch.nn.ReLU, "relu"), (torch.nn.Tanh, "tanh"), (torch.nn.Sigmoid, "sigmoid"), (torch.nn.LeakyReLU, "leaky_relu"),
                      (torch.nn.SELU, "selu"), (Mish, "mish"), (torch.nn.SiLU, "swish"), (torch.nn.GELU, "gelu"), (DoubleSwish, "double_swish")):
        if isinstance(module, cls):
            return name
    raise NotImplementedError("activation module %r has no HIP implementation" % (module,))
