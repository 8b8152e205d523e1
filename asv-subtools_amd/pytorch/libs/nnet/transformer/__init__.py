# -*- coding:utf-8 -*-
"""The encoder package of the transformer x-vector family (reference libs/nnet/transformer/): parameter holders with the
reference's class names, constructor arguments and state_dict keys whose forward() records the encoder for libasv_amd.so.

Built: TransformerEncoder (pre-norm layers of multi-head self-attention + position-wise feed-forward) behind LinearNoSubsampling
or Conv2dSubsampling4, with PositionalEncoding / NoPositionalEncoding.  ConformerEncoder and ReConformerEncoder exist as names that
refuse; every option of the built classes that is not implemented raises NotImplementedError naming it.  As the reference does,
`from libs.nnet import *` gets the names of __all__ only."""

__all__ = ["TransformerEncoder", "ConformerEncoder", "MultiHeadedAttention", "LayerNorm", "ReConformerEncoder"]

from .layer_norm import LayerNorm  # noqa: F401
from .embedding import PositionalEncoding, NoPositionalEncoding  # noqa: F401
from .subsampling import LinearNoSubsampling, Conv2dSubsampling4  # noqa: F401
from .attention import MultiHeadedAttention  # noqa: F401
from .positionwise_feed_forward import PositionwiseFeedForward  # noqa: F401
from .encoder_layer import TransformerEncoderLayer  # noqa: F401
from .encoder import TransformerEncoder, ConformerEncoder, ReConformerEncoder  # noqa: F401
