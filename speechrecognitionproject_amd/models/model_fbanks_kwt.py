"""Keyword Transformer (KWT, Berg et al., Interspeech 2021): a post-norm transformer encoder over the frames of the
log-mel filter banks of model_fbanks_cnn.  No reference counterpart: the reference has no transformer.

    fbank [B, 98, 120]
     -> embed: Linear(120 -> dim) per frame, + pos [98, dim]                  tokens [B, 98, dim]
     -> layers x TransformerEncoderLayer(dim, heads, mlp_dim)                 (nn.TransformerEncoderLayer)
     -> mean over the 98 tokens -> fc: Linear(dim -> 12)

The defaults are KWT-1's sizes (dim 64, 1 head, MLP 256, 12 layers; KWT-2: 128 / 2 / 512, KWT-3: 192 / 3 / 768).  The
paper reads the prediction off a learned class token; here the tokens are averaged (GlobalAvgPool2d on the
[B, 98, 1, dim] view), which needs no concatenation in front of the encoder and reuses an existing kernel.

``state_dict`` keys: ``pos``, ``embed.*``, ``layers.{i}.<torch.nn.TransformerEncoderLayer's keys>``, ``fc.*``; ``pos`` is
drawn from N(0, 0.02^2).  ``pos`` is two-dimensional, so the optimizer's default weight-decay filter decays it along
with the weight matrices.  ``vtlp=(lo, hi)`` warps the filter bank per training clip exactly as in model_fbanks_cnn.

Kernels: K2 (features), K7 (every Linear: matrix cores, 16-bit operands under ``--precision bf16|fp16``; the
positional add is the embedding GEMM's beta = 1 epilogue, the gradient of ``pos`` srk_colsum_f32 over the batch),
srk_mhsa_*, srk_layernorm_* (both residual adds fused) and srk_gelu_* (fp32 at every precision), srk_avgpool_nhwc_*.
"""
import torch
import torch.nn as nn

from .. import features
from ..nn import GlobalAvgPool2d, Linear, TransformerEncoderLayer, _EmbedPosFn
from . import model_fbanks_cnn
from ._common import DEVICE, accuracy, class_accuracy   # noqa: F401  (plugin API)
from .model_fbanks_cnn import filter_banks              # noqa: F401  (plugin API)

FRAMES, BANDS = 98, 120


class Network(nn.Module):
    """``vtlp`` as in model_fbanks_cnn.Network (whose draw it shares): ``None`` never warps, ``(lo, hi)`` warps
    training-mode forwards; the factors of the last drawn batch are in ``last_alpha``."""

    _draw_alpha = model_fbanks_cnn.Network._draw_alpha

    def __init__(self, dim=64, heads=1, mlp_dim=256, layers=12, vtlp=None):
        super().__init__()
        if dim <= 0 or heads <= 0 or dim % heads:
            raise ValueError("dim %r must be a positive multiple of heads %r" % (dim, heads))
        if (dim // heads) % 4 or not 4 <= dim // heads <= 64:
            raise ValueError("head size dim / heads = %d is outside the attention kernel's domain (a multiple of 4 in "
                             "4..64)" % (dim // heads))
        if not 1 <= dim <= 1024 or mlp_dim < 1 or layers < 1:
            raise ValueError("needs 1 <= dim <= 1024 (LayerNorm), mlp_dim >= 1 and layers >= 1")
        self.vtlp = model_fbanks_cnn.check_vtlp(vtlp)
        self.last_alpha = None
        self._alpha_bufs = {}
        self.pos = nn.Parameter(torch.empty(FRAMES, dim).normal_(std=0.02))
        self.embed = Linear(BANDS, dim)
        self.layers = nn.ModuleList([TransformerEncoderLayer(dim, heads, mlp_dim) for _ in range(layers)])
        self.pool = GlobalAvgPool2d()
        self.fc = Linear(dim, 12)

    def forward(self, x, alpha=None):
        with torch.no_grad():
            if alpha is None and self.training and self.vtlp is not None:
                alpha = self._draw_alpha(x.shape[0] if len(x.shape) > 1 else 1)
            inx = features.fbank(x, alpha=alpha)              # [B, 98, 120]
        B = inx.shape[0]
        h = _EmbedPosFn.apply(inx.reshape(B * FRAMES, BANDS), self.embed.weight, self.embed.bias, self.pos)
        h = h.view(B, FRAMES, -1)
        for layer in self.layers:
            h = layer(h)
        return self.fc(self.pool(h.unsqueeze(2)))             # the mean over the tokens: [B, dim]
