"""Small-footprint keyword spotting: a depthwise-separable CNN (DS-CNN, Zhang et al. 2017, "Hello Edge") on the
log-mel filter banks of model_fbanks_cnn.  No reference counterpart: the reference's CNN is dense.

    fbank [B, 98, 120]
     -> conv1 (7x3, pad (3,1)) + maxpool (1,3), fused                          [B, 98, 40, 64]
     -> bn1, ReLU
     -> ds1: dw 3x3 stride (1,2), bn, ReLU -> pw 1x1 64 -> 128, bn, ReLU       [B, 98, 20, 128]
     -> ds2: dw 3x3 stride (1,1)           -> pw 128 -> 128                    [B, 98, 20, 128]
     -> ds3: dw 3x3 stride (2,2)           -> pw 128 -> 256                    [B, 49, 10, 256]
     -> ds4: dw 3x3 stride (1,1)           -> pw 256 -> 256                    [B, 49, 10, 256]
     -> global average pool -> fc (256 -> 12)

Every convolution after conv1 is bias-free (a BatchNorm follows each).  ``state_dict`` keys: ``conv1.*``, ``bn1.*``,
``ds{1..4}.{dw,bn_dw,pw,bn_pw}.*``, ``fc.*``; ``conv1.*`` has model_fbanks_cnn's names and shapes, so a trained
fbanks_cnn checkpoint warm-starts the first layer: ``load_state_dict(sd, strict=False)``.  ``vtlp=(lo, hi)`` warps
the filter bank per training clip exactly as in model_fbanks_cnn.

Kernels: K2 (features), the fused one-channel conv1 + max-pool, srk_dwconv2d_nhwc_* (depthwise, fp32 at every
precision), K6 (the 1x1 convolutions: matrix cores, 16-bit operands under ``--precision bf16|fp16``), K9 (BatchNorm +
ReLU), srk_avgpool_nhwc_*, K7 (fc).  In the 16-bit modes the BatchNorm in front of a depthwise conv still writes the
16-bit copy of its output that a dense conv would take; the depthwise conv reads the fp32 tensor.
"""
import torch
import torch.nn as nn

from .. import features
from ..nn import BatchNorm1d, Conv2d, DepthwiseConv2d, GlobalAvgPool2d, Linear, MaxPool2d, _copy16_drop, conv1_pool
from . import model_fbanks_cnn
from ._common import DEVICE, accuracy, apply_specaug, check_specaug, class_accuracy   # noqa: F401  (plugin API)
from .model_fbanks_cnn import filter_banks              # noqa: F401  (plugin API)


class DSBlock(nn.Module):
    """Depthwise 3x3 (stride given) + BatchNorm + ReLU, then pointwise 1x1 + BatchNorm + ReLU."""

    def __init__(self, cin, cout, stride):
        super().__init__()
        self.dw = DepthwiseConv2d(cin, 3, stride=stride, padding=1, bias=False)
        self.bn_dw = BatchNorm1d(cin)
        self.pw = Conv2d(cin, cout, 1, bias=False)
        self.bn_pw = BatchNorm1d(cout)

    def forward(self, x):
        x = self.bn_dw(self.dw(x), relu=True)
        return self.bn_pw(self.pw(x), relu=True)


class Network(nn.Module):
    """``vtlp`` as in model_fbanks_cnn.Network (whose draw it shares): ``None`` never warps, ``(lo, hi)`` warps
    training-mode forwards; the factors of the last drawn batch are in ``last_alpha``.  ``specaug`` likewise as in
    model_fbanks_cnn.Network: SpecAugment on the (warped) filter banks, its parameters in ``last_specaug``."""

    _draw_alpha = model_fbanks_cnn.Network._draw_alpha

    def __init__(self, vtlp=None, specaug=None):
        super().__init__()
        self.vtlp = model_fbanks_cnn.check_vtlp(vtlp)
        self.last_alpha = None
        self._alpha_bufs = {}
        self.specaug = check_specaug(specaug, 98, 120)
        self.last_specaug = None
        self._specaug_bufs = {}
        self.conv1 = Conv2d(1, 64, kernel_size=(7, 3), padding=(3, 1))
        self.maxpool1 = MaxPool2d((1, 3))
        self.bn1 = BatchNorm1d(64)
        self.ds1 = DSBlock(64, 128, (1, 2))
        self.ds2 = DSBlock(128, 128, (1, 1))
        self.ds3 = DSBlock(128, 256, (2, 2))
        self.ds4 = DSBlock(256, 256, (1, 1))
        self.pool = GlobalAvgPool2d()
        self.fc = Linear(256, 12)

    def forward(self, x, alpha=None, specaug_params=None):
        with torch.no_grad():
            if alpha is None and self.training and self.vtlp is not None:
                alpha = self._draw_alpha(x.shape[0] if len(x.shape) > 1 else 1)
            inx = features.fbank(x, alpha=alpha)              # [B, 98, 120]
            inx = apply_specaug(self, inx, specaug_params)
        h = conv1_pool(inx, self.conv1, self.maxpool1)        # fused conv1 + maxpool1: NHWC [B, 98, 40, 64]
        # 16-bit training steps: the fused kernel hands its output's 16-bit copy over for a dense conv2, which this
        # model does not have.  bn1 reads the fp32 tensor, so nobody would take the entry, and it would keep h — and
        # through h this step's autograd graph — alive into the next step (and into a graph capture)
        _copy16_drop(h)
        h = self.bn1(h, relu=True)
        h = self.ds4(self.ds3(self.ds2(self.ds1(h))))         # [B, 49, 10, 256]
        return self.fc(self.pool(h))
