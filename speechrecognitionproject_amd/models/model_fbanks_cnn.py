"""Drop-in for the reference plugin ``models/model_fbanks_cnn.py``: log-mel filter banks (98 x 120)
-> conv1 (7x3) -> maxpool (1,3) -> conv2 (1x7) -> maxpool (1,4) -> conv3 (1x10) -> conv4 (7x1)
-> max over time -> dropout -> fc1 -> fc2, no nonlinearities (model_fbanks_cnn.py:68-147).

Same constructor, ``state_dict`` keys/shapes and helpers.  The per-clip CPU ``filter_banks`` loop
(:84-87) becomes one batched HIP launch (K2); conv1 + maxpool1 run as one fused one-channel kernel
(srk_conv1_pool_*: the pre-pool activation is never written), conv2-4 as channels-last implicit GEMMs
on the matrix cores (K6), conv2's maxpool in its GEMM epilogue (srk_conv2d_nhwc_fwd_pool).
"""
import torch
import torch.nn as nn

from .. import features
from ..nn import Conv2d, Dropout, Linear, MaxPool1d, MaxPool2d, conv1_pool, conv_pool
from ._common import DEVICE, accuracy, apply_specaug, check_specaug, class_accuracy   # noqa: F401


def filter_banks(sample):
    """FloatTensor[16000] -> FloatTensor[98, 120] (time x mel) on the CPU (model_fbanks_cnn.py:15-66)."""
    return features.fbank(sample.reshape(1, -1))[0].cpu()


def check_vtlp(vtlp):
    """The constructor argument ``vtlp`` of the filter-bank plugins as ``(lo, hi)`` floats, or None."""
    if vtlp is None:
        return None
    lo, hi = (float(v) for v in vtlp)
    if not 0.8 <= lo <= hi <= 1.25:
        raise ValueError("vtlp=(lo, hi) must satisfy 0.8 <= lo <= hi <= 1.25, got %r" % (vtlp,))
    return (lo, hi)


class Network(nn.Module):
    """``vtlp=(lo, hi)`` turns on the reference's VTLP augmentation (legacy/model_8/dataset_top.py:245-267:
    the mel filter bank warped by one uniform(lo, hi) factor per clip) for training-mode forwards;
    ``None`` (the default, and the reference's constructor call) never warps.  ``eval()`` never warps
    either (dataset_top.py warps under ``self.train`` only).  The factors of the last drawn batch are in
    ``last_alpha`` (float64 [B], one persistent buffer per batch size: a captured step reads a static
    address).

    ``specaug=(W, NF, f_max, NT, t_max)`` (or a ``features.SpecAugPolicy``) turns on SpecAugment for training-mode
    forwards: a time warp, NF frequency masks and NT time masks on the feature map the network reads, drawn on
    the device (features.spec_augment); ``None`` (the default) and ``eval()`` leave the features untouched.  The
    parameters of the last augmented batch are in ``last_specaug`` (int32 [B, P]).  With VTLP on as well, the
    bank is warped first and the warped features are masked."""

    def __init__(self, vtlp=None, specaug=None):
        super().__init__()
        self.vtlp = check_vtlp(vtlp)
        self.last_alpha = None
        self._alpha_bufs = {}
        self.specaug = check_specaug(specaug, 98, 120)
        self.last_specaug = None
        self._specaug_bufs = {}
        self.conv1 = Conv2d(1, 64, kernel_size=(7, 3), padding=(3, 1))
        self.maxpool1 = MaxPool2d((1, 3))
        self.conv2 = Conv2d(64, 128, (1, 7), padding=(0, 3))
        self.maxpool2 = MaxPool2d((1, 4))
        self.conv3 = Conv2d(128, 256, (1, 10))
        self.conv4 = Conv2d(256, 512, (7, 1), padding=(3, 0))
        self.maxpool3 = MaxPool1d(98)
        self.dropout = Dropout()
        self.fc1 = Linear(512, 256)
        self.fc2 = Linear(256, 12)

    def _draw_alpha(self, n):
        # one buffer per (device, batch size), kept for the module's life: a captured step of the full
        # batch keeps its address while a short last batch runs eagerly on another
        key = (torch.cuda.current_device(), n)
        buf = self._alpha_bufs.get(key)
        if buf is None:
            buf = self._alpha_bufs[key] = torch.empty(n, device="cuda", dtype=torch.float64)
        self.last_alpha = features.vtlp_draw(n, self.vtlp[0], self.vtlp[1], out=buf)
        return buf

    def forward(self, x, alpha=None, specaug_params=None):
        with torch.no_grad():
            if alpha is None and self.training and self.vtlp is not None:
                alpha = self._draw_alpha(x.shape[0] if len(x.shape) > 1 else 1)
            inx = features.fbank(x, alpha=alpha)          # [B, 98, 120]
            inx = apply_specaug(self, inx, specaug_params)
        # fused conv1 + maxpool1: NHWC [B, 98, 40, 64] (its fp32 copy skipped when conv2 reads the 16-bit one)
        h = conv1_pool(inx, self.conv1, self.maxpool1, next_conv_pool16=True)
        h = conv_pool(h, self.conv2, self.maxpool2)      # fused conv2 + maxpool2: [B, 98, 10, 128]
        h = self.conv4(self.conv3(h))                     # [B, 98, 1, 512]
        h = self.maxpool3(h.squeeze(2)).squeeze(1)        # [B, 512]
        h = self.dropout(h)
        return self.fc2(self.fc1(h))
