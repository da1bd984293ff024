"""CPU statement of the depthwise convolution, the global average pool and the fbanks_dscnn plugin — TEST
INFRASTRUCTURE ONLY.

``dwconv`` / ``dwconv_backward`` are numpy direct sums over the taps on channels-last arrays, in the dtype of their
inputs (float64 in the tests):

    y[n, ho, wo, c] = b[c] + sum_{kh, kw} w[c, 0, kh, kw] x[n, ho sh - ph + kh, wo sw - pw + kw, c]
    dx[n, hi, wi, c] = sum over the (kh, kw, ho, wo) with ho sh - ph + kh = hi, wo sw - pw + kw = wi of w dy
    dw[c, 0, kh, kw] = sum_{n, ho, wo} dy x,   db[c] = sum dy

(tests/test_dscnn.py holds them to float64 autograd of ``F.conv2d(groups=C)``), ``dw_case`` the seeded inputs with
those results, ``FbanksDscnn`` the model in torch CPU modules (NCHW, ``F.conv2d(groups=C)``) with the plugin's
``state_dict`` keys and shapes; it runs in float64 after ``.double()``.
"""
import functools

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import features as OF
from oracle import models as OM

# name -> (N, H, W, C, KH, KW, ph, pw, sh, sw): the smallest shapes that reach each code path of csrc/dwconv.hip
CASES = {
    "vec4_ragged": (2, 5, 7, 4, 3, 3, 1, 1, 1, 1),         # one float4 channel group, ragged everything
    "scalar_c6": (2, 7, 8, 6, 3, 3, 1, 1, 1, 1),           # C % 4 != 0: the scalar path
    "scalar_c1": (2, 5, 6, 1, 3, 3, 1, 1, 1, 1),
    "stride2_odd": (3, 9, 11, 12, 3, 3, 1, 1, 2, 2),       # stride 2 both ways, odd H / W (Ho 5, Wo 6): dgrad parity
    "stride2_h": (3, 8, 10, 12, 3, 3, 1, 1, 2, 1),         # stride 2 on H only, even H
    "tiny_input": (2, 2, 2, 8, 3, 3, 1, 1, 2, 2),          # input smaller than the kernel: taps mostly padding
    "no_pad_1x1": (1, 3, 3, 8, 3, 3, 0, 0, 1, 1),          # no padding, Ho = Wo = 1
    "k5x3": (2, 4, 9, 8, 5, 3, 2, 1, 1, 1),                # non-square
    "k7x7": (2, 9, 9, 8, 7, 7, 3, 3, 1, 1),                # the largest kernel: six tap groups in the weight gradient
    "scalar_stride2": (2, 6, 7, 3, 3, 3, 1, 1, 2, 2),      # the scalar path of the stride-2 register tiles
    "stride2_pad0": (2, 7, 9, 8, 3, 3, 0, 0, 2, 2),        # 3 x 3, stride 2 along W, pw != 1: the looped data gradient
    "pad2": (1, 4, 5, 4, 3, 3, 2, 2, 1, 1),                # padding K - 1: outputs that see padding only
    "ds1": (2, 98, 40, 64, 3, 3, 1, 1, 1, 2),              # the plugin's four layers
    "ds2": (2, 98, 20, 128, 3, 3, 1, 1, 1, 1),
    "ds3": (2, 98, 20, 128, 3, 3, 1, 1, 2, 2),
    "ds4": (2, 49, 10, 256, 3, 3, 1, 1, 1, 1),
    "ds1_n16": (16, 98, 40, 64, 3, 3, 1, 1, 1, 2),         # many workgroups: the slab reduction of dw / db
}


def out_size(size, k, p, s):
    return (size + 2 * p - k) // s + 1


def _tap_ranges(size, osize, k, p, s):
    """Output positions [lo, hi) whose input position o s - p + k lies in [0, size), and the first input position."""
    lo = max(0, -((k - p) // s))           # smallest o with o s - p + k >= 0
    hi = min(osize, (size - 1 + p - k) // s + 1)
    return lo, hi, lo * s - p + k


def dwconv(x, w, b, padding, stride):
    """x [N, H, W, C], w [C, 1, KH, KW], b [C] or None -> y [N, Ho, Wo, C]."""
    N, H, W, C = x.shape
    KH, KW = w.shape[2:]
    (ph, pw), (sh, sw) = padding, stride
    Ho, Wo = out_size(H, KH, ph, sh), out_size(W, KW, pw, sw)
    y = np.zeros((N, Ho, Wo, C), x.dtype)
    if b is not None:
        y += b
    for kh in range(KH):
        h0, h1, hi = _tap_ranges(H, Ho, kh, ph, sh)
        for kw in range(KW):
            w0, w1, wi = _tap_ranges(W, Wo, kw, pw, sw)
            if h1 <= h0 or w1 <= w0:
                continue
            y[:, h0:h1, w0:w1] += w[:, 0, kh, kw] * x[:, hi:hi + (h1 - h0) * sh:sh, wi:wi + (w1 - w0) * sw:sw]
    return y


def dwconv_backward(x, w, dy, padding, stride):
    """(dx, dw, db) of sum(y dy), closed form."""
    N, H, W, C = x.shape
    KH, KW = w.shape[2:]
    (ph, pw), (sh, sw) = padding, stride
    Ho, Wo = dy.shape[1:3]
    dx = np.zeros_like(x)
    dw = np.zeros_like(w)
    for kh in range(KH):
        h0, h1, hi = _tap_ranges(H, Ho, kh, ph, sh)
        for kw in range(KW):
            w0, w1, wi = _tap_ranges(W, Wo, kw, pw, sw)
            if h1 <= h0 or w1 <= w0:
                continue
            d = dy[:, h0:h1, w0:w1]
            sl = (slice(None), slice(hi, hi + (h1 - h0) * sh, sh), slice(wi, wi + (w1 - w0) * sw, sw))
            dx[sl] += w[:, 0, kh, kw] * d
            dw[:, 0, kh, kw] = (d * x[sl]).sum(axis=(0, 1, 2))
    return dx, dw, dy.sum(axis=(0, 1, 2))


@functools.lru_cache(maxsize=None)
def dw_case(name):
    """The seeded float64 inputs of a case (rounded to float32 first: the kernels see exactly these values) with the
    forward (with bias ``y``, without ``y_nobias``) and the backward; computed once, shared, never written to."""
    N, H, W, C, KH, KW, ph, pw, sh, sw = CASES[name]
    rng = np.random.default_rng(sum(v * 31 ** i for i, v in enumerate(CASES[name])) % (1 << 32))
    Ho, Wo = out_size(H, KH, ph, sh), out_size(W, KW, pw, sw)
    x = rng.standard_normal((N, H, W, C))
    w = rng.standard_normal((C, 1, KH, KW)) / np.sqrt(KH * KW)
    b = rng.standard_normal(C)
    dy = rng.standard_normal((N, Ho, Wo, C))
    x, w, b, dy = (a.astype(np.float32).astype(np.float64) for a in (x, w, b, dy))
    y = dwconv(x, w, b, (ph, pw), (sh, sw))
    dx, dw, db = dwconv_backward(x, w, dy, (ph, pw), (sh, sw))
    out = {"x": x, "w": w, "b": b, "dy": dy, "y": y, "y_nobias": y - b, "dx": dx, "dw": dw, "db": db,
           "padding": (ph, pw), "stride": (sh, sw)}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


class _DSBlock(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.dw = nn.Conv2d(cin, cin, 3, stride=stride, padding=1, groups=cin, bias=False)
        self.bn_dw = nn.BatchNorm2d(cin)
        self.pw = nn.Conv2d(cin, cout, 1, bias=False)
        self.bn_pw = nn.BatchNorm2d(cout)

    def forward(self, x):
        x = F.conv2d(x, self.dw.weight, None, self.dw.stride, self.dw.padding, 1, self.dw.in_channels)
        x = F.relu(self.bn_dw(x))
        return F.relu(self.bn_pw(self.pw(x)))


class FbanksDscnn(nn.Module):
    """models/model_fbanks_dscnn.py in torch CPU modules, NCHW."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(1, 64, kernel_size=(7, 3), padding=(3, 1))
        self.maxpool1 = nn.MaxPool2d((1, 3))
        self.bn1 = nn.BatchNorm2d(64)
        self.ds1 = _DSBlock(64, 128, (1, 2))
        self.ds2 = _DSBlock(128, 128, (1, 1))
        self.ds3 = _DSBlock(128, 256, (2, 2))
        self.ds4 = _DSBlock(256, 256, (1, 1))
        self.fc = nn.Linear(256, OM.NUM_CLASSES)

    @staticmethod
    def features(x):
        return torch.from_numpy(np.stack([OF.filter_banks(c) for c in x.numpy()]))

    def forward_features(self, inx):
        h = self.maxpool1(self.conv1(inx.to(self.conv1.weight.dtype).unsqueeze(1)))   # [B, 64, 98, 40]
        h = F.relu(self.bn1(h))
        h = self.ds4(self.ds3(self.ds2(self.ds1(h))))                                  # [B, 256, 49, 10]
        return self.fc(h.mean(dim=(2, 3)))

    def forward(self, x):
        with torch.no_grad():
            inx = self.features(x)
        return self.forward_features(inx)
