"""fbanks_cnn with a trainable front-end: log-mel filter banks (98 x 120, K2's dB output) -> per-channel energy
normalisation (nn.PCEN: each band divided by a smoothed version of its own recent energy, then root-compressed,
every constant learned per band) -> the fbanks_cnn convolutions and classifier.  No reference counterpart: the
reference's front-ends all end in a fixed logarithm, which turns the gain changes of its own augmentations into
offsets the CNN has to learn around.

``state_dict`` keys are model_fbanks_cnn's plus ``pcen.params`` [4, 120], so a trained fbanks_cnn checkpoint
warm-starts everything but the front-end: ``load_state_dict(sd, strict=False)``.  ``vtlp=(lo, hi)`` warps the
filter bank per training clip as in model_fbanks_cnn.  PCEN's output carries a gradient (towards ``pcen.params``),
so the fused conv1 + maxpool1 also runs its data gradient (srk_conv1_pool_dgrad).  ``specaug=...`` (as in
model_fbanks_cnn.Network) masks and warps the dB filter banks before PCEN, so the smoother sees the masked energy.
"""
import torch

from .. import features
from ..nn import PCEN, conv1_pool, conv_pool
from . import model_fbanks_cnn
from ._common import DEVICE, accuracy, apply_specaug, class_accuracy   # noqa: F401  (plugin API)
from .model_fbanks_cnn import filter_banks              # noqa: F401  (plugin API)


class Network(model_fbanks_cnn.Network):
    def __init__(self, vtlp=None, specaug=None):
        super().__init__(vtlp=vtlp, specaug=specaug)
        self.pcen = PCEN(120)

    def forward(self, x, alpha=None, specaug_params=None):
        with torch.no_grad():
            if alpha is None and self.training and self.vtlp is not None:
                alpha = self._draw_alpha(x.shape[0] if len(x.shape) > 1 else 1)
            inx = features.fbank(x, alpha=alpha)          # [B, 98, 120] dB, no gradient: PCEN writes no dx
            inx = apply_specaug(self, inx, specaug_params)
        h = self.pcen(inx)
        h = conv1_pool(h, self.conv1, self.maxpool1, next_conv_pool16=True)
        h = conv_pool(h, self.conv2, self.maxpool2)
        h = self.conv4(self.conv3(h))
        h = self.maxpool3(h.squeeze(2)).squeeze(1)
        h = self.dropout(h)
        return self.fc2(self.fc1(h))
