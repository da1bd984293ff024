"""mfcc_bgru with attention pooling in place of the last-step select: MFCC(+deltas) -> 2-layer
BiGRU(39 -> 512) -> a query from the last step scores all 51 steps -> softmax over time -> the weighted
sum of the steps -> Linear(1024 -> 12).  The "attention RNN" form of a recurrent keyword spotter; no
reference counterpart (the reference's recurrent plugins all keep one step and drop the other 50).

``state_dict`` keys are model_mfcc_bgru's plus ``query.weight`` / ``query.bias``, so a trained mfcc_bgru
checkpoint warm-starts everything but the query: ``load_state_dict(sd, strict=False)``.
``Network.attention(x)`` returns the per-step weights [B, 51]: where in the second the model listened.
"""
import torch
import torch.nn as nn

from .. import features
from ..nn import AttentionPool, BiGRU, Linear, last_step
from ._common import DEVICE, accuracy, apply_specaug, check_specaug, class_accuracy   # noqa: F401  (plugin API)


class Network(nn.Module):
    """``specaug`` as in model_mfcc_bgru.Network: SpecAugment on the [51, 39] MFCC map of training-mode forwards,
    its parameters in ``last_specaug``; ``None`` (the default) and ``eval()`` leave the features untouched."""

    def __init__(self, num_features=512, num_layers=2, specaug=None):
        super().__init__()
        self.specaug = check_specaug(specaug, 51, 39)
        self.last_specaug = None
        self._specaug_bufs = {}
        self.gru = BiGRU(39, num_features, num_layers=num_layers, bidirectional=True, batch_first=True)
        self.query = Linear(num_features * 2, num_features * 2)
        self.fc = Linear(num_features * 2, 12)
        self.pool = AttentionPool()   # scale 1 / sqrt(2 H); no parameters

    def _pooled(self, x, specaug_params=None):
        with torch.no_grad():
            inx = features.mfcc(x, time_major=True)     # [B, 51, 39]
            inx = apply_specaug(self, inx, specaug_params)
        y, _ = self.gru(inx)
        return self.pool(y, self.query(last_step(y)))

    def forward(self, x, specaug_params=None):
        return self.fc(self._pooled(x, specaug_params)[0])

    def attention(self, x):
        """The attention weights alpha [B, 51] of a batch of clips (rows sum to 1)."""
        with torch.no_grad():
            return self._pooled(x)[1]
