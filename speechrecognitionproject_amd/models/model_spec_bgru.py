"""Drop-in for the reference plugin ``models/model_spec_bgru.py``: log spectrogram (321 x 49)
-> 2-layer BiGRU(321 -> 512) -> Linear(1024 -> 12) on the last time step
(model_spec_bgru.py:11-79).  Spectrogram = K3 (srk_spec_fwd), GRU/Linear = libsrk kernels."""
import torch
import torch.nn as nn

from .. import features
from ..nn import BiGRU, Linear
from ._common import DEVICE, accuracy, apply_specaug, check_specaug, class_accuracy   # noqa: F401


def compute_spec(sample):
    """FloatTensor[16000] -> FloatTensor[321, 49] (freq x time) on the CPU (model_spec_bgru.py:11-17)."""
    return features.spec(sample.reshape(1, -1))[0].cpu()


class Network(nn.Module):
    """``specaug=(W, NF, f_max, NT, t_max)`` (or a ``features.SpecAugPolicy``) turns on SpecAugment for training-mode
    forwards: a time warp, NF frequency masks and NT time masks on the [49, 321] spectrogram the GRU reads, drawn
    on the device (features.spec_augment); ``None`` (the default) and ``eval()`` leave the features untouched.  The
    parameters of the last augmented batch are in ``last_specaug`` (int32 [B, P])."""

    def __init__(self, num_features=512, num_layers=2, specaug=None):
        super().__init__()
        self.specaug = check_specaug(specaug, 49, 321)
        self.last_specaug = None
        self._specaug_bufs = {}
        self.gru = BiGRU(321, num_features, num_layers=num_layers, bidirectional=True, batch_first=True)
        self.fc = Linear(num_features * 2, 12)

    def forward(self, x, specaug_params=None):
        with torch.no_grad():
            inx = features.spec(x, transposed=True)     # [B, 49, 321] = transpose(spec, 1, 2)
            inx = apply_specaug(self, inx, specaug_params)
        return self.fc(self.gru.forward_last(inx))
