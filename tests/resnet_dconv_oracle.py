"""CPU restatement of the reference's ``models/model_resnet_dconv.py`` — TEST INFRASTRUCTURE ONLY.

A plain-torch module with the reference's arithmetic and ``state_dict`` layout, as ``oracle/models.py``
restates the other plugins: raw waveform -> Conv1d(1, 64, k 80, s 4, p 38) + BatchNorm + ReLU (L 4000) ->
four stages of two residual blocks of k = 3 convolutions (64, 128, 256, 256 channels; stages 2-4 halve
the length to 500) -> Linear(256, 256) per step -> the dilation head: three biased k = 5 convolutions
(256 -> 384 -> 512 -> 640, padding / dilation 2/1, 8/4, 32/16), MaxPool1d(10), Conv1d(640, 640, k 50),
Linear(640, 640), Linear(640, 12).  The head has no nonlinearity besides the max-pool.

One quirk is part of the arithmetic: the per-step Linear's [B * 500, 256] result is handed to the head by
``view(B, -1, 500)``, i.e. the clip's [500 steps, 256] block is READ as [256 channels, 500 steps] without a
transpose.  ``tests/golden/resnet_dconv_golden.npz`` (written from the reference itself) pins it.
"""
import torch
import torch.nn as nn

NUM_CLASSES = 12


class _Block(nn.Module):
    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv1d(inplanes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm1d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv1d(planes, planes, 3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm1d(planes)
        self.downsample = downsample

    def forward(self, x):
        res = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return self.relu(out + res)


class _ResNet1d(nn.Module):
    def __init__(self):
        super().__init__()
        self.inplanes = 64
        self.conv1 = nn.Conv1d(1, 64, kernel_size=80, stride=4, padding=38, bias=False)
        self.bn1 = nn.BatchNorm1d(64)
        self.relu = nn.ReLU(inplace=True)
        self.layer1 = self._layer(64, 2)
        self.layer2 = self._layer(128, 2, 2)
        self.layer3 = self._layer(256, 2, 2)
        self.layer4 = self._layer(256, 2, 2)
        self.fc1 = nn.Linear(256, 256)

    def _layer(self, planes, blocks, stride=1):
        ds = None
        if stride != 1 or self.inplanes != planes:
            ds = nn.Sequential(nn.Conv1d(self.inplanes, planes, 1, stride=stride, bias=False), nn.BatchNorm1d(planes))
        layers = [_Block(self.inplanes, planes, stride, ds)]
        self.inplanes = planes
        layers += [_Block(planes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def forward(self, x):
        x = self.relu(self.bn1(self.conv1(x)))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))   # [B, 256, 500]
        b, _, t = x.shape
        x = self.fc1(x.transpose(1, 2).reshape(b * t, -1))          # [B * 500, 256]
        return x.view(b, -1, t)   # the quirk: [500, 256] read as [256 channels, 500 steps]


class _DilationHead(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv1d(256, 384, kernel_size=5, padding=2, dilation=1)
        self.conv2 = nn.Conv1d(384, 512, kernel_size=5, padding=8, dilation=4)
        self.conv3 = nn.Conv1d(512, 640, kernel_size=5, padding=32, dilation=16)
        self.maxpool = nn.MaxPool1d(10)
        self.conv4 = nn.Conv1d(640, 640, kernel_size=50)
        self.fc1 = nn.Linear(640, 640)
        self.fc2 = nn.Linear(640, NUM_CLASSES)

    def forward(self, x):
        x = self.maxpool(self.conv3(self.conv2(self.conv1(x))))
        return self.fc2(self.fc1(self.conv4(x).squeeze(2)))


class ResnetDconv(nn.Module):
    def __init__(self):
        super().__init__()
        self.resnet = _ResNet1d()
        self.dilation = _DilationHead()

    def forward(self, x):
        return self.dilation(self.resnet(x.to(self.dilation.fc2.weight.dtype).unsqueeze(1)))


def white_noise_clips(batch, seed):
    """The fixture's clips: rint(N(0, 3000)) white noise, [batch, 16000] float32, and labels (5 i + 3) % 12."""
    import numpy as np
    rng = np.random.default_rng(seed)
    x = np.rint(rng.normal(0.0, 3000.0, (batch, 16000))).astype(np.float32)
    return x, ((np.arange(batch) * 5 + 3) % NUM_CLASSES).astype(np.int64)


def sampled_grad_errors(got, idx, ref64):
    """(max-norm relative, 2-norm relative) error of the sampled entries got[idx] against the float64 values."""
    import numpy as np
    g = np.asarray(got, np.float64).reshape(-1)[idx]
    r = np.asarray(ref64, np.float64)
    return (float(np.abs(g - r).max() / max(np.abs(r).max(), 1e-300)),
            float(np.linalg.norm(g - r) / max(np.linalg.norm(r), 1e-300)))
