"""Drop-in for the reference plugin ``models/model_resnet_dconv.py``: raw-waveform ResNet-18-style
1-D front end (Conv1d k=80/s=4 stem -> L 4000, 4 stages x 2 BasicBlocks with k=3 convs, 64 / 128 / 256 /
256 channels, BatchNorm, ReLU) -> Linear(256, 256) per step -> a dilated-convolution head: three biased
k=5 convs (256 -> 384 -> 512 -> 640; padding / dilation 2/1, 8/4, 32/16) over the 500 steps, MaxPool1d(10),
Conv1d(640, 640, k=50) over the remaining 50 steps, Linear(640, 640), Linear(640, 12); no ReLU in the head
(model_resnet_dconv.py:10-127).

Same constructor ``Network()``, ``state_dict`` keys / shapes (``resnet.*``, ``dilation.conv1..4``,
``dilation.fc1``, ``dilation.fc2``, so reference checkpoints load) and helpers.  Activations stay
channels-last [B, L, C].  Convolutions = K6 (the dilated ones through srk_conv1d_nlc_dil_*, conv4 as the
full-width plain GEMM), BatchNorm(+residual+ReLU) = K9.

One quirk is kept exactly: after fc1 the reference REINTERPRETS the [B * 500, 256] result with
``x.view(bs, -1, sl)`` as [B, 256 channels, 500 steps] (model_resnet_dconv.py:91) — not a transpose: channel c
at step t of the head's input is element (c * 500 + t) of the clip's [500, 256] block.  In channels-last
terms that is ``y.view(bs, 256, 500).transpose(1, 2).contiguous()``, one torch copy.

BatchNorm under data parallelism uses per-rank batch statistics.
"""
import torch
import torch.nn as nn

from ..nn import BatchNorm1d, Conv1d, Linear, MaxPool1d
from ._common import DEVICE, accuracy, class_accuracy   # noqa: F401


class BasicBlock(nn.Module):
    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = Conv1d(inplanes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn1 = BatchNorm1d(planes)
        self.conv2 = Conv1d(planes, planes, 3, stride=1, padding=1, bias=False)
        self.bn2 = BatchNorm1d(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        residual = x
        if self.downsample is not None:
            residual = self.downsample[1](self.downsample[0](x))
        out = self.bn1(self.conv1(x), relu=True)
        return self.bn2(self.conv2(out), residual=residual, relu=True)


class ResNet(nn.Module):
    def __init__(self, block):
        super().__init__()
        self.inplanes = 64
        self.conv1 = Conv1d(1, 64, kernel_size=80, stride=4, padding=38, bias=False)
        self.bn1 = BatchNorm1d(64)
        self.relu = nn.ReLU(inplace=True)
        self.layer1 = self._make_layer(block, 64, 2)
        self.layer2 = self._make_layer(block, 128, 2, stride=2)
        self.layer3 = self._make_layer(block, 256, 2, stride=2)
        self.layer4 = self._make_layer(block, 256, 2, stride=2)
        self.fc1 = Linear(256, 256)
        for m in self.modules():
            if isinstance(m, Conv1d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes:
            downsample = nn.Sequential(Conv1d(self.inplanes, planes, kernel_size=1, stride=stride, bias=False),
                                       BatchNorm1d(planes))
        layers = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes))
        return nn.Sequential(*layers)

    def forward(self, x):
        # x: [B, L, 1] channels-last waveform
        x = self.bn1(self.conv1(x), relu=True)                      # [B, 4000, 64]
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))   # [B, 500, 256]
        bs, sl, _ = x.shape
        x = self.fc1(x.reshape(bs * sl, -1))                        # [B * 500, 256]
        # :91, x.view(bs, -1, sl): the clip's [sl, 256] block read as [256 channels, sl steps]
        return x.view(bs, -1, sl).transpose(1, 2).contiguous()      # channels-last [B, sl, 256]


class Dilation(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = Conv1d(256, 384, kernel_size=5, padding=2, dilation=1)
        self.conv2 = Conv1d(384, 512, kernel_size=5, padding=8, dilation=4)
        self.conv3 = Conv1d(512, 640, kernel_size=5, padding=32, dilation=16)
        self.maxpool = MaxPool1d(10)
        self.conv4 = Conv1d(640, 640, kernel_size=50)
        self.fc1 = Linear(640, 640)
        self.fc2 = Linear(640, 12)

    def forward(self, x):
        x = self.conv3(self.conv2(self.conv1(x)))   # [B, 500, 640]
        x = self.conv4(self.maxpool(x))             # [B, 50, 640] -> [B, 1, 640]
        return self.fc2(self.fc1(x.reshape(x.shape[0], -1)))


class Network(nn.Module):
    def __init__(self):
        super().__init__()
        self.resnet = ResNet(BasicBlock)
        self.dilation = Dilation()

    def forward(self, x):
        if not torch.is_tensor(x):
            x = torch.as_tensor(x)
        x = x.to(DEVICE, torch.float32).reshape(x.shape[0], -1, 1)   # [B, 16000, 1]
        return self.dilation(self.resnet(x))
