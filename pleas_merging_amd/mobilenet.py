"""MobileNetV2 definition with torchvision-compatible state-dict keys.

torchvision is not a dependency (see resnet.py), so the MobileNet family needs its own definition as well.  Attribute names
and the order of the modules follow the public torchvision layout (``features.k.conv.{0.0, 0.1, 1.0, 1.1, 2, 3}``,
``classifier.1``), so that real torchvision checkpoints load with ``load_state_dict``; the activations are
``nn.ReLU6(inplace=True)`` modules, which carry no keys.  The forward is fx-traceable and spells the head the way the spec rules
and the inference graph recognise it: ``AdaptiveAvgPool2d((1, 1)) -> torch.flatten(x, 1) -> Dropout -> Linear``.
The residual add of an inverted-residual block has no activation behind it (linear bottleneck).
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch
from torch import nn


def _make_divisible(v: float, divisor: int, min_value: Optional[int] = None) -> int:
    """``v`` rounded to the nearest multiple of ``divisor``, at least ``min_value`` and never more than 10 % below ``v``."""
    if min_value is None:
        min_value = divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


def _conv_bn_relu6(cin: int, cout: int, k: int = 3, stride: int = 1, groups: int = 1) -> nn.Sequential:
    """conv (no bias) -> BatchNorm2d -> ReLU6 at indices 0, 1, 2."""
    return nn.Sequential(nn.Conv2d(cin, cout, k, stride, (k - 1) // 2, groups=groups, bias=False), nn.BatchNorm2d(cout),
                         nn.ReLU6(inplace=True))


class InvertedResidual(nn.Module):
    def __init__(self, inp: int, oup: int, stride: int, expand_ratio: int):
        super().__init__()
        if stride not in (1, 2):
            raise ValueError("stride should be 1 or 2 instead of %s" % stride)
        hidden = int(round(inp * expand_ratio))
        self.use_res_connect = stride == 1 and inp == oup
        layers: List[nn.Module] = []
        if expand_ratio != 1:
            layers.append(_conv_bn_relu6(inp, hidden, k=1))                     # pointwise expansion
        layers += [_conv_bn_relu6(hidden, hidden, stride=stride, groups=hidden),  # depthwise
                   nn.Conv2d(hidden, oup, 1, 1, 0, bias=False),                    # pointwise projection, linear
                   nn.BatchNorm2d(oup)]
        self.conv = nn.Sequential(*layers)

    def forward(self, x):
        if self.use_res_connect:
            return x + self.conv(x)
        return self.conv(x)


DEFAULT_SETTING = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))


class MobileNetV2(nn.Module):
    def __init__(self, num_classes: int = 1000, width_mult: float = 1.0,
                 inverted_residual_setting: Optional[Sequence[Sequence[int]]] = None, round_nearest: int = 8, dropout: float = 0.2):
        super().__init__()
        setting = DEFAULT_SETTING if inverted_residual_setting is None else inverted_residual_setting
        if len(setting) == 0 or any(len(row) != 4 for row in setting):
            raise ValueError("inverted_residual_setting should be non-empty rows of 4 (t, c, n, s), got %s" % (setting,))
        cin = _make_divisible(32 * width_mult, round_nearest)
        self.last_channel = _make_divisible(1280 * max(1.0, width_mult), round_nearest)
        features: List[nn.Module] = [_conv_bn_relu6(3, cin, stride=2)]
        for t, c, n, s in setting:
            cout = _make_divisible(c * width_mult, round_nearest)
            for i in range(n):
                features.append(InvertedResidual(cin, cout, s if i == 0 else 1, t))
                cin = cout
        features.append(_conv_bn_relu6(cin, self.last_channel, k=1))
        self.features = nn.Sequential(*features)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.classifier = nn.Sequential(nn.Dropout(p=dropout), nn.Linear(self.last_channel, num_classes))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out")
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0, 0.01)
                nn.init.zeros_(m.bias)

    def forward(self, x):
        x = self.features(x)
        x = torch.flatten(self.avgpool(x), 1)
        return self.classifier(x)


def mobilenet_v2(num_classes: int = 1000, width_mult: float = 1.0,
                 inverted_residual_setting: Optional[Sequence[Sequence[int]]] = None, round_nearest: int = 8,
                 dropout: float = 0.2) -> MobileNetV2:
    return MobileNetV2(num_classes, width_mult, inverted_residual_setting, round_nearest, dropout)


MODELS = {"mobilenet_v2": mobilenet_v2}
