"""Drop-in for Modules/JDC/model.py: JDCNet, the frozen pitch extractor of the fine-tune step.

train.py builds `JDCNet(num_class=1, seq_len=192)`, loads the pretrained F0 model into it, and calls it in eval
mode under no_grad on the cropped mel (train.py:260-261): F0_real, _, _ = pitch_extractor(gt.unsqueeze(1)).
This module holds the reference's 77 state-dict entries (so `load_state_dict(strict=True)` takes the checkpoint's
`pitch_extractor` block) and runs forward on the HIP plan (engine.PitchEngine -> stts_pitch_fwd).  It is
inference-only, as the reference uses it: train mode (batch statistics, dropout) raises.  The detector branch
(`detector_conv`, `bilstm_detector`, `detector`) is never run by the reference's forward; its parameters are kept
for the state dict only.
"""
from __future__ import annotations

import torch
from torch import nn


class ResBlock(nn.Module):
    """reference Modules/JDC/model.py:158-190 (parameter layout)."""

    def __init__(self, in_channels: int, out_channels: int, leaky_relu_slope=0.01):
        super().__init__()
        self.downsample = in_channels != out_channels
        self.pre_conv = nn.Sequential(
            nn.BatchNorm2d(num_features=in_channels),
            nn.LeakyReLU(leaky_relu_slope, inplace=True),
            nn.MaxPool2d(kernel_size=(1, 2)),
        )
        self.conv = nn.Sequential(
            nn.Conv2d(in_channels, out_channels, 3, padding=1, bias=False),
            nn.BatchNorm2d(out_channels),
            nn.LeakyReLU(leaky_relu_slope, inplace=True),
            nn.Conv2d(out_channels, out_channels, 3, padding=1, bias=False),
        )
        self.conv1by1 = None
        if self.downsample:
            self.conv1by1 = nn.Conv2d(in_channels, out_channels, 1, bias=False)


class JDCNet(nn.Module):
    """reference Modules/JDC/model.py:10-137."""

    def __init__(self, num_class=722, seq_len=31, leaky_relu_slope=0.01):
        super().__init__()
        self.num_class = num_class
        self.seq_len = seq_len  # (unused by the reference's forward too)
        self.leaky_relu_slope = leaky_relu_slope
        self.conv_block = nn.Sequential(
            nn.Conv2d(1, 64, 3, padding=1, bias=False),
            nn.BatchNorm2d(64),
            nn.LeakyReLU(leaky_relu_slope, inplace=True),
            nn.Conv2d(64, 64, 3, padding=1, bias=False),
        )
        self.res_block1 = ResBlock(64, 128)
        self.res_block2 = ResBlock(128, 192)
        self.res_block3 = ResBlock(192, 256)
        self.pool_block = nn.Sequential(
            nn.BatchNorm2d(256),
            nn.LeakyReLU(leaky_relu_slope, inplace=True),
            nn.MaxPool2d(kernel_size=(1, 4)),
            nn.Dropout(p=0.2),
        )
        self.detector_conv = nn.Sequential(
            nn.Conv2d(640, 256, 1, bias=False),
            nn.BatchNorm2d(256),
            nn.LeakyReLU(leaky_relu_slope, inplace=True),
            nn.Dropout(p=0.2),
        )
        self.bilstm_classifier = nn.LSTM(input_size=512, hidden_size=256, batch_first=True, bidirectional=True)
        self.bilstm_detector = nn.LSTM(input_size=512, hidden_size=256, batch_first=True, bidirectional=True)
        self.classifier = nn.Linear(512, num_class)
        self.detector = nn.Linear(512, 2)
        self._engine = None

    def invalidate(self):
        """Drop the packed weights (after writes through `param.data`, which stale() cannot see)."""
        self._engine = None

    def engine(self, dtype="fp32"):
        from .engine import PitchEngine
        if self._engine is None or self._engine.dtype != dtype or self._engine.stale(self):
            self._engine = PitchEngine(self, dtype=dtype)
        return self._engine

    def forward(self, x, dtype="fp32"):
        """mel [B, 1, 80, T] -> (F0 = |classifier| squeezed, GAN_feature [B, 256, 10, T], poolblock_out
        [B, 256, T, 2]), as reference :102-137 in eval mode."""
        if self.training:
            raise NotImplementedError("JDCNet: the HIP path is the eval-mode forward train.py uses (running BatchNorm "
                                      "statistics, no dropout); call .eval() first")
        if self.leaky_relu_slope != 0.01:
            raise NotImplementedError("JDCNet: the HIP plan is built for leaky_relu_slope = 0.01 (the reference's)")
        with torch.no_grad():
            f0, gan, pool = self.engine(dtype).forward(x)
        return torch.abs(f0.squeeze()), gan, pool
