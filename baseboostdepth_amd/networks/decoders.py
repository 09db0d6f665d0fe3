"""Decoder heads with the reference's interfaces and checkpoint layouts.

* `DepthDecoder` (reference networks/depth_decoder.py:11-59): U-Net disparity decoder; state dict
  `decoder.{0..13}.conv.conv.{weight,bias}` = ten ConvBlocks (upconv i,0 / i,1 for i = 4..0)
  followed by the four dispconvs.
* `PoseDecoder` (reference networks/pose_decoder.py:9-48): `net.{0..3}.{weight,bias}` = squeeze
  1x1, two 3x3, final 1x1; output scaled by 0.01 and split into axis-angle / translation.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..layers import ConvBlock, Conv3x3

_DECODER_WIDTHS = (16, 32, 64, 128, 256)


class DepthDecoder(nn.Module):
    def __init__(self, num_ch_enc, scales=range(4), num_output_channels=1, use_skips=True):
        super().__init__()
        self.num_output_channels, self.use_skips, self.scales = num_output_channels, use_skips, scales
        self.num_ch_enc = num_ch_enc
        self.num_ch_dec = np.array(_DECODER_WIDTHS)
        stages, self._slot = [], {}

        def add(key, module):
            self._slot[key] = len(stages)
            stages.append(module)

        for level in reversed(range(5)):
            width = int(self.num_ch_dec[level])
            fan_in = int(self.num_ch_enc[-1]) if level == 4 else int(self.num_ch_dec[level + 1])
            add(("upconv", level, 0), ConvBlock(fan_in, width))
            skip = int(self.num_ch_enc[level - 1]) if (use_skips and level > 0) else 0
            add(("upconv", level, 1), ConvBlock(width + skip, width))
        for s in self.scales:
            add(("dispconv", s), Conv3x3(int(self.num_ch_dec[s]), num_output_channels))
        self.decoder = nn.ModuleList(stages)

    def _stage(self, *key):
        return self.decoder[self._slot[key]]

    def _glued(self, level, x):
        """Can bias + ELU of both ConvBlocks of `level` move into the glue passes around them?  Both must start from a
        bias-free convolution (of `x`, resp. of the concatenation) and have a bias.  ops.FUSED_DECODER_GLUE selects
        between two fused forms: off (BBD_FUSED_DECODER_GLUE=0), every level takes `_plain`, as before the glue kernels."""
        first, second = self._stage("upconv", level, 0), self._stage("upconv", level, 1)
        return ops.FUSED_DECODER_GLUE and first._fused(x) and second.conv.conv.bias is not None

    def _plain(self, level, x, skip):
        """Each block with its own bias + ELU pass: first(x), then up-sample + concatenate + second."""
        return self._stage("upconv", level, 1).forward_upcat(self._stage("upconv", level, 0)(x), skip)

    def _level(self, level, x, xp, skip):
        """One decoder level: (x, xp) of the level above -> (x, xp) of this one.  `xp` is `x` with its reflection border
        where the level above wrote both in one pass (`ops.bias_elu_pad`), None wherever it did not: after a level that
        is not glued, in front of a level that is not, and below level 0."""
        if not self._glued(level, x):
            return self._plain(level, x, skip), None
        first, second = self._stage("upconv", level, 0), self._stage("upconv", level, 1)
        bias = first.conv.conv.bias
        z = first.conv_raw(xp if xp is not None else first.conv.pad(x))
        if not ops.upcat_pad_act_supported(z, bias, skip):
            # glue refused for this level (too many planes for one launch): what `_plain` does from `z` on
            return second.forward_upcat(first.bias_act_(z), skip), None
        # glued: conv -> upcat_pad_act -> conv -> bias_elu_pad, the blocks' bias + ELU ride on the glue passes
        if skip is None and ops.up2_conv3x3_routed(z, bias, second.conv.conv.weight):
            # up-sample + border + convolution as four 2x2 convolutions of z: no up-sampled copy
            z = ops.up2_conv3x3(z, bias, second.conv.conv.weight)
        else:
            z = second.conv_raw(ops.upcat_pad_act(z, bias, skip))
        if level > 0 and self._glued(level - 1, z) and ops.bias_elu_pad_supported(z, second.conv.conv.bias):
            return ops.bias_elu_pad(z, second.conv.conv.bias)
        return second.bias_act_(z), None            # level 0: nothing pads its output

    def forward(self, input_features):
        self.outputs = {}
        x, xp = input_features[-1], None
        for level in reversed(range(5)):
            skip = input_features[level - 1] if (self.use_skips and level > 0) else None
            x, xp = self._level(level, x, xp, skip)
            if level in self.scales:
                self.outputs[("disp", level)] = self._stage("dispconv", level).disparity(x)
        return self.outputs


class PoseDecoder(nn.Module):
    def __init__(self, num_ch_enc, num_input_features, num_frames_to_predict_for=None, stride=1):
        super().__init__()
        frames = num_input_features - 1 if num_frames_to_predict_for is None else num_frames_to_predict_for
        self.num_ch_enc, self.num_input_features, self.num_frames_to_predict_for = num_ch_enc, num_input_features, frames
        self.net = nn.ModuleList([
            nn.Conv2d(int(num_ch_enc[-1]), 256, 1),                      # squeeze
            nn.Conv2d(num_input_features * 256, 256, 3, stride, 1),
            nn.Conv2d(256, 256, 3, stride, 1),
            nn.Conv2d(256, 6 * frames, 1)])

    def forward(self, input_features):
        x = torch.cat([F.relu(self.net[0](feats[-1])) for feats in input_features], 1)
        x = F.relu(self.net[1](x))
        x = F.relu(self.net[2](x))
        pose = 0.01 * self.net[3](x).mean(3).mean(2).view(-1, self.num_frames_to_predict_for, 1, 6)
        return pose[..., :3], pose[..., 3:]
