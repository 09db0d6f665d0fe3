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

    def _glue_level(self, level, x):
        """Do both ConvBlocks of `level` start from a bias-free convolution of input `x`, so that bias + ELU can move
        into the glue passes (BBD_FUSED_DECODER_GLUE=0: never)?"""
        return (ops.FUSED_DECODER_GLUE and self._stage("upconv", level, 0)._fused(x)
                and self._stage("upconv", level, 1).conv.conv.bias is not None)

    def forward(self, input_features):
        self.outputs = {}
        x = input_features[-1]
        xp = None       # x with its reflection border, where the level above wrote both in one pass (ops.bias_elu_pad)
        for level in reversed(range(5)):
            first, second = self._stage("upconv", level, 0), self._stage("upconv", level, 1)
            skip = input_features[level - 1] if (self.use_skips and level > 0) else None
            glued = False
            if self._glue_level(level, x):
                # the blocks' bias + ELU ride on the glue passes: conv -> upcat_pad_act -> conv -> bias_elu_pad
                z = first.conv_raw(xp if xp is not None else first.conv.pad(x))
                glued = ops.upcat_pad_act_supported(z, first.conv.conv.bias, skip)
                if not glued:
                    x = first.bias_act_(z)              # what first(x) does
            else:
                x = first(x)
            xp = None
            if glued:
                if skip is None and ops.up2_conv3x3_routed(z, first.conv.conv.bias, second.conv.conv.weight):
                    # up-sample + border + convolution as four 2x2 convolutions of z: no up-sampled copy
                    z = ops.up2_conv3x3(z, first.conv.conv.bias, second.conv.conv.weight)
                else:
                    z = second.conv_raw(ops.upcat_pad_act(z, first.conv.conv.bias, skip))
                if level > 0 and self._glue_level(level - 1, z) and ops.bias_elu_pad_supported(z, second.conv.conv.bias):
                    x, xp = ops.bias_elu_pad(z, second.conv.conv.bias)
                else:
                    x = second.bias_act_(z)             # level 0: nothing pads its output
            elif ops.upcat_pad_supported(x, skip):
                # nearest x2 + skip concatenation + the next block's reflection border in ONE HIP pass
                x = self._stage("upconv", level, 1).forward_padded(ops.upcat_pad(x, skip))
            else:
                x = F.interpolate(x, scale_factor=2, mode="nearest")
                if skip is not None:
                    x = torch.cat([x, skip], 1)
                x = self._stage("upconv", level, 1)(x)
            if level in self.scales:
                head = self._stage("dispconv", level)
                if head._fused(x):
                    # convolution to one channel and its sigmoid in ONE HIP pass each way
                    self.outputs[("disp", level)] = ops.disp_head(x, head.conv.weight, head.conv.bias)
                else:
                    self.outputs[("disp", level)] = torch.sigmoid(head(x))
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
