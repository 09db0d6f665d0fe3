"""ResNet encoder with the reference's interface (networks/resnet_encoder.py:56-91).

torchvision is not available on the target image, so the ResNet-18/34/50 trunk is defined
here with torchvision-identical module names - `conv1, bn1, layer{1..4}.{i}.conv{j}/bn{j},
layer{k}.0.downsample.{0,1}, fc` - so `encoder.pth` checkpoints written by the reference
(trainer.py:783-805) load with `load_state_dict` unchanged, including the unused `fc`.
"""
import numpy as np
import torch.nn as nn
import torch.nn.functional as F

from .. import ops


class FusedBatchNorm2d(nn.BatchNorm2d):
    """`nn.BatchNorm2d` (same parameters, buffers and state-dict keys) whose training-mode forward on
    the GPU also absorbs what follows it in a ResNet block: `relu(bn(x) + residual)` runs as two HIP
    launches each way (csrc/bbd_nn.hip) instead of MIOpen batch-norm + add + clamp kernels.  Host
    tensors, eval mode and exotic configurations take the stock PyTorch ops."""

    fused = ops.switch("BBD_FUSED_BN")

    def takes_fused_launches(self, x):
        """Does this module, in its current mode, normalise `x` with the fused launches (`ops.batch_norm_act`, the stem)?"""
        return (self.fused and self.training and self.affine and self.track_running_stats and self.momentum is not None
                and ops.batch_norm_act_supported(x))

    def forward(self, x, residual=None, relu=False):
        if self.takes_fused_launches(x):
            return ops.batch_norm_act(x, self.weight, self.bias, residual, self.running_mean, self.running_var,
                                      self.momentum, self.eps, relu, num_batches_tracked=self.num_batches_tracked)
        if self.training and x.is_cuda:
            if ops.call_groups(x.shape[0]).rows != (x.shape[0],):
                raise RuntimeError("a batched pass with call groups needs the fused BatchNorm path")
        y = super().forward(x)
        if residual is not None:
            y = y + residual
        return F.relu(y) if relu else y


class MaxPool3s2(nn.MaxPool2d):
    """The stem's `nn.MaxPool2d(3, 2, 1)`; fp32 GPU tensors take the HIP kernels (atomic-free backward)."""

    def __init__(self):
        super().__init__(kernel_size=3, stride=2, padding=1)

    def forward(self, x):
        if ops.maxpool3s2_supported(x):
            return ops.maxpool3s2(x)
        return super().forward(x)


def _plain_conv(conv, kernel, stride, padding):
    """Is `conv` a bias-free `nn.Conv2d` of that square kernel, stride and zero padding, dilation 1, groups 1?"""
    return (type(conv) is nn.Conv2d and conv.bias is None and conv.kernel_size == (kernel, kernel)
            and conv.stride == (stride, stride) and conv.padding == (padding, padding) and conv.dilation == (1, 1)
            and conv.groups == 1 and conv.padding_mode == "zeros")


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = FusedBatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = FusedBatchNorm2d(planes)
        self.downsample = downsample

    def _entry(self, x):
        """(conv1(x), the shortcut of x).  A down-sampling block whose shortcut convolution is routed in some direction
        sends it through `ops.conv1x1_s2`, or where `ops.block_entry_routed` says so both convolutions through `ops.block_entry`
        (one node: the shortcut's gradient is added into conv1's in place); `downsample.1` follows as before."""
        ds = self.downsample
        if ds is None:
            return self.conv1(x), x
        short = ds[0] if isinstance(ds, nn.Sequential) and len(ds) > 0 else None
        if (_plain_conv(short, 1, 2, 0)
                and any(ops.conv1x1s2_routed(x, short.weight, d) for d in ("fwd", "dgrad", "wgrad"))):
            if _plain_conv(self.conv1, 3, 2, 1) and ops.block_entry_routed(x, short.weight):
                out, identity = ops.block_entry(x, self.conv1.weight, short.weight)
            else:
                identity = ops.conv1x1_s2(x, short.weight)
                out = self.conv1(x)
            for module in list(ds)[1:]:
                identity = module(identity)
            return out, identity
        identity = ds(x)
        return self.conv1(x), identity

    def forward(self, x):
        out, identity = self._entry(x)
        out = self.bn1(out, relu=True)
        return self.bn2(self.conv2(out), residual=identity, relu=True)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = FusedBatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = FusedBatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = FusedBatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = self.bn1(self.conv1(x), relu=True)
        out = self.bn2(self.conv2(out), relu=True)
        return self.bn3(self.conv3(out), residual=identity, relu=True)


_CONFIGS = {18: (BasicBlock, [2, 2, 2, 2]), 34: (BasicBlock, [3, 4, 6, 3]), 50: (Bottleneck, [3, 4, 6, 3]),
            101: (Bottleneck, [3, 4, 23, 3]), 152: (Bottleneck, [3, 8, 36, 3])}


class ResNetTrunk(nn.Module):
    """ImageNet-style ResNet; `num_input_images` widens conv1 like ResNetMultiImageInput
    (networks/resnet_encoder.py:12-33)."""

    def __init__(self, num_layers, num_input_images=1, num_classes=1000):
        super().__init__()
        block, layers = _CONFIGS[num_layers]
        self.inplanes = 64
        self.conv1 = nn.Conv2d(num_input_images * 3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = FusedBatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = MaxPool3s2()
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512 * block.expansion, num_classes)   # never used; kept for checkpoint parity
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(
                nn.Conv2d(self.inplanes, planes * block.expansion, 1, stride, bias=False),
                FusedBatchNorm2d(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        layers += [block(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)


class ResnetEncoder(nn.Module):
    """`ResnetEncoder(num_layers, pretrained, num_input_images=1)`; forward -> 5 feature maps."""

    def __init__(self, num_layers, pretrained, num_input_images=1):
        super().__init__()
        if num_layers not in _CONFIGS:
            raise ValueError("{} is not a valid number of resnet layers".format(num_layers))
        if pretrained:
            raise RuntimeError("ImageNet weights cannot be downloaded here (no network); load a checkpoint "
                               "with load_state_dict instead (--weights_init scratch)")
        self.num_ch_enc = np.array([64, 64, 128, 256, 512])
        self.encoder = ResNetTrunk(num_layers, num_input_images)
        if num_layers > 34:
            self.num_ch_enc[1:] *= 4
        # False: nobody reads the stem's full-resolution feature (the pose network: only features[-1] reaches
        # PoseDecoder) - forward returns None in its place and the fused stem does not write it
        self.stem_feature = True

    def _stem(self, x):
        """conv1's output -> (f0 or None, pooled f0): one fused op where the library takes the activation
        (`ops.stem_bn_relu_pool`), else bn1 + ReLU and the max-pool as two."""
        e = self.encoder
        bn = e.bn1
        if (isinstance(bn, FusedBatchNorm2d) and isinstance(e.maxpool, MaxPool3s2) and bn.takes_fused_launches(x)
                and ops.stem_routed(x)):
            return ops.stem_bn_relu_pool(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps,
                                         want_y=self.stem_feature, num_batches_tracked=bn.num_batches_tracked)
        f0 = bn(x, relu=True)
        return (f0 if self.stem_feature else None), e.maxpool(f0)

    def _conv1(self, image, normalized):
        """conv1 of the normalised image: `ops.stem_conv` where a direction of it is routed (it normalises on the way in),
        else the normalisation and the module's own convolution."""
        conv = self.encoder.conv1
        if (type(conv) is nn.Conv2d and conv.bias is None and conv.stride == (2, 2) and conv.padding == (3, 3)
                and conv.dilation == (1, 1) and conv.groups == 1 and conv.padding_mode == "zeros"
                and any(ops.stem_conv_routed(image, conv.weight, d) for d in ("fwd", "wgrad"))):
            return ops.stem_conv(image, conv.weight, normalize=not normalized)
        return conv(image if normalized else (image - 0.45) / 0.225)

    def forward(self, input_image, normalized=False):
        """`normalized`: the caller hands in `(image - 0.45) / 0.225` already (the pooled step's pair gather does it in the
        same pass, `ops.gather_pairs`)."""
        e = self.encoder
        f0, pooled = self._stem(self._conv1(input_image, normalized))
        f1 = e.layer1(pooled)
        f2 = e.layer2(f1)
        f3 = e.layer3(f2)
        f4 = e.layer4(f3)
        self.features = [f0, f1, f2, f3, f4]
        return self.features
