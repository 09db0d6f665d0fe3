"""`layers` API of the reference (layers.py), MI355X-native.

Same names, constructor arguments and return shapes as the reference so that `trainer.py`- and
`evaluate_depth.py`-style callers are drop-in.  The geometry / photometric classes run as HIP
kernels through the C ABI (include/bbd_hip.h), including the pose-matrix composition
(`transformation_from_parameters`, one launch each way on GPU tensors).
"""
import torch
import torch.nn as nn

from . import ops


def disp_to_depth(disp, min_depth, max_depth):
    """Sigmoid output -> (scaled disparity, depth)  (layers.py:13-22)."""
    min_disp = 1 / max_depth
    max_disp = 1 / min_depth
    scaled_disp = min_disp + (max_disp - min_disp) * disp
    return scaled_disp, 1 / scaled_disp


def rot_from_axisangle(vec):
    """[n,1,3] axis-angle -> [n,4,4] rotation, Rodrigues entries of layers.py:61-100."""
    angle = torch.norm(vec, 2, 2, True)
    axis = vec / (angle + 1e-7)
    ca, sa = torch.cos(angle), torch.sin(angle)
    C = 1 - ca
    x, y, z = axis[..., 0:1], axis[..., 1:2], axis[..., 2:3]
    xs, ys, zs = x * sa, y * sa, z * sa
    xC, yC, zC = x * C, y * C, z * C
    xyC, yzC, zxC = x * yC, y * zC, z * xC
    zero, one = torch.zeros_like(ca), torch.ones_like(ca)
    rows = [x * xC + ca, xyC - zs, zxC + ys, zero,
            xyC + zs, y * yC + ca, yzC - xs, zero,
            zxC - ys, yzC + xs, z * zC + ca, zero,
            zero, zero, zero, one]
    return torch.cat(rows, dim=2).view(-1, 4, 4)


def get_translation_matrix(translation_vector):
    """[n,1,3] -> [n,4,4] homogeneous translation (layers.py:45-58)."""
    t = translation_vector.contiguous().view(-1, 3, 1)
    n = t.shape[0]
    eye = torch.eye(4, device=t.device, dtype=t.dtype).expand(n, 4, 4)
    top = torch.cat([eye[:, :3, :3], t], dim=2)
    return torch.cat([top, eye[:, 3:, :]], dim=1)


def transformation_from_parameters(axisangle, translation, invert=False):
    """(axisangle, translation) [n,1,3] -> [n,4,4]; inverted form is R^T @ T(-t)  (layers.py:25-42).

    GPU tensors go through the fused pose-matrix kernel (one launch forward, one backward, instead
    of ~35 element-wise launches each way); host tensors - fixtures, synthetic-pose helpers - use the
    op-for-op torch form below, which is what the golden vectors pin."""
    if axisangle.is_cuda:
        return ops.pose_matrix(axisangle, translation, invert)
    return _transformation_from_parameters_torch(axisangle, translation, invert)


def _transformation_from_parameters_torch(axisangle, translation, invert=False):
    R = rot_from_axisangle(axisangle)
    t = translation.clone()
    if invert:
        R = R.transpose(1, 2)
        t = t * -1
    T = get_translation_matrix(t)
    return torch.matmul(R, T) if invert else torch.matmul(T, R)


class ReflectionPad1(nn.ReflectionPad2d):
    """`nn.ReflectionPad2d(1)`; fp32 GPU tensors take the HIP kernels (gather-form backward)."""

    def __init__(self):
        super().__init__(1)

    def forward(self, x):
        if ops.reflect_pad1_supported(x):
            return ops.reflect_pad1(x)
        return super().forward(x)


class Conv3x3(nn.Module):
    """Reflection-padded 3x3 convolution (layers.py:118-133)."""

    def __init__(self, in_channels, out_channels, use_refl=True):
        super().__init__()
        self.pad = ReflectionPad1() if use_refl else nn.ZeroPad2d(1)
        self.conv = nn.Conv2d(int(in_channels), int(out_channels), 3)

    def _fused(self, x):
        """Is this a disparity head (one output channel behind a reflection border) on a tensor the HIP head takes?"""
        return (self.conv.out_channels == 1 and isinstance(self.pad, ReflectionPad1)
                and ops.disp_head_supported(x, self.conv.in_channels))

    def forward(self, x):
        if self._fused(x):
            return ops.dispconv(x, self.conv.weight, self.conv.bias)    # disparity head: one streaming kernel
        return self.conv(self.pad(x))

    def disparity(self, x):
        """sigmoid(self(x)); a disparity head does the convolution and its sigmoid in ONE HIP pass each way."""
        if self._fused(x):
            return ops.disp_head(x, self.conv.weight, self.conv.bias)
        return torch.sigmoid(self(x))


class ConvBlock(nn.Module):
    """Conv3x3 + ELU (layers.py:103-115).  fp32 GPU tensors: bias-free MIOpen convolution, then bias + ELU as
    one in-place HIP pass (and ELU' + bias gradient as one pass backward) instead of conv / add / ELU."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv = Conv3x3(in_channels, out_channels)
        self.nonlin = nn.ELU(inplace=True)

    def _fused(self, x, border=0):
        """Do bias + ELU run as `ops.bias_elu_` on the convolution of `x` (which carries `border` pixels of padding)?  A
        one-channel block leaves an `x` without its border to `Conv3x3`'s disparity head."""
        conv = self.conv.conv
        return conv.bias is not None and (border > 0 or conv.out_channels > 1) and ops.bias_elu_supported(x, border)

    def forward(self, x):
        if self._fused(x):
            return self.forward_padded(self.conv.pad(x))
        return self.nonlin(self.conv(x))

    def forward_padded(self, xp):
        """`xp` already carries the 1-pixel reflection border (e.g. from `ops.upcat_pad`)."""
        if self._fused(xp, 1):
            return self.bias_act_(self.conv_raw(xp))
        return self.nonlin(self.conv.conv(xp))

    def forward_upcat(self, x, skip=None):
        """self(cat(nearest_x2(x), skip)); up-sampling, concatenation and this block's reflection border are ONE HIP pass
        where `ops.upcat_pad` takes the tensors."""
        if ops.upcat_pad_supported(x, skip):
            return self.forward_padded(ops.upcat_pad(x, skip))
        x = upsample(x)
        return self(x if skip is None else torch.cat([x, skip], 1))

    def conv_raw(self, xp):
        """The bias-free convolution of the padded input: what `bias_act_` and the decoder's fused glue start from.
        The measured fine-scale shapes take their weight gradient from the NCHW tensors (`ops.conv3x3_valid`)."""
        weight = self.conv.conv.weight
        if ops.conv3x3_wgrad_routed(xp, weight):
            return ops.conv3x3_valid(xp, weight)
        return torch.nn.functional.conv2d(xp, weight, None)

    def bias_act_(self, y):
        """bias + ELU on `conv_raw`'s result (H * W a multiple of 4), in place where the HIP pass takes it."""
        conv = self.conv.conv
        if y.is_contiguous():        # channels-last inputs / NHWC policies can hand back a strided result
            return ops.bias_elu_(y, conv.bias)
        return self.nonlin(y + conv.bias.view(1, -1, 1, 1))


def upsample(x):
    return torch.nn.functional.interpolate(x, scale_factor=2, mode="nearest")


class BackprojectDepth(nn.Module):
    """depth [n,1,H,W], inv_K [n,4,4] -> camera points [n,4,H*W]  (layers.py:136-167); differentiable
    w.r.t. depth like the reference's module.

    The reference keeps [batch,3,H*W] pixel-grid and ones buffers; the kernel derives pixel
    coordinates from the thread index, so this module holds no tensors."""

    def __init__(self, batch_size, height, width):
        super().__init__()
        self.batch_size, self.height, self.width = batch_size, height, width

    def forward(self, depth, inv_K, backend=None):
        return ops.backproject(depth, inv_K, self.height, self.width, backend)


class GeometryConsistency(nn.Module):
    """SC-SfMLearner's geometry-consistency term (Bian et al., NeurIPS 2019) as one differentiable op:
    sigmoid disparity of the target frames [B,1,H,W], a list of V source disparities of that shape, a list of V
    target-to-source poses [B,4,4], K and inv_K [B,4,4] -> `ops.GeometryConsistency` (its `loss` is the mean of
    |z s - 1| / (z s + 1) over the visible samples).  Gradients reach every disparity and every pose."""

    def __init__(self, min_depth, max_depth):
        super().__init__()
        self.min_depth, self.max_depth = float(min_depth), float(max_depth)

    def forward(self, disp, source_disps, poses, K, inv_K, want_err=False, want_code=False, backend=None):
        source_disps, poses = list(source_disps), list(poses)
        if not source_disps or len(source_disps) != len(poses):
            raise ValueError("GeometryConsistency: one pose per source disparity is needed, got %d and %d"
                             % (len(source_disps), len(poses)))
        q_tgt = disp_to_depth(disp, self.min_depth, self.max_depth)[0][:, 0]
        q_src = torch.stack([disp_to_depth(d, self.min_depth, self.max_depth)[0][:, 0] for d in source_disps])
        T = torch.stack([p[:, :3] for p in poses])
        return ops.geometry_consistency(q_tgt, q_src, T, K, inv_K, want_err, want_code, backend)


class DepthHints(nn.Module):
    """Depth Hints (Watson et al., ICCV 2019) with the proxy depth computed inside the step: a semi-global
    matcher (`ops.stereo_hints`) on the frame and its stereo partner gives a hint depth per pixel; wherever the stereo
    partner warped with the HINT reprojects better than the step's own minimum photometric loss, the network's depth is
    pulled towards the hint with log(1 + |depth - hint|).

    `forward(left, right, K, inv_K, stereo_T, disps, to_optimise)`: `left`, `right` float32 [B,3,H,W]; `disps` the
    sigmoid disparities of the scales (any resolution, up-sampled bilinearly as the reprojection does); `to_optimise`
    one [B,H,W] map per scale.  Returns (term, share): the mean over scales of mean(mask * log(1 + |depth_s - hint|)) over
    ALL pixels, and the mean of the masks.  Hint, its loss `l_h` (computed once) and the masks are made under no_grad:
    gradients reach `disps` only.  The matcher's scratch is allocated on the first call and kept."""

    def __init__(self, min_depth, max_depth, disparities=128, no_ssim=False):
        super().__init__()
        self.min_depth, self.max_depth = float(min_depth), float(max_depth)
        self.disparities, self.no_ssim = int(disparities), bool(no_ssim)
        self._scratch = None

    def scratch(self, B, H, W, device):
        need = ops.sgm_scratch_bytes(B, H, W, self.disparities, 8)
        if self._scratch is None or self._scratch.numel() < need or self._scratch.device != device:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=device)
        return self._scratch

    @torch.no_grad()
    def hints(self, left, right, K, inv_K, stereo_T, backend=None):
        """(hint depth [B,H,W], valid [B,H,W], l_h [B,H,W]: the photometric loss of `right` warped with the hint)."""
        B, _, H, W = left.shape
        side = (stereo_T[:, 0, 3] > 0).to(torch.int32)
        disp16, _ = ops.stereo_hints(left, right, side, self.disparities, scratch=self.scratch(B, H, W, left.device),
                                     backend=backend)
        hint, valid = ops.hint_depth(disp16, K, stereo_T)
        depth = torch.where(valid, hint, torch.ones_like(hint)).unsqueeze(1)
        points = ops.backproject(depth, inv_K, H, W, backend)
        grid = ops.project3d(points, K, stereo_T, H, W, backend=backend)
        warped = torch.nn.functional.grid_sample(right, grid, padding_mode="border", align_corners=True)
        l_h = torch.abs(left - warped).mean(1)
        if not self.no_ssim:
            l_h = 0.85 * ops.ssim_map(warped, left, backend).mean(1) + 0.15 * l_h
        return hint, valid, l_h

    def forward(self, left, right, K, inv_K, stereo_T, disps, to_optimise, backend=None):
        disps, to_optimise = list(disps), list(to_optimise)
        if not disps or len(disps) != len(to_optimise):
            raise ValueError("DepthHints: one minimum-loss map per disparity scale is needed, got %d and %d"
                             % (len(disps), len(to_optimise)))
        if right.shape != left.shape:
            raise ValueError("DepthHints needs the stereo partner of every sample of the batch, got %s for %s"
                             % (tuple(right.shape), tuple(left.shape)))
        H, W = left.shape[2:]
        hint, valid, l_h = self.hints(left, right, K, inv_K, stereo_T, backend)
        term, share = 0.0, 0.0
        for disp, best in zip(disps, to_optimise):
            if tuple(disp.shape[2:]) != (H, W):
                disp = torch.nn.functional.interpolate(disp, [H, W], mode="bilinear", align_corners=False)
            depth = disp_to_depth(disp, self.min_depth, self.max_depth)[1][:, 0]
            mask = valid & (l_h < best.detach())
            term = term + torch.where(mask, torch.log1p(torch.abs(depth - hint)), torch.zeros_like(depth)).mean()
            share = share + mask.to(torch.float32).mean()
        return term / len(disps), share / len(disps)


class Project3D(nn.Module):
    """points [n,4,H*W], K, T [n,4,4] -> sampling grid [n,H,W,2] in [-1,1]  (layers.py:170-195);
    differentiable w.r.t. points, T and K."""

    def __init__(self, batch_size, height, width, eps=1e-7):
        super().__init__()
        self.batch_size, self.height, self.width, self.eps = batch_size, height, width, eps

    def forward(self, points, K, T, backend=None):
        return ops.project3d(points, K, T, self.height, self.width, self.eps, backend)


class SSIM(nn.Module):
    """(1 - SSIM)/2 map between image pairs, [n,3,H,W] -> [n,3,H,W]  (layers.py:219-249); differentiable
    w.r.t. both images."""

    def forward(self, x, y, backend=None):
        return ops.ssim_map(x, y, backend)


def get_smooth_loss(disp, img):
    """Edge-aware first-order smoothness (layers.py:203-216)."""
    gdx = torch.abs(disp[:, :, :, :-1] - disp[:, :, :, 1:])
    gdy = torch.abs(disp[:, :, :-1, :] - disp[:, :, 1:, :])
    gix = torch.mean(torch.abs(img[:, :, :, :-1] - img[:, :, :, 1:]), 1, keepdim=True)
    giy = torch.mean(torch.abs(img[:, :, :-1, :] - img[:, :, 1:, :]), 1, keepdim=True)
    return (gdx * torch.exp(-gix)).mean() + (gdy * torch.exp(-giy)).mean()


def compute_depth_errors(gt, pred):
    """KITTI depth metrics abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3 (layers.py:271-286)."""
    thresh = torch.max(gt / pred, pred / gt)
    a1 = (thresh < 1.25).float().mean()
    a2 = (thresh < 1.25 ** 2).float().mean()
    a3 = (thresh < 1.25 ** 3).float().mean()
    rmse = torch.sqrt(((gt - pred) ** 2).mean())
    rmse_log = torch.sqrt(((torch.log(gt) - torch.log(pred)) ** 2).mean())
    abs_rel = torch.mean(torch.abs(gt - pred) / gt)
    sq_rel = torch.mean((gt - pred) ** 2 / gt)
    return abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3
