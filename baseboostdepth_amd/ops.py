"""torch.autograd wrappers around the C-ABI kernels (include/bbd_hip.h).

PyTorch is plumbing here (device memory, streams, autograd tape); all arithmetic of the hot
path runs in baseboostdepth_amd/csrc/bbd_kernels.hip.  `HipBackend` is the only backend the
product has: it refuses non-GPU tensors and raises if the extension is missing.  (The CPU test
tier injects a host build of the same arithmetic through the `backend=` seam - see
tests/ports.py - but nothing in this package can fall back to it.  A backend provides `name`, `lib`, `_check`, `run`,
`num_tiles*`, `smooth_chunks` and `fused_work_items`.)
"""
import collections
import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import COMPOSE_STRIDE, COMPOSE_ERROR, COMPOSE_REPLACE, POSE_STRIDE, PROJ_STRIDE, MAX_FRAME_SLOTS, ptr
from .plan import frame_slot
from .tables import join64, split64, upload


def switch(name):
    """A `BBD_FUSED_*` switch of the A/B runs: on unless the environment sets it to 0.  Every switch is a module global
    (one class attribute: `FusedBatchNorm2d.fused`) initialised here, once, and read where a path is chosen; the list is
    in INTEGRATION.md."""
    return os.environ.get(name, "1") != "0"


def hip_fp32(*tensors):
    """Is every argument that is not None a float32 tensor on the GPU - the only kind the network ops below take?"""
    return all(t is None or (t.is_cuda and t.dtype == torch.float32) for t in tensors)


# The y extent of a launch grid.  The pad, pool and glue entry points put one plane (sample x channel) there, the stem one
# channel, the disparity head one sample, and refuse more with BBD_E_BADARG (csrc/bbd_nn.hip, the `> 65535` tests of the
# bbd_* functions at its end; include/bbd_hip.h where it documents the limit).  The `*_supported` predicates use this name.
MAX_PLANES = 65535


def _experiment(name, default):
    """Experiment knobs of the A/B tooling (tools/*.sh) are read only under BBD_EXPERIMENT=1: a stray variable in a
    user's environment cannot put the shipped library into a configuration no test covers."""
    if os.environ.get("BBD_EXPERIMENT") != "1":
        return default
    return os.environ.get(name, default)


FUSED_NN = switch("BBD_FUSED_NN")     # 0: the encoder / decoder glue (pad, pool, bias + ELU, heads) back to the stock ATen kernels
FUSED_TOKEN_GLUE = switch("BBD_FUSED_TOKEN_GLUE")   # MonoViT: residual + DropPath + LayerNorm passes


class KernelTimer:
    """HIP-event timing of individual C-ABI launches, on the stream they are launched on.

    Used by bench.py to measure the fused kernels' own duration inside the full training step
    (torch.cuda.Event records on torch's current stream, which is the stream `HipBackend` launches
    on).  Off by default: `backend.timer = KernelTimer()` turns it on."""

    def __init__(self):
        self.events = {}

    def launch(self, name, fn):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        # (the grouped identity launch is reported under the plain entry point's name: same work, same byte model)
        self.events.setdefault(name.replace("_grouped_", "_"), []).append((e0, e1))

    def reset(self):
        self.events = {}

    def summary(self):
        """{kernel: (launches, mean ms)} - call after a device synchronise."""
        out = {}
        for name, evs in self.events.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            out[name] = (len(ms), sum(ms) / max(len(ms), 1))
        return out


class HipBackend:
    """Launches on the current torch HIP stream of the tensors' device."""

    name = "hip"

    def __init__(self):
        self.lib = _lib.get_lib()
        self.timer = None
        self._shared_work = {}

    def num_tiles(self, H, W):
        return self.lib.num_tiles(H, W)

    def num_tiles_fwd(self, H, W):
        return self.lib.num_tiles_fwd(H, W)

    def num_tiles_bwd(self, H, W):
        return self.lib.num_tiles_bwd(H, W)

    def smooth_chunks(self):
        return self.lib.smooth_chunks

    def fused_work_items(self, plan, S, H, W, backward, device):
        """Device table [S*B*ntiles, 2] of bbd_fused_work_items (slab order per XCD, the plan's samples with the most
        candidates first).  Batch order - every batch whose samples arrive sorted by candidate count, `Trainer`'s
        canonical order - is ONE table per launch shape, uploaded once and shared by all plans; any other order is part
        of the step's table upload (`steptables.StepTables`) or, for callers without one, a single asynchronous upload."""
        if _experiment("BBD_WORK_TABLE", "1") == "0":      # A/B switch: grid order, decoded in the kernel
            return None
        if plan.sample_order is None:
            tb = self._shared_work
            key = (str(device), plan.B, S, H, W, int(backward))
        else:
            tb = plan.tables(device)
            key = ("work", S, H, W, int(backward))
        if key not in tb:
            from . import steptables
            n = S * plan.B * (self.num_tiles_bwd(H, W) if backward else self.num_tiles_fwd(H, W))
            host = torch.empty(n, 2, dtype=torch.int32, pin_memory=torch.device(device).type == "cuda")
            order = None if plan.sample_order is None else (ctypes.c_int32 * plan.B)(*plan.sample_order)
            try:
                self.lib.call("bbd_fused_work_items", plan.B, S, H, W, int(backward), order, host.data_ptr())
                tb[key] = host.to(device, non_blocking=True)
                steptables.STATS["single_uploads"] += 1
            except _lib.BbdError:
                # outside the table's packing limits (more than 4 096 samples, 8 scales or 2^17 tiles): the launches take
                # the grid order and decode it themselves - a speed choice only
                tb[key] = None
        return tb[key]

    @staticmethod
    def _check(*tensors):
        for t in tensors:
            if t is not None and not t.is_cuda:
                raise _lib.BbdError("the HIP hot path needs GPU tensors (got %s); there is no CPU path"
                                    % t.device)

    def run(self, name, anchor, *args):
        if self.timer is not None:
            self.timer.launch(name, lambda: self.lib.call(name, *args, self.lib.stream_for(anchor)))
        else:
            self.lib.call(name, *args, self.lib.stream_for(anchor))


_BACKEND = None


def _frame_list(frame_tensors):
    return [frame_tensors] if torch.is_tensor(frame_tensors) else list(frame_tensors.values())


def default_backend():
    global _BACKEND
    if _BACKEND is None:
        _BACKEND = HipBackend()
    return _BACKEND


def frame_pointer_array(frame_tensors):
    """Host array[MAX_FRAME_SLOTS] of base addresses; `frame_tensors` maps frame id -> [n,3,H,W] - or IS one pool tensor
    [F,3,H,W] holding every frame of the step (`pooled.PooledStep`): all slots then point at it and the tables address
    it by row."""
    arr = (ctypes.c_void_p * MAX_FRAME_SLOTS)()
    if torch.is_tensor(frame_tensors):
        assert frame_tensors.is_contiguous() and frame_tensors.dtype == torch.float32
        for i in range(MAX_FRAME_SLOTS):
            arr[i] = frame_tensors.data_ptr()
        return arr
    for f, t in frame_tensors.items():
        assert t.is_contiguous() and t.dtype == torch.float32
        arr[frame_slot(f)] = t.data_ptr()
    return arr


# ---------------------------------------------------------------------------- disp -> depth
class _DispToDepth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disp, H, W, min_depth, max_depth, backend):
        B, one, h, w = disp.shape
        assert one == 1
        disp = disp.contiguous()
        depth = torch.empty(B, 1, H, W, device=disp.device, dtype=torch.float32)
        backend._check(disp)
        backend.run("bbd_disp_to_depth_fwd", disp, ptr(disp), ptr(depth), B, h, w, H, W,
                    float(min_depth), float(max_depth))
        ctx.save_for_backward(disp, depth)
        ctx.meta = (H, W, float(min_depth), float(max_depth), backend)
        return depth

    @staticmethod
    def backward(ctx, grad_depth):
        disp, depth = ctx.saved_tensors
        H, W, lo, hi, backend = ctx.meta
        B, _, h, w = disp.shape
        grad_depth = grad_depth.contiguous()
        grad_disp = torch.empty_like(disp)
        backend.run("bbd_disp_to_depth_bwd", disp, ptr(disp), ptr(depth), ptr(grad_depth), ptr(grad_disp), B, h, w,
                    H, W, lo, hi)
        return grad_disp, None, None, None, None, None


def disp_to_depth_fullres(disp, H, W, min_depth, max_depth, backend=None):
    """F.interpolate(bilinear, align_corners=False) + layers.disp_to_depth (trainer.py:455-461)."""
    return _DispToDepth.apply(disp, H, W, min_depth, max_depth, backend or default_backend())


class _DispPyramidToDepth(torch.autograd.Function):
    """All scales at once: S low-res disparity maps -> one [S,B,H,W] depth buffer (no cat copy)."""

    @staticmethod
    def forward(ctx, H, W, min_depth, max_depth, backend, *disps):
        disps = [d.contiguous() for d in disps]
        B = disps[0].shape[0]
        depth = torch.empty(len(disps), B, H, W, device=disps[0].device, dtype=torch.float32)
        backend._check(*disps)
        for i, d in enumerate(disps):
            backend.run("bbd_disp_to_depth_fwd", d, ptr(d), ptr(depth[i]), B, d.shape[2], d.shape[3], H, W,
                        float(min_depth), float(max_depth))
        ctx.save_for_backward(depth, *disps)
        ctx.meta = (H, W, float(min_depth), float(max_depth), backend)
        return depth

    @staticmethod
    def backward(ctx, grad_depth):
        depth, disps = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        H, W, lo, hi, backend = ctx.meta
        grad_depth = grad_depth.contiguous()
        grads = []
        for i, d in enumerate(disps):
            g = torch.empty_like(d)
            backend.run("bbd_disp_to_depth_bwd", d, ptr(d), ptr(depth[i]), ptr(grad_depth[i]), ptr(g), d.shape[0],
                        d.shape[2], d.shape[3], H, W, lo, hi)
            grads.append(g)
        return (None, None, None, None, None) + tuple(grads)


def disp_pyramid_to_depth(disps, H, W, min_depth, max_depth, backend=None):
    """[("disp", s)] list -> depth [S,B,H,W]; depth[i] is the reference's outputs[("depth",0,s_i)]."""
    return _DispPyramidToDepth.apply(H, W, min_depth, max_depth, backend or default_backend(), *disps)


# ---------------------------------------------------------------------------- pose matrix
class _PoseMatrix(torch.autograd.Function):
    @staticmethod
    def forward(ctx, axisangle, translation, invert, backend, invert_rows):
        aa = axisangle.reshape(-1, 3).contiguous()
        tr = translation.reshape(-1, 3).contiguous()
        backend._check(aa, tr)
        n = aa.shape[0]
        assert invert_rows is None or (invert_rows.dtype == torch.int32 and invert_rows.numel() == n)
        M = torch.empty(n, 4, 4, device=aa.device, dtype=torch.float32)
        backend.run("bbd_pose_matrix_fwd", aa, ptr(aa), ptr(tr), ptr(M), n, int(invert), ptr(invert_rows))
        ctx.save_for_backward(aa, tr)
        ctx.meta = (bool(invert), backend, axisangle.shape, translation.shape, invert_rows)
        return M

    @staticmethod
    def backward(ctx, gM):
        aa, tr = ctx.saved_tensors
        invert, backend, shp_a, shp_t, invert_rows = ctx.meta
        gM = gM.contiguous()
        ga, gt = torch.empty_like(aa), torch.empty_like(tr)
        backend.run("bbd_pose_matrix_bwd", aa, ptr(aa), ptr(tr), ptr(gM), ptr(ga), ptr(gt), aa.shape[0], int(invert),
                    ptr(invert_rows))
        return ga.view(shp_a), gt.view(shp_t), None, None, None


def pose_matrix(axisangle, translation, invert=False, backend=None, invert_rows=None):
    """layers.transformation_from_parameters as one kernel (forward) + one (backward).  `invert_rows` (device int32 [n])
    replaces the scalar flag row by row: the poses of both signs of a step in one launch each way."""
    return _PoseMatrix.apply(axisangle, translation, invert, backend or default_backend(), invert_rows)


# ---------------------------------------------------------------------------- smoothness
class _SmoothLoss(torch.autograd.Function):
    """get_smooth_loss(disp / (mean(disp)+1e-7), img) as two launches forward, two backward."""

    @staticmethod
    def forward(ctx, disp, img, backend):
        B, _, h, w = disp.shape
        disp, img = disp.contiguous(), img.contiguous()
        backend._check(disp, img)
        chunks = backend.smooth_chunks()
        mean = torch.empty(B, chunks, device=disp.device, dtype=torch.float32)   # partial sums of disp
        sums = torch.empty(B, chunks, 2, device=disp.device, dtype=torch.float32)
        backend.run("bbd_smooth_loss_fwd", disp, ptr(disp), ptr(img), ptr(mean), ptr(sums), B, h, w)
        ctx.save_for_backward(disp, img, mean)
        ctx.meta = (backend, chunks)
        tot = sums.sum(dim=(0, 1))
        return tot[0] / (B * h * (w - 1)) + tot[1] / (B * (h - 1) * w)

    @staticmethod
    def backward(ctx, g):
        disp, img, mean = ctx.saved_tensors
        backend, chunks = ctx.meta
        B, _, h, w = disp.shape
        gscale = g.reshape(1).contiguous().to(torch.float32)
        grad = torch.empty_like(disp)
        dots = torch.empty(B, chunks, device=disp.device, dtype=torch.float32)
        backend.run("bbd_smooth_loss_bwd", disp, ptr(disp), ptr(img), ptr(mean), ptr(gscale), ptr(grad), ptr(dots),
                    B, h, w)
        return grad, None, None


class _SmoothLossMulti(torch.autograd.Function):
    """The smoothness terms of ALL scales of a step (trainer.py:560-564 inside the scale loop) as one launch pair each way
    (bbd_smooth_loss_multi_*): MD2's four scales took 16 launches.  Returns the [S] vector of smooth values."""
    _den = {}

    @staticmethod
    def forward(ctx, backend, n, *tensors):
        disps = [t.contiguous() for t in tensors[:n]]
        imgs = [t.contiguous() for t in tensors[n:]]
        backend._check(*disps, *imgs)
        B, dev = disps[0].shape[0], disps[0].device
        chunks = backend.smooth_chunks()
        mean = torch.empty(n, B, chunks, device=dev, dtype=torch.float32)
        sums = torch.empty(n, B, chunks, 2, device=dev, dtype=torch.float32)
        backend.run("bbd_smooth_loss_multi_fwd", disps[0], _ptr_array(disps), _ptr_array(imgs), _hw_array(disps), ptr(mean),
                    ptr(sums), n, B)
        ctx.save_for_backward(mean, *disps, *imgs)
        ctx.meta = (backend, chunks, n)
        key = (str(dev), B) + tuple(tuple(d.shape[-2:]) for d in disps)
        den = _SmoothLossMulti._den.get(key)
        if den is None:       # mean over the x-terms' B*h*(w-1) and the y-terms' B*(h-1)*w elements (layers.py:213-216)
            from .steptables import upload_single      # (pinned + asynchronous: legal wherever this node first runs)
            den = upload_single([[B * d.shape[-2] * (d.shape[-1] - 1), B * (d.shape[-2] - 1) * d.shape[-1]] for d in disps],
                                dev, torch.float32)
            _SmoothLossMulti._den[key] = den
        return (sums.sum(dim=(1, 2)) / den).sum(dim=1)

    @staticmethod
    def backward(ctx, g):
        backend, chunks, n = ctx.meta
        mean = ctx.saved_tensors[0]
        disps, imgs = ctx.saved_tensors[1:1 + n], ctx.saved_tensors[1 + n:]
        B = disps[0].shape[0]
        gscale = g.contiguous().to(torch.float32)
        grads = [torch.empty_like(d) for d in disps]
        dots = torch.empty(n, B, chunks, device=mean.device, dtype=torch.float32)
        backend.run("bbd_smooth_loss_multi_bwd", disps[0], _ptr_array(disps), _ptr_array(imgs), _hw_array(disps), ptr(mean),
                    ptr(gscale), _ptr_array(grads), ptr(dots), n, B)
        return (None, None) + tuple(grads) + (None,) * n


def normalised_smooth_losses(disps, imgs, backend=None):
    """[S] tensor: normalised_smooth_loss of every (disp, img) pair, one launch pair each way (at most 4 scales)."""
    return _SmoothLossMulti.apply(backend or default_backend(), len(disps), *disps, *imgs)


def normalised_smooth_loss(disp, img, backend=None):
    """layers.get_smooth_loss(disp / (disp.mean(2,True).mean(3,True) + 1e-7), img)  (trainer.py:560-563)."""
    return _SmoothLoss.apply(disp, img, backend or default_backend())


# ---------------------------------------------------------------------------- per-scale losses -> total (trainer.py:557-568)
class _CombineLosses(torch.autograd.Function):
    """per[s] = loss_sum[s] / n_px + w[s] * smooth[s];  total = sum(per) / num_scales  (trainer.py:557, :563-564, :566-568).
    As scalar torch ops this was ~25 launches forward and ~45 backward per step (divisions, multiplications, additions and
    their autograd nodes on one-element tensors - the eager hot path is launch-bound, profiles/r04/hot_path_launches.txt);
    here it is 4 + 3 on [S]-vectors, the backward being two constants times the incoming gradient."""
    _w = {}

    @staticmethod
    def forward(ctx, loss_sum, smooths, n_px, smoothness, scales, num_scales):
        key = (str(loss_sum.device), float(smoothness), tuple(scales))
        w = _CombineLosses._w.get(key)
        if w is None:       # disparity_smoothness / 2**s in fp32: scaling by a power of two commutes with the rounding
            from .steptables import upload_single
            w = upload_single((torch.tensor([float(smoothness)] * len(scales), dtype=torch.float32) /
                               torch.tensor([2.0 ** s for s in scales], dtype=torch.float32)), loss_sum.device, torch.float32)
            _CombineLosses._w[key] = w
        per = torch.addcmul(loss_sum / n_px, smooths, w)
        total = per.sum() / num_scales
        ctx.save_for_backward(w)
        ctx.meta = (float(n_px), float(num_scales))
        return total, per

    @staticmethod
    def backward(ctx, g_total, g_per):
        (w,) = ctx.saved_tensors
        n_px, num_scales = ctx.meta
        g = (g_total / num_scales).expand_as(w)
        if g_per is not None:
            g = g + g_per
        return g / n_px, g * w, None, None, None, None


def combine_losses(loss_sum, smooths, n_px, smoothness, scales, num_scales):
    """(total, per-scale [S]) of the step's loss from the fused launch's per-scale sums and the smoothness terms."""
    return _CombineLosses.apply(loss_sum, smooths, n_px, smoothness, scales, num_scales)


# ---------------------------------------------------------------------------- pose composition
FUSED_POSE_COMPOSE = switch("BBD_FUSED_POSE_COMPOSE")


class ComposeTable:
    """Host-built description of every composed 4x4 of a step (include/bbd_hip.h, bbd_pose_compose_fwd): rows =
    [(chain of step-row indices, direct row | -1, flags)], plus the inverse table the backward walks."""

    def __init__(self, rows, n_steps):
        import numpy as np
        self.NO, self.R = len(rows), n_steps
        tab = np.zeros((max(self.NO, 1), COMPOSE_STRIDE), dtype=np.int32)
        refs = [[] for _ in range(n_steps)]
        for o, (chain, direct, flags) in enumerate(rows):
            assert len(chain) <= 7
            tab[o, 0] = len(chain)
            tab[o, 1:1 + len(chain)] = chain
            tab[o, 8], tab[o, 9] = direct, flags
            for k, r in enumerate(chain):
                refs[r].append((o, k))
            if direct >= 0 and (flags & COMPOSE_REPLACE):
                refs[direct].append((o, -1))
        off = np.zeros(n_steps + 1, dtype=np.int32)
        for r in range(n_steps):
            off[r + 1] = off[r] + len(refs[r])
        flat = np.array([e for rr in refs for e in rr], dtype=np.int32).reshape(-1, 2)
        if flat.shape[0] == 0:
            flat = np.zeros((1, 2), dtype=np.int32)
        self.np = (tab, off, flat)
        self._dev = {}

    def device(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(a).to(device).contiguous() for a in self.np)
        return self._dev[key]


class _PoseCompose(torch.autograd.Function):
    @staticmethod
    def forward(ctx, steps, table, pose_error, backend):
        steps = steps.contiguous()
        tab, off, refs = table.device(steps.device)
        out = torch.empty(table.NO, 4, 4, device=steps.device, dtype=torch.float32)
        backend._check(steps)
        backend.run("bbd_pose_compose_fwd", steps, ptr(steps), ptr(tab), ptr(out), table.NO, float(pose_error))
        ctx.save_for_backward(steps)
        ctx.meta = (table, backend)
        return out

    @staticmethod
    def backward(ctx, gout):
        (steps,) = ctx.saved_tensors
        table, backend = ctx.meta
        tab, off, refs = table.device(steps.device)
        gout = gout.contiguous()
        gsteps = torch.empty_like(steps)
        backend.run("bbd_pose_compose_bwd", steps, ptr(steps), ptr(tab), ptr(off), ptr(refs), ptr(gout), ptr(gsteps),
                    table.R)
        return gsteps, None, None, None


def pose_compose(steps, table, pose_error, backend=None):
    """steps [R,4,4] -> [NO,4,4]: every chained / error-induced / partially swapped pose of the step, one launch."""
    return _PoseCompose.apply(steps, table, pose_error, backend or default_backend())


class _PoseComposeStatic(torch.autograd.Function):
    """`_PoseCompose` on tables that are views of the step's static table buffer (`pooled.PooledStep`): NO rows of which
    the trailing ones are constant no-op rows, `off` = R + 1 entries."""

    @staticmethod
    def forward(ctx, steps, tab, off, refs, NO, pose_error, backend):
        steps = steps.contiguous()
        out = torch.empty(NO, 4, 4, device=steps.device, dtype=torch.float32)
        backend._check(steps, tab, off, refs)
        assert off.numel() == steps.shape[0] + 1 and tab.shape[0] >= NO
        backend.run("bbd_pose_compose_fwd", steps, ptr(steps), ptr(tab), ptr(out), NO, float(pose_error))
        ctx.save_for_backward(steps, tab, off, refs)
        ctx.backend = backend
        return out

    @staticmethod
    def backward(ctx, gout):
        steps, tab, off, refs = ctx.saved_tensors
        gout = gout.contiguous()
        gsteps = torch.empty_like(steps)
        ctx.backend.run("bbd_pose_compose_bwd", steps, ptr(steps), ptr(tab), ptr(off), ptr(refs), ptr(gout), ptr(gsteps),
                        steps.shape[0])
        return gsteps, None, None, None, None, None, None


def pose_compose_static(steps, tab, off, refs, NO, pose_error, backend=None):
    return _PoseComposeStatic.apply(steps, tab, off, refs, NO, pose_error, backend or default_backend())


# ---------------------------------------------------------------------------- identity pre-pass
def identity_losses(plan, frame_tensors, target, no_ssim=False, backend=None):
    """[NI,H,W] identity photometric losses (no gradient: inputs are images)."""
    backend = backend or default_backend()
    B, _, H, W = target.shape
    tb = plan.tables(target.device)
    ident = torch.empty(plan.NI, H, W, device=target.device, dtype=torch.float32)
    backend._check(target, *_frame_list(frame_tensors))
    frames = frame_pointer_array(frame_tensors)
    # one workgroup per (target sample, tile) walks the sample's identity candidates (round 3).  Round 5 measured a streaming,
    # LDS-free form against it - slower (tools/experiments/streaming_identity.hip.txt, profiles/r05/identity_forms.txt), round 6
    # the form with aligned 8-byte loads and the halo columns over DPP - slower too (profiles/r06/identity_stream_ab.txt)
    backend.run("bbd_identity_loss_grouped_fwd", target, frames, ptr(target), ptr(tb["items"]), ptr(tb["ident_off"]),
                plan.B, ptr(ident), H, W, int(no_ssim))
    return ident


def gather_pairs(pool, idx_a, idx_b, normalize=None, backend=None):
    """[R, 6, H, W]: row r = cat(pool[idx_a[r]], pool[idx_b[r]]) of the frame pool [F, 3, H, W] - the batched pose pass's input
    in the pooled form - in one launch; `normalize = (mean, std)` folds the encoder's `(x - mean) / std` in (evaluated like
    PyTorch-ROCm does: subtract, then multiply by the float reciprocal of std).  No gradient: the pool holds images."""
    import numpy as np
    backend = backend or default_backend()
    F, C, H, W = pool.shape
    R = idx_a.numel()
    assert pool.is_contiguous() and idx_a.dtype == torch.int32 and idx_b.dtype == torch.int32 and idx_b.numel() == R
    backend._check(pool, idx_a, idx_b)
    idx_a, idx_b = idx_a.contiguous(), idx_b.contiguous()        # held until the launch: a temporary's memory is reused at once
    out = torch.empty(R, 2 * C, H, W, device=pool.device, dtype=torch.float32)
    sub, mul = (0.0, 1.0) if normalize is None else (float(np.float32(normalize[0])),
                                                     float(np.float32(1.0) / np.float32(normalize[1])))
    backend.run("bbd_gather_pairs", pool, ptr(pool), ptr(idx_a), ptr(idx_b), ptr(out), R, C * H * W, sub, mul)
    return out


# ---------------------------------------------------------------------------- pose table
def pose_table(plan, K, inv_K, poses):
    """[NP,40] rows  K[:3,:] | T | inv_K[:3,:3] | pad, differentiable w.r.t. the poses.

    `poses[(kind, f)]` is the [n_job,4,4] transform of warp job (kind, f) with rows in
    plan.jobs[f] order.  K/inv_K rows are taken by count like the reference (trainer.py:431-432).
    The kernels form P = (K@T)[:3,:] themselves (reference CPU rounding order, bbd_math.h).
    """
    tb = plan.tables(K.device)
    T_all = torch.cat([poses[job] for job in plan.pose_jobs], dim=0)
    return pose_table_rows(T_all, K.index_select(0, tb["k_rows"]), inv_K.index_select(0, tb["k_rows"]))


def pose_table_rows(T_all, K_all, iK_all):
    """[NP,40] pose-table rows from the already gathered per-row matrices ([NP,4,4] each)."""
    NP = T_all.shape[0]
    pad = torch.zeros(NP, POSE_STRIDE - 37, device=T_all.device, dtype=torch.float32)
    return torch.cat([K_all[:, :3, :].reshape(NP, 12), T_all.reshape(NP, 16),
                      iK_all[:, :3, :3].reshape(NP, 9), pad], dim=1).contiguous()


# ---------------------------------------------------------------------------- fused warp+SSIM+min
def _kt_times(K3, gP):
    """K[:3,:]^T @ dL/dP for every pose row ([NP,3,4] x [NP,3,4] -> [NP,4,4]) as a broadcast multiply + a three-term sum:
    no BLAS call on the hot path.  The batch count NP changes with every batch signature of the boosted recipe, and a batched
    GEMM of a new shape can make rocBLAS load another kernel library on the spot (1.6 s on the training thread, measured)."""
    prod = K3.unsqueeze(3) * gP.unsqueeze(2)            # [NP,3,4,1] * [NP,3,1,4] -> [NP,3,4,4]
    return (prod[:, 0] + prod[:, 1]) + prod[:, 2]


class _FusedReprojectionMin(torch.autograd.Function):
    """depth [S,B,H,W], pose table [NP,40] -> per-scale sum of the per-pixel minimum loss."""

    @staticmethod
    def forward(ctx, depth, proj, target, ident, noise, plan, frame_tensors, no_ssim, materialize, backend):
        S, B, H, W = depth.shape
        dev = depth.device
        tb = plan.tables(dev)
        ntiles = backend.num_tiles_fwd(H, W)
        depth, proj = depth.contiguous(), proj.contiguous()
        min_loss = torch.empty(S, B, H, W, device=dev, dtype=torch.float32)
        argmin = torch.empty(S, B, H, W, device=dev, dtype=torch.uint8)
        partial = torch.empty(S, B, ntiles, device=dev, dtype=torch.float32)
        warped = torch.empty(S, plan.NP, 3, H, W, device=dev, dtype=torch.float32) if materialize else None
        backend._check(depth, proj, target, ident, noise, *_frame_list(frame_tensors))
        frames = frame_pointer_array(frame_tensors)
        # pose table (K | T | inv_K) -> projection table (P | inv_K), once per step
        ptab = torch.empty(plan.NP, PROJ_STRIDE, device=dev, dtype=torch.float32)
        backend.run("bbd_pose_expand", proj, ptr(proj), ptr(ptab), plan.NP)
        backend.run("bbd_warp_ssim_min_fwd", depth, frames, ptr(target), ptr(depth), ptr(ptab), ptr(ident),
                    ptr(noise), ptr(tb["cand"]), ptr(tb["ncand"]), ptr(min_loss), ptr(argmin), ptr(partial),
                    ptr(warped), S, B, plan.NP, H, W, int(no_ssim))
        ctx.save_for_backward(depth, proj, target, argmin, ptab)
        ctx.meta = (plan, frame_tensors, frames, int(no_ssim), backend, backend.num_tiles_bwd(H, W))
        ctx.mark_non_differentiable(min_loss, argmin)
        outs = (partial.view(S, -1).sum(dim=1), min_loss, argmin)
        if materialize:
            ctx.mark_non_differentiable(warped)
            return outs + (warped,)
        return outs + (None,)

    @staticmethod
    def backward(ctx, g_sum, *_unused):
        depth, proj, target, argmin, ptab = ctx.saved_tensors
        plan, frame_tensors, frames, no_ssim, backend, ntiles = ctx.meta
        S, B, H, W = depth.shape
        dev = depth.device
        tb = plan.tables(dev)
        gscale = g_sum.contiguous().to(torch.float32)
        grad_depth = torch.empty_like(depth)
        gp_partial = torch.empty(S, plan.NP, ntiles, 12, device=dev, dtype=torch.float32)
        backend.run("bbd_warp_ssim_min_bwd", depth, frames, ptr(target), ptr(depth), ptr(ptab), ptr(tb["cand"]),
                    ptr(tb["ncand"]), ptr(argmin), ptr(gscale), ptr(grad_depth), ptr(gp_partial),
                    S, B, plan.NP, H, W, no_ssim)
        # dL/dT = K[:3,:]^T @ dL/dP  (P = (K@T)[:3,:]); K and inv_K columns get no gradient
        gP = gp_partial.sum(dim=(0, 2)).view(plan.NP, 3, 4)
        gT = _kt_times(proj[:, :12].view(plan.NP, 3, 4), gP)
        grad_pose = torch.zeros_like(proj)
        grad_pose[:, 12:28] = gT.reshape(plan.NP, 16)
        return grad_depth, grad_pose, None, None, None, None, None, None, None, None


def _ptr_array(tensors):
    arr = (ctypes.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        assert t.is_contiguous() and t.dtype == torch.float32
        arr[i] = t.data_ptr()
    return arr


def _hw_array(tensors):
    arr = (ctypes.c_int32 * (2 * len(tensors)))()
    for i, t in enumerate(tensors):
        arr[2 * i], arr[2 * i + 1] = t.shape[-2], t.shape[-1]
    return arr


class _FusedReprojectionMinDisp(torch.autograd.Function):
    """The fused launch fed with the decoder's disparity maps themselves: bilinear up-sampling +
    disp_to_depth happen per staged pixel inside the kernels, no depth buffer is read, and the backward folds
    d depth / d disparity in; only the bilinear adjoint of the reduced scales is a second (single) launch.
    Returns (loss_sum [S], min_loss, argmin, warped | None, depth [S,B,H,W] | None)."""

    @staticmethod
    def forward(ctx, proj, target, ident, noise, plan, frame_tensors, no_ssim, materialize, want_depth, min_depth,
                max_depth, backend, *disps):
        disps = [d.contiguous() for d in disps]
        S, B = len(disps), disps[0].shape[0]
        H, W = target.shape[-2:]
        dev = target.device
        tb = plan.tables(dev)
        ntiles = backend.num_tiles_fwd(H, W)
        proj = proj.contiguous()
        min_loss = torch.empty(S, B, H, W, device=dev, dtype=torch.float32)
        argmin = torch.empty(S, B, H, W, device=dev, dtype=torch.uint8)
        partial = torch.empty(S, B, ntiles, device=dev, dtype=torch.float32)
        warped = torch.empty(S, plan.NP, 3, H, W, device=dev, dtype=torch.float32) if materialize else None
        depth = torch.empty(S, B, H, W, device=dev, dtype=torch.float32) if want_depth else None
        backend._check(proj, target, ident, noise, *disps, *_frame_list(frame_tensors))
        frames = frame_pointer_array(frame_tensors)
        ptab = torch.empty(plan.NP, PROJ_STRIDE, device=dev, dtype=torch.float32)
        backend.run("bbd_pose_expand", proj, ptr(proj), ptr(ptab), plan.NP)
        backend.run("bbd_warp_ssim_min_disp_fwd", target, frames, ptr(target), _ptr_array(disps), _hw_array(disps),
                    float(min_depth), float(max_depth), ptr(ptab), ptr(ident), ptr(noise), ptr(tb["cand"]),
                    ptr(tb["ncand"]), ptr(backend.fused_work_items(plan, S, H, W, False, dev)), ptr(min_loss), ptr(argmin),
                    ptr(partial), ptr(warped), ptr(depth), S, B, plan.NP, H, W, int(no_ssim))
        # the depth by-product is handed to the caller (outputs[("depth",0,s)], NOT differentiable: a depth-based
        # regulariser must use disp_to_depth / opt.fused_disp=False) AND read by the backward: saving it
        # through autograd makes an in-place edit by the caller an error instead of a silently corrupted gradient
        ctx.has_depth = depth is not None
        ctx.save_for_backward(proj, target, argmin, ptab, *([depth] if depth is not None else []), *disps)
        ctx.meta = (plan, frame_tensors, frames, int(no_ssim), backend, float(min_depth), float(max_depth))
        ctx.mark_non_differentiable(min_loss, argmin)
        if materialize:
            ctx.mark_non_differentiable(warped)
        if want_depth:
            ctx.mark_non_differentiable(depth)
        return partial.view(S, -1).sum(dim=1), min_loss, argmin, warped, depth

    @staticmethod
    def backward(ctx, g_sum, *_unused):
        proj, target, argmin, ptab = ctx.saved_tensors[:4]
        depth = ctx.saved_tensors[4] if ctx.has_depth else None
        disps = ctx.saved_tensors[5:] if ctx.has_depth else ctx.saved_tensors[4:]
        plan, frame_tensors, frames, no_ssim, backend, lo, hi = ctx.meta
        S, B = len(disps), disps[0].shape[0]
        H, W = target.shape[-2:]
        dev = target.device
        tb = plan.tables(dev)
        gscale = g_sum.contiguous().to(torch.float32)
        grad_up = torch.empty(S, B, H, W, device=dev, dtype=torch.float32)
        ntb = backend.num_tiles_bwd(H, W)
        # (a plan view over static tables has more pose-table rows than the step uses: the launch never writes those)
        make = torch.zeros if getattr(plan, "zero_partials", False) else torch.empty
        gp_partial = make(S, plan.NP, ntb, 12, device=dev, dtype=torch.float32)
        backend.run("bbd_warp_ssim_min_disp_bwd", target, frames, ptr(target), _ptr_array(disps), _hw_array(disps), lo, hi,
                    ptr(depth), ptr(ptab), ptr(tb["cand"]), ptr(tb["ncand"]), ptr(backend.fused_work_items(plan, S, H, W, True, dev)),
                    ptr(argmin), ptr(gscale), ptr(grad_up), ptr(gp_partial), S, B, plan.NP, H, W, no_ssim)
        # a scale at full resolution: grad_up IS its disparity gradient; the reduced ones share one adjoint launch
        grads, small, small_g, small_up = [None] * S, [], [], []
        for i, d in enumerate(disps):
            if tuple(d.shape[-2:]) == (H, W):
                grads[i] = grad_up[i].unsqueeze(1)
            else:
                grads[i] = torch.empty_like(d)
                small.append(d)
                small_g.append(grads[i])
                small_up.append(grad_up[i])
        if small:
            backend.run("bbd_disp_upsample_adjoint", grad_up, _ptr_array(small_up), _hw_array(small), _ptr_array(small_g),
                        len(small), B, H, W)
        gP = gp_partial.sum(dim=(0, 2)).view(plan.NP, 3, 4)
        gT = _kt_times(proj[:, :12].view(plan.NP, 3, 4), gP)
        grad_pose = torch.zeros_like(proj)
        grad_pose[:, 12:28] = gT.reshape(plan.NP, 16)
        return (grad_pose,) + (None,) * 11 + tuple(grads)


def fused_reprojection_min_disp(disps, proj, target, ident, noise, plan, frame_tensors, min_depth, max_depth,
                                no_ssim=False, materialize=False, want_depth=True, backend=None):
    """[("disp", s)] maps in, (loss_sum [S], min_loss, argmin, warped | None, depth [S,B,H,W] | None) out."""
    return _FusedReprojectionMinDisp.apply(proj, target, ident, noise, plan, frame_tensors, bool(no_ssim),
                                           bool(materialize), bool(want_depth), min_depth, max_depth,
                                           backend or default_backend(), *disps)


def fused_reprojection_min(depth, proj, target, ident, noise, plan, frame_tensors, no_ssim=False,
                           materialize=False, backend=None):
    """Returns (loss_sum [S], min_loss [S,B,H,W], argmin u8 [S,B,H,W], warped [S,NP,3,H,W] | None)."""
    return _FusedReprojectionMin.apply(depth, proj, target, ident, noise, plan, frame_tensors, bool(no_ssim),
                                       bool(materialize), backend or default_backend())


# ---------------------------------------------------------------------------- stand-alone layers (autograd)
class _Backproject(torch.autograd.Function):
    """layers.BackprojectDepth.forward (layers.py:160-167) with its closed-form backward."""

    @staticmethod
    def forward(ctx, depth, inv_K, H, W, backend):
        n = len(inv_K)
        depth, inv_K = depth.contiguous(), inv_K.contiguous()
        backend._check(depth, inv_K)
        pts = torch.empty(n, 4, H * W, device=depth.device, dtype=torch.float32)
        backend.run("bbd_backproject_fwd", depth, ptr(depth), ptr(inv_K), ptr(pts), n, H, W)
        ctx.save_for_backward(inv_K)
        ctx.meta = (n, H, W, depth.shape, backend)
        return pts

    @staticmethod
    def backward(ctx, grad_points):
        (inv_K,) = ctx.saved_tensors
        n, H, W, shape, backend = ctx.meta
        if ctx.needs_input_grad[1]:
            raise NotImplementedError("BackprojectDepth: no gradient w.r.t. inv_K (camera intrinsics are constants "
                                      "of the reference's training path)")
        grad_points = grad_points.contiguous()
        grad_depth = torch.empty(n, H, W, device=grad_points.device, dtype=torch.float32)
        backend.run("bbd_backproject_bwd", grad_points, ptr(grad_points), ptr(inv_K), ptr(grad_depth), n, H, W)
        return grad_depth.view(shape), None, None, None, None


def backproject(depth, inv_K, H, W, backend=None):
    return _Backproject.apply(depth, inv_K, H, W, backend or default_backend())


class _Project3D(torch.autograd.Function):
    """layers.Project3D.forward (layers.py:181-195); backward gives d points, d T and d K."""

    @staticmethod
    def forward(ctx, points, K, T, H, W, eps, backend):
        n = len(K)
        points, K, T = points.contiguous(), K.contiguous(), T.contiguous()
        backend._check(points, K, T)
        grid = torch.empty(n, H, W, 2, device=points.device, dtype=torch.float32)
        backend.run("bbd_project3d_fwd", points, ptr(points), ptr(K), ptr(T), ptr(grid), n, H, W, float(eps))
        ctx.save_for_backward(points, K, T)
        ctx.meta = (n, H, W, float(eps), backend)
        return grid

    @staticmethod
    def backward(ctx, grad_grid):
        points, K, T = ctx.saved_tensors
        n, H, W, eps, backend = ctx.meta
        grad_grid = grad_grid.contiguous()
        grad_points = torch.empty_like(points)
        blocks = backend.lib.project3d_bwd_blocks
        gp_partial = torch.empty(n, blocks, 12, device=points.device, dtype=torch.float32)
        backend.run("bbd_project3d_bwd", points, ptr(points), ptr(K), ptr(T), ptr(grad_grid), ptr(grad_points),
                    ptr(gp_partial), n, H, W, eps)
        gP = gp_partial.sum(dim=1).view(n, 3, 4)                    # dL/dP,  P = (K @ T)[:3, :]
        grad_K = grad_T = None
        if ctx.needs_input_grad[1]:
            grad_K = torch.zeros_like(K)
            grad_K[:, :3, :] = torch.matmul(gP, T.transpose(1, 2))
        if ctx.needs_input_grad[2]:
            grad_T = torch.matmul(K[:, :3, :].transpose(1, 2), gP)
        return grad_points, grad_K, grad_T, None, None, None, None


def project3d(points, K, T, H, W, eps=1e-7, backend=None):
    return _Project3D.apply(points, K, T, H, W, eps, backend or default_backend())


class _SSIMMap(torch.autograd.Function):
    """layers.SSIM.forward (layers.py:235-249), [n,3k,H,W] x2 -> same shape; differentiable in both."""

    @staticmethod
    def forward(ctx, x, y, backend):
        x, y = x.contiguous(), y.contiguous()
        backend._check(x, y)
        n, c, H, W = x.shape
        assert (n * c) % 3 == 0, "SSIM kernels work on groups of three colour planes"
        out = torch.empty_like(x)
        backend.run("bbd_ssim_fwd", x, ptr(x), ptr(y), ptr(out), (n * c) // 3, H, W)
        ctx.save_for_backward(x, y)
        ctx.backend = backend
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, y = ctx.saved_tensors
        backend = ctx.backend
        n, c, H, W = x.shape
        grad_out = grad_out.contiguous()
        gx = gy = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            backend.run("bbd_ssim_bwd", x, ptr(x), ptr(y), ptr(grad_out), ptr(gx), (n * c) // 3, H, W)
        if ctx.needs_input_grad[1]:       # the SSIM expression is symmetric in its two arguments
            gy = torch.empty_like(y)
            backend.run("bbd_ssim_bwd", x, ptr(y), ptr(x), ptr(grad_out), ptr(gy), (n * c) // 3, H, W)
        return gx, gy, None


def ssim_map(x, y, backend=None):
    return _SSIMMap.apply(x, y, backend or default_backend())


# ---------------------------------------------------------------------------- MonoViT: depth-wise conv on tokens
def _slice_ptr(t, c0):
    return ctypes.c_void_p(t.data_ptr() + 4 * c0)


class SharedGrads:
    """Gradient accumulation for parameters that several layers of one sequential chain share (MPViT's MHCAEncoder: the
    blocks of a path share one ConvPosEnc and one ConvRelPosEnc).  As plain autograd every extra use costs an
    AccumulateGrad add per parameter - ~270 tiny launches per MonoViT step, each a cross-stream fork/join inside the
    step graph.  Here the layers' weight-gradient launches add into ONE buffer per parameter (the kernel's `accumulate`
    mode; backward runs the layers last to first, on one stream) and only the chain's first layer hands it to autograd."""

    def __init__(self):
        self.buf = {}
        self.last = {}

    def target(self, key, like, index, count):
        """(buffer to write the gradient into, accumulate flag) for layer `index` of `count`.  One sink belongs to ONE
        forward pass of the chain (MHCAEncoder.forward makes a fresh pair per call), so two forwards before a backward, or
        a second backward through a retained graph, cannot meet in one buffer; inside a pass the layers must arrive
        last to first - anything else (nodes of a partial autograd.grad pass interleaved out of order) is refused rather
        than summed wrongly."""
        if key in self.buf and index >= self.last[key]:
            raise RuntimeError("shared position-encoding gradients: layer %d after layer %d in one backward pass "
                               "(set BBD_FUSED_TOKEN_GLUE=0 for per-layer gradients)" % (index, self.last[key]))
        start = key not in self.buf                          # the layer whose backward runs first starts the sum
        if start:
            self.buf[key] = torch.empty_like(like)
        self.last[key] = index
        return self.buf[key], 0 if start else 1

    def result(self, key, index):
        """What the layer returns to autograd for this parameter: the finished sum from layer 0, nothing from the others."""
        if index != 0:
            return None
        self.last.pop(key, None)
        return self.buf.pop(key)


def _wgrad_target(share, tag, like):
    if share is None:
        return torch.empty_like(like), 0
    sink, index, count = share
    return sink.target(tag, like, index, count)


def _wgrad_result(share, tag, tensor):
    if share is None:
        return tensor
    sink, index, _ = share
    return sink.result(tag, index)


def _i32_array(values):
    return (ctypes.c_int32 * len(values))(*[int(v) for v in values])


def _addr_array(tensors):
    """Host array of device addresses (0 for None)."""
    arr = (ctypes.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        if t is not None:
            assert t.is_contiguous() and t.dtype == torch.float32
            arr[i] = t.data_ptr()
    return arr


def _dw_group_args(splits, weights):
    c0, at = [], 0
    for n in splits:
        c0.append(at)
        at += n
    return len(splits), _i32_array(c0), _i32_array(splits), _i32_array([w.shape[-1] for w in weights])


def _dwconv_groups_fwd(backend, x, x_base, x_row, y, y_base, y_row, splits, weights, biases, B, H, W, add_input, flip):
    """One launch for all channel groups (several window sizes); `*_base`: first channel of the slice inside the rows."""
    n, c0, cn, k = _dw_group_args(splits, weights)
    backend.run("bbd_dwconv_tokens_groups_fwd", x, _slice_ptr(x, x_base), x_row, _slice_ptr(y, y_base), y_row, n, c0, cn, k,
                _addr_array(weights), _addr_array(biases), B, H, W, int(add_input), int(flip))


def _dwconv_groups_wgrad(backend, x, x_base, x_row, gy, gy_base, gy_row, splits, weights, gws, gbs, B, H, W, accumulate):
    n, c0, cn, k = _dw_group_args(splits, weights)
    scratch = torch.empty(backend.lib.dwconv_tokens_groups_wgrad_scratch_floats(B, H, W, n, cn, k), device=x.device, dtype=torch.float32)
    backend.run("bbd_dwconv_tokens_groups_wgrad", x, _slice_ptr(x, x_base), x_row, _slice_ptr(gy, gy_base), gy_row, ptr(scratch),
                n, c0, cn, k, _addr_array(gws), _addr_array(gbs), B, H, W, int(accumulate))


class _DepthwiseTokens(torch.autograd.Function):
    """Depth-wise k x k convolutions over token-layout activations [B, H*W, C] (csrc/bbd_vit.hip): channel
    groups `splits` use their own (weight [n,1,k,k], bias [n]) - MPViT's ConvRelPosEnc gives head groups
    windows 3 / 5 / 7, ConvPosEnc is one group with the residual folded in (`add_input`).  `x` may be a
    channel-slice view of wider rows (v inside the packed qkv activation)."""

    @staticmethod
    def forward(ctx, x, H, W, add_input, backend, splits, share, *params):
        B, N, C = x.shape
        assert N == H * W and sum(splits) == C and x.dtype == torch.float32
        if x.stride(2) != 1 or x.stride(0) != N * x.stride(1):
            x = x.contiguous()
        backend._check(x, *params)
        y = torch.empty(B, N, C, device=x.device, dtype=torch.float32)
        if len(splits) > 1:
            _dwconv_groups_fwd(backend, x, 0, x.stride(1), y, 0, C, splits, [params[2 * i].contiguous() for i in range(len(splits))],
                               [params[2 * i + 1] for i in range(len(splits))], B, H, W, add_input, 0)
        else:
            w, b = params[0].contiguous(), params[1]
            backend.run("bbd_dwconv_tokens_fwd", x, ptr(x) if x.is_contiguous() else _slice_ptr(x, 0), x.stride(1), ptr(w), ptr(b),
                        ptr(y), C, B, H, W, C, w.shape[-1], int(add_input), 0)
        ctx.save_for_backward(x, *params)
        ctx.meta = (H, W, bool(add_input), backend, tuple(splits), share)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, params = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        H, W, add_input, backend, splits, share = ctx.meta
        B, N, C = x.shape
        gy = gy.contiguous()
        gx = torch.empty(B, N, C, device=x.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        ws = [params[2 * i].contiguous() for i in range(len(splits))]
        bs = [params[2 * i + 1] for i in range(len(splits))]
        gws, gbs, acc = [], [], 0
        for i, (w, b) in enumerate(zip(ws, bs)):
            gw, acc = _wgrad_target(share, ("w", i), w)
            gws.append(gw)
            gbs.append(_wgrad_target(share, ("b", i), b)[0] if b is not None else None)
        if len(splits) > 1:
            if gx is not None:
                _dwconv_groups_fwd(backend, gy, 0, C, gx, 0, C, splits, ws, [None] * len(ws), B, H, W, add_input, 1)
            _dwconv_groups_wgrad(backend, x, 0, x.stride(1), gy, 0, C, splits, ws, gws, gbs, B, H, W, acc)
        else:
            k = ws[0].shape[-1]
            if gx is not None:
                backend.run("bbd_dwconv_tokens_fwd", gy, ptr(gy), C, ptr(ws[0]), ptr(None), ptr(gx), C, B, H, W, C, k, int(add_input), 1)
            scratch = torch.empty(backend.lib.dwconv_tokens_wgrad_scratch_floats(B, H, W, C, k), device=x.device, dtype=torch.float32)
            backend.run("bbd_dwconv_tokens_wgrad", x, _slice_ptr(x, 0), x.stride(1), ptr(gy), C, ptr(scratch), ptr(gws[0]), ptr(gbs[0]),
                        B, H, W, C, k, acc)
        grads = []
        for i, b in enumerate(bs):
            grads += [_wgrad_result(share, ("w", i), gws[i]), _wgrad_result(share, ("b", i), gbs[i]) if b is not None else None]
        return (gx, None, None, None, None, None, None) + tuple(grads)


def dwconv_tokens(x, size, convs, add_input=False, backend=None, share=None):
    """`convs`: list of nn.Conv2d (depth-wise, stride 1, padding k//2) covering consecutive channel groups.
    `share` = (SharedGrads, layer index, layer count) when the convs' parameters are shared by a chain of layers."""
    params, splits = [], []
    for conv in convs:
        params += [conv.weight, conv.bias]
        splits.append(conv.weight.shape[0])
    return _DepthwiseTokens.apply(x, size[0], size[1], add_input, backend or default_backend(), tuple(splits), share, *params)


class _FactorAttention(torch.autograd.Function):
    """MPViT's factorised attention on the packed qkv activation (csrc/bbd_vit.hip):
    out = q (scale * softmax_N(k)^T v) + q * convv, per head.  qkv [B,N,3C] is the qkv Linear's output,
    convv [B,N,C] the ConvRelPosEnc convolution of v."""

    @staticmethod
    def forward(ctx, qkv, convv, heads, scale, backend):
        B, N, C3 = qkv.shape
        C = C3 // 3
        Ch = C // heads
        qkv, convv = qkv.contiguous(), convv.contiguous()
        backend._check(qkv, convv)
        dev = qkv.device
        kmax = torch.empty(B, C, device=dev, dtype=torch.float32)
        krsum = torch.empty(B, C, device=dev, dtype=torch.float32)
        ctxs = torch.empty(B, C * Ch, device=dev, dtype=torch.float32)
        scratch = torch.empty(backend.lib.factor_att_scratch_floats(B, N, C, Ch), device=dev, dtype=torch.float32)
        out = torch.empty(B, N, C, device=dev, dtype=torch.float32)
        backend.run("bbd_factor_att_fwd", qkv, ptr(qkv), ptr(convv), ptr(kmax), ptr(krsum), ptr(ctxs), ptr(scratch),
                    ptr(out), B, N, C, Ch, float(scale))
        ctx.save_for_backward(qkv, convv, kmax, krsum, ctxs)
        ctx.meta = (heads, float(scale), backend)
        return out

    @staticmethod
    def backward(ctx, gout):
        qkv, convv, kmax, krsum, ctxs = ctx.saved_tensors
        heads, scale, backend = ctx.meta
        B, N, C3 = qkv.shape
        C = C3 // 3
        Ch = C // heads
        gout = gout.contiguous()
        dev = qkv.device
        dctx = torch.empty_like(ctxs)
        scratch = torch.empty(backend.lib.factor_att_scratch_floats(B, N, C, Ch), device=dev, dtype=torch.float32)
        gqkv = torch.empty_like(qkv)
        gconvv = torch.empty_like(convv)
        backend.run("bbd_factor_att_bwd", qkv, ptr(qkv), ptr(convv), ptr(kmax), ptr(krsum), ptr(ctxs), ptr(gout),
                    ptr(dctx), ptr(scratch), ptr(gqkv), ptr(gconvv), B, N, C, Ch, scale)
        return gqkv, gconvv, None, None, None


class _FactorAttentionCRPE(torch.autograd.Function):
    """`_FactorAttention` with the ConvRelPosEnc convolution of v inside the node: v is read in place from the packed qkv
    activation and - the point - its data gradient is ADDED in place to the v third of the attention's gqkv.  As two
    nodes autograd materialises the slice's gradient (a zero fill of [B,N,3C], a strided copy) and adds the two
    [B,N,3C] tensors: three passes over the widest activation of the block, per block."""

    @staticmethod
    def forward(ctx, qkv, heads, scale, H, W, backend, splits, share, *params):
        B, N, C3 = qkv.shape
        C = C3 // 3
        Ch = C // heads
        assert N == H * W and sum(splits) == C
        qkv = qkv.contiguous()
        backend._check(qkv, *params)
        dev = qkv.device
        convv = torch.empty(B, N, C, device=dev, dtype=torch.float32)
        _dwconv_groups_fwd(backend, qkv, 2 * C, C3, convv, 0, C, splits, [params[2 * i].contiguous() for i in range(len(splits))],
                           [params[2 * i + 1] for i in range(len(splits))], B, H, W, 0, 0)
        kmax = torch.empty(B, C, device=dev, dtype=torch.float32)
        krsum = torch.empty(B, C, device=dev, dtype=torch.float32)
        ctxs = torch.empty(B, C * Ch, device=dev, dtype=torch.float32)
        scratch = torch.empty(backend.lib.factor_att_scratch_floats(B, N, C, Ch), device=dev, dtype=torch.float32)
        out = torch.empty(B, N, C, device=dev, dtype=torch.float32)
        backend.run("bbd_factor_att_fwd", qkv, ptr(qkv), ptr(convv), ptr(kmax), ptr(krsum), ptr(ctxs), ptr(scratch),
                    ptr(out), B, N, C, Ch, float(scale))
        ctx.save_for_backward(qkv, convv, kmax, krsum, ctxs, *params)
        ctx.meta = (heads, float(scale), H, W, backend, tuple(splits), share)
        return out

    @staticmethod
    def backward(ctx, gout):
        qkv, convv, kmax, krsum, ctxs = ctx.saved_tensors[:5]
        params = ctx.saved_tensors[5:]
        heads, scale, H, W, backend, splits, share = ctx.meta
        B, N, C3 = qkv.shape
        C = C3 // 3
        Ch = C // heads
        gout = gout.contiguous()
        dev = qkv.device
        dctx = torch.empty_like(ctxs)
        scratch = torch.empty(backend.lib.factor_att_scratch_floats(B, N, C, Ch), device=dev, dtype=torch.float32)
        gqkv = torch.empty_like(qkv)
        gconvv = torch.empty_like(convv)
        backend.run("bbd_factor_att_bwd", qkv, ptr(qkv), ptr(convv), ptr(kmax), ptr(krsum), ptr(ctxs), ptr(gout),
                    ptr(dctx), ptr(scratch), ptr(gqkv), ptr(gconvv), B, N, C, Ch, scale)
        ws = [params[2 * i].contiguous() for i in range(len(splits))]
        bs = [params[2 * i + 1] for i in range(len(splits))]
        gws, gbs, acc = [], [], 0
        for i, (w, b) in enumerate(zip(ws, bs)):
            gw, acc = _wgrad_target(share, ("w", i), w)
            gws.append(gw)
            gbs.append(_wgrad_target(share, ("b", i), b)[0] if b is not None else None)
        # data gradient of the convolutions, accumulated into the v third of gqkv; then the weight gradients - one launch each
        _dwconv_groups_fwd(backend, gconvv, 0, C, gqkv, 2 * C, C3, splits, ws, [None] * len(ws), B, H, W, 2, 1)
        _dwconv_groups_wgrad(backend, qkv, 2 * C, C3, gconvv, 0, C, splits, ws, gws, gbs, B, H, W, acc)
        grads = []
        for i, b in enumerate(bs):
            grads += [_wgrad_result(share, ("w", i), gws[i]), _wgrad_result(share, ("b", i), gbs[i]) if b is not None else None]
        return (gqkv, None, None, None, None, None, None, None) + tuple(grads)


def factor_attention_crpe(qkv, size, convs, heads, scale, backend=None, share=None):
    """Factorised attention with MPViT's ConvRelPosEnc of v computed inside (`convs`: its depth-wise nn.Conv2d list;
    `share`: see dwconv_tokens)."""
    params, splits = [], []
    for conv in convs:
        params += [conv.weight, conv.bias]
        splits.append(conv.weight.shape[0])
    return _FactorAttentionCRPE.apply(qkv, heads, scale, size[0], size[1], backend or default_backend(), tuple(splits), share,
                                      *params)


def factor_attention(qkv, convv, heads, scale, backend=None):
    return _FactorAttention.apply(qkv, convv, heads, scale, backend or default_backend())


def factor_attention_supported(C, heads, backend=None):
    """The library's limits only (`bbd_factor_att_supported`): no switch, no tensor kind - `mpvit._hip_tokens` has those."""
    return bool((backend or default_backend()).lib.factor_att_supported(C, C // heads))


class _ResidualLayerNorm(torch.autograd.Function):
    """y = x + branch * mask[b];  z = LayerNorm(y)  on [B, N, C] tokens in one pass each way (csrc/bbd_tokens.hip).
    `branch is None`: plain LayerNorm of x (returns z only).  `mask`: [B] stochastic-depth scale (0 or 1/keep) or None."""

    @staticmethod
    def forward(ctx, x, branch, mask, weight, bias, eps, backend, passthrough=False):
        B, N, C = x.shape
        x = x.contiguous()
        backend._check(x, branch, mask, weight, bias)
        if branch is not None:
            branch = branch.contiguous()
        y = torch.empty_like(x) if branch is not None else x
        z = torch.empty_like(x)
        stats = torch.empty(B * N, 2, device=x.device, dtype=torch.float32)
        backend.run("bbd_token_ln_fwd", x, ptr(x), ptr(branch), ptr(mask), ptr(weight), ptr(bias),
                    ptr(y) if branch is not None else ptr(None), ptr(z), ptr(stats), B * N, N, C, float(eps))
        ctx.save_for_backward(y, stats, weight, mask)
        ctx.meta = (backend, branch is not None, bool(passthrough))
        if branch is not None:
            return y, z
        # `passthrough`: x is handed back as an OUTPUT of this node (a view), so a caller that goes on using it (the
        # residual) sends that gradient here and the kernel adds it to LayerNorm's - no separate add
        return (x.view_as(x), z) if passthrough else z

    @staticmethod
    def backward(ctx, *grads):
        y, stats, weight, mask = ctx.saved_tensors
        backend, has_branch, passthrough = ctx.meta
        gy, gz = (grads if (has_branch or passthrough) else (None, grads[0]))
        B, N, C = y.shape
        if gz is None:                     # z unused downstream: only the residual carries gradient
            gz = torch.zeros_like(y)
        gz = gz.contiguous()
        gy = gy.contiguous() if gy is not None else None
        gx = torch.empty_like(y)
        gbranch = torch.empty_like(y) if has_branch else None
        gw, gb = torch.empty_like(weight), torch.empty_like(weight)
        scratch = torch.empty(backend.lib.token_ln_scratch_floats(B * N, C), device=y.device, dtype=torch.float32)
        backend.run("bbd_token_ln_bwd", gz, ptr(gz), ptr(gy), ptr(y), ptr(stats), ptr(weight), ptr(mask), ptr(gx), ptr(gbranch),
                    ptr(scratch), ptr(gw), ptr(gb), B * N, N, C)
        return gx, gbranch, None, gw, gb, None, None, None


class _ResidualAdd(torch.autograd.Function):
    """y = x + branch * mask[b] (one launch instead of a broadcast multiply and an add)."""

    @staticmethod
    def forward(ctx, x, branch, mask, backend):
        B, N, C = x.shape
        x, branch = x.contiguous(), branch.contiguous()
        backend._check(x, branch, mask)
        y = torch.empty_like(x)
        backend.run("bbd_token_ln_fwd", x, ptr(x), ptr(branch), ptr(mask), ptr(None), ptr(None), ptr(y), ptr(None), ptr(None),
                    B * N, N, C, 0.0)
        ctx.save_for_backward(mask)
        return y

    @staticmethod
    def backward(ctx, gy):
        (mask,) = ctx.saved_tensors
        return gy, (gy if mask is None else gy * mask.view(-1, 1, 1)), None, None


class _LinearTokens(torch.autograd.Function):
    """nn.Linear on [..., C_in] tokens with the bias gradient from `bbd_colsum` (two short launches) instead of ATen's
    generic reduction of the tall-skinny [tokens, C_out] gradient; the three GEMMs stay with hipBLASLt / rocBLAS."""

    @staticmethod
    def forward(ctx, x, weight, bias, backend):
        ctx.save_for_backward(x, weight)
        ctx.meta = (backend, bias is not None)
        return torch.nn.functional.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        backend, has_bias = ctx.meta
        g2 = g.reshape(-1, g.shape[-1])
        if not g2.is_contiguous():
            g2 = g2.contiguous()
        gx = g2.mm(weight).view(x.shape) if ctx.needs_input_grad[0] else None
        gw = g2.t().mm(x.reshape(-1, x.shape[-1])) if ctx.needs_input_grad[1] else None
        gb = None
        if has_bias and ctx.needs_input_grad[2]:
            rows, C = g2.shape
            gb = torch.empty(C, device=g2.device, dtype=torch.float32)
            scratch = torch.empty(backend.lib.colsum_scratch_floats(rows, C), device=g2.device, dtype=torch.float32)
            backend.run("bbd_colsum", g2, ptr(g2), ptr(scratch), ptr(gb), rows, C)
        return gx, gw, gb, None


def linear_tokens(x, linear, backend=None):
    """`linear(x)` for an nn.Linear on GPU fp32 tokens whose output width is a multiple of 4 (else the module itself)."""
    if not (hip_fp32(x) and FUSED_TOKEN_GLUE and linear.out_features % 4 == 0):
        return linear(x)
    return _LinearTokens.apply(x, linear.weight, linear.bias, backend or default_backend())


def token_glue_supported(x, backend=None):
    """The library's limits only (include/bbd_hip.h:1265, `bbd_token_ln_supported`): no switch, no tensor kind."""
    return x.dim() == 3 and bool((backend or default_backend()).lib.token_ln_supported(x.shape[-1]))


def layernorm_tokens(x, norm, backend=None, passthrough=False):
    """nn.LayerNorm `norm` over the channel axis of [B, N, C] tokens; `passthrough`: returns (x, norm(x)) with x routed
    through the node (see _ResidualLayerNorm.forward)."""
    return _ResidualLayerNorm.apply(x, None, None, norm.weight, norm.bias, norm.eps, backend or default_backend(), passthrough)


def residual_layernorm(x, branch, mask, norm, backend=None):
    """(x + branch * mask[b], norm(of that)) - `mask` [B] or None."""
    return _ResidualLayerNorm.apply(x, branch, mask, norm.weight, norm.bias, norm.eps, backend or default_backend())


def residual_add(x, branch, mask, backend=None):
    return _ResidualAdd.apply(x, branch, mask, backend or default_backend())


# ---------------------------------------------------------------------------- BatchNorm (+add) (+ReLU)
BN_MAX_GROUPS = _lib.BN_MAX_GROUPS
_call_groups = None         # the `CallGroups` of the batched pass being run (None = one group, the whole batch)


class CallGroups(collections.namedtuple("CallGroups", "rows untracked table groups bound")):
    """The call groups of a fused BatchNorm: host row counts `rows` with `untracked` trailing padding groups, or a device
    `table` of `groups` groups of at most `bound` rows each (the fields of the other description are None)."""
    __slots__ = ()
    G = property(lambda self: len(self.rows) if self.table is None else self.groups)
    biggest = property(lambda self: max(self.rows) if self.table is None else self.bound)
    infix = property(lambda self: "" if self.table is None else "_dev")          # bbd_bn_act_grouped<infix>_fwd, ...

    def fwd_args(self):
        """What follows `scratch` in the forward entry points; `bwd_args`: in the backward ones."""
        if self.table is not None:
            return ptr(self.table), self.G, self.bound
        return (ctypes.c_int32 * (self.G + 1))(*np.cumsum((0,) + self.rows).tolist()), self.G, self.untracked

    def bwd_args(self):
        return self.fwd_args()[:2 if self.table is None else 3]

    def check(self, N=None):
        """ValueError unless this describes a batch of N rows (None: only what does not depend on the batch)."""
        host = self.table is None
        if not (1 <= self.G <= BN_MAX_GROUPS and ((min(self.rows) > 0 and 0 <= self.untracked < self.G) if host else
                                                  (self.table.dtype == torch.int32 and self.table.numel() >= BN_MAX_GROUPS + 2))):
            raise ValueError("no description of 1 .. %d call groups: %s" % (BN_MAX_GROUPS, tuple(self)))
        if N is not None and (sum(self.rows) != N if host else self.bound > N):
            raise ValueError("ops.bn_call_groups does not describe this batch (%s vs %d rows)" % (self.rows or self.bound, N))
        return self


def call_groups(N):
    """The active description of the call groups, or the single group of a batch of N rows."""
    return _call_groups if _call_groups is not None else CallGroups((N,), 0, None, None, None)


class _CallGroupsScope:
    def __init__(self, groups):
        self.groups = groups

    def __enter__(self):
        global _call_groups
        if self.groups is not None and _call_groups is not None and self.groups.infix != _call_groups.infix:
            raise ValueError("a host and a device description of the call groups are active together")
        self.prev, _call_groups = _call_groups, self.groups
        return self

    def __exit__(self, *exc):
        global _call_groups
        _call_groups = self.prev


def bn_call_groups(rows, padding_groups=0):
    """`with ops.bn_call_groups([n_0, n_1, ...]):` - every fused BatchNorm inside treats its batch as consecutive
    call groups of n_g samples with their own batch statistics: one batched pass of a network computes what the
    reference's separate calls on the sub-batches compute (the pose network: trainer.py:348-418).  `padding_groups`:
    the last that many groups are padding rows - normalised, but the running statistics and num_batches_tracked see
    only the real calls (bbd_bn_act_grouped_fwd, `untracked_groups`).  None or fewer than two groups: no groups."""
    if rows is None or len(rows) <= 1:
        return _CallGroupsScope(None)
    return _CallGroupsScope(CallGroups(tuple(int(r) for r in rows), int(padding_groups), None, None, None).check())


def bn_call_groups_device(table, groups, max_rows):
    """`with ops.bn_call_groups_device(table, G, max_rows):` - the call groups of `bn_call_groups`, read from a DEVICE table
    (int32 [BN_MAX_GROUPS + 2]: rows[0..G], number of tracked groups at index BN_MAX_GROUPS + 1; groups may be empty) by
    `bbd_bn_act_grouped_dev_*`: nothing of the batch signature is in the launch arguments, so one captured step graph
    serves every ordering with the same padded row count (`pooled.PooledStep`).  `max_rows` bounds every group."""
    return _CallGroupsScope(CallGroups(None, None, table, int(groups), int(max_rows)).check())


def check_group_table(section, G, bound, R):
    """ValueError unless the host copy of a packed group table (`bn_call_groups_device`'s layout) is one that launches with
    a grid of G groups and scratch for groups of `bound` rows can take for a pass of R rows: the kernels trust the table."""
    rows, tracked = [int(v) for v in section[:BN_MAX_GROUPS + 1]], int(section[BN_MAX_GROUPS + 1])
    sizes = [b - a for a, b in zip(rows, rows[1:])]
    if not (1 <= G <= BN_MAX_GROUPS and rows[0] == 0 and 0 <= min(sizes) and max(sizes) <= bound
            and all(r == R for r in rows[G:]) and 0 <= tracked <= sum(n > 0 for n in sizes)):
        raise ValueError("group table %s with %d tracked groups: not %d rows in at most %d groups of at most %d rows"
                         % (rows, tracked, R, G, bound))


class _BatchNormAct(torch.autograd.Function):
    """Training-mode BatchNorm2d, optional residual add and ReLU in two launches each way
    (csrc/bbd_nn.hip) - the tail of every ResNet block of the encoders."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, running_mean, running_var, batches, momentum, eps, relu, backend):
        x = x.contiguous()
        N, C, H, W = x.shape
        if residual is not None:
            residual = residual.contiguous()
            assert residual.shape == x.shape
        backend._check(x, weight, bias, residual, running_mean, running_var)
        y = torch.empty_like(x)
        groups = call_groups(N).check(N)
        mean = torch.empty(groups.G, C, device=x.device, dtype=torch.float32)
        invstd = torch.empty(groups.G, C, device=x.device, dtype=torch.float32)
        scratch = torch.empty(backend.lib.bn_grouped_scratch_doubles(groups.biggest, groups.G, C, H * W), device=x.device,
                              dtype=torch.float64)
        backend.run("bbd_bn_act_grouped%s_fwd" % groups.infix, x, ptr(x), ptr(residual), ptr(weight), ptr(bias), ptr(y),
                    ptr(mean), ptr(invstd), ptr(running_mean), ptr(running_var), ptr(batches), ptr(scratch),
                    *groups.fwd_args(), N, C, H * W, float(eps), float(momentum), int(relu))
        # without a residual the backward re-derives the ReLU mask from x (one activation read less per launch)
        ctx.save_for_backward(x, y if (relu and residual is not None) else None, weight, bias, mean, invstd)
        ctx.meta = (bool(relu), residual is not None, backend, groups)
        return y

    @staticmethod
    def backward(ctx, grad_y):
        x, y, weight, bias, mean, invstd = ctx.saved_tensors
        relu, has_res, backend, groups = ctx.meta
        N, C, H, W = x.shape
        grad_y = grad_y.contiguous()
        grad_x = torch.empty_like(x)
        grad_res = torch.empty_like(x) if has_res else None
        grad_w = torch.empty(C, device=x.device, dtype=torch.float32)
        grad_b = torch.empty(C, device=x.device, dtype=torch.float32)
        scratch = torch.empty(backend.lib.bn_grouped_scratch_doubles(groups.biggest, groups.G, C, H * W), device=x.device,
                              dtype=torch.float64)
        backend.run("bbd_bn_act_grouped%s_bwd" % groups.infix, x, ptr(x), ptr(y), ptr(grad_y), ptr(weight), ptr(bias),
                    ptr(mean), ptr(invstd), ptr(grad_x), ptr(grad_res), ptr(grad_w), ptr(grad_b), ptr(scratch),
                    *groups.bwd_args(), N, C, H * W, int(relu))
        return grad_x, grad_w, grad_b, grad_res, None, None, None, None, None, None, None


def batch_norm_act_supported(x):
    """Tensor kind only: `bbd_bn_act_grouped_*` takes any [N,C,H,W] (include/bbd_hip.h:1019).  Its switch is the module's
    (`FusedBatchNorm2d.fused`, BBD_FUSED_BN), and so is the module's mode: `FusedBatchNorm2d.takes_fused_launches`."""
    return hip_fp32(x) and x.dim() == 4


def batch_norm_act(x, weight, bias, residual, running_mean, running_var, momentum, eps, relu, backend=None,
                   num_batches_tracked=None):
    return _BatchNormAct.apply(x, weight, bias, residual, running_mean, running_var, num_batches_tracked, momentum,
                               eps, relu, backend or default_backend())


# ---------------------------------------------------------------------------- ReflectionPad2d(1), MaxPool2d(3,2,1)
class _ReflectPad1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, backend):
        x = x.contiguous()
        N, C, H, W = x.shape
        backend._check(x)
        out = torch.empty(N, C, H + 2, W + 2, device=x.device, dtype=torch.float32)
        backend.run("bbd_reflect_pad1_fwd", x, ptr(x), ptr(out), N * C, H, W)
        ctx.meta = (N, C, H, W, backend)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        N, C, H, W, backend = ctx.meta
        grad_out = grad_out.contiguous()
        grad_in = torch.empty(N, C, H, W, device=grad_out.device, dtype=torch.float32)
        backend.run("bbd_reflect_pad1_bwd", grad_out, ptr(grad_out), ptr(grad_in), N * C, H, W)
        return grad_in, None


def reflect_pad1(x, backend=None):
    """nn.ReflectionPad2d(1) (layers.py:124); gather-form backward instead of ATen's atomics."""
    return _ReflectPad1.apply(x, backend or default_backend())


def reflect_pad1_supported(x):
    """Switch (FUSED_NN), tensor kind and the limits of `bbd_reflect_pad1_*`: H, W >= 2 and at most MAX_PLANES planes
    (the argument check of `bbd_reflect_pad1_fwd` in csrc/bbd_nn.hip; include/bbd_hip.h:1061 declares the call and is silent on them)."""
    return (FUSED_NN and hip_fp32(x) and x.dim() == 4 and min(x.shape[2:]) >= 2
            and x.shape[0] * x.shape[1] <= MAX_PLANES)


class _MaxPool3s2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, backend):
        x = x.contiguous()
        N, C, H, W = x.shape
        backend._check(x)
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        out = torch.empty(N, C, OH, OW, device=x.device, dtype=torch.float32)
        code = torch.empty(N, C, OH, OW, device=x.device, dtype=torch.uint8)
        backend.run("bbd_maxpool3s2_fwd", x, ptr(x), ptr(out), ptr(code), N * C, H, W)
        ctx.save_for_backward(code)
        ctx.meta = (N, C, H, W, backend)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (code,) = ctx.saved_tensors
        N, C, H, W, backend = ctx.meta
        grad_out = grad_out.contiguous()
        grad_in = torch.empty(N, C, H, W, device=grad_out.device, dtype=torch.float32)
        backend.run("bbd_maxpool3s2_bwd", grad_out, ptr(grad_out), ptr(code), ptr(grad_in), N * C, H, W)
        return grad_in, None


def maxpool3s2(x, backend=None):
    """nn.MaxPool2d(kernel_size=3, stride=2, padding=1) of the ResNet stem."""
    return _MaxPool3s2.apply(x, backend or default_backend())


def maxpool3s2_supported(x):
    """Switch (FUSED_NN), tensor kind and the limit of `bbd_maxpool3s2_*`: at most MAX_PLANES planes, any H, W >= 1
    (the argument check of `bbd_maxpool3s2_fwd` in csrc/bbd_nn.hip; include/bbd_hip.h:1063 declares the call and is silent on it)."""
    return FUSED_NN and hip_fp32(x) and x.dim() == 4 and x.shape[0] * x.shape[1] <= MAX_PLANES


# ---------------------------------------------------------------------------- encoder stem: bn1 + ReLU + max-pool
FUSED_STEM = switch("BBD_FUSED_STEM")   # 0: batch_norm_act then maxpool3s2, as before (A/B runs)


def stem_supported(x, rows):
    """Does `bbd_stem_*` take activation `x` [N,C,H,W] whose largest call group has `rows` samples?  (The library's own
    condition: the two-launch BatchNorm form and rows of whole float4s; it refuses everything else.)
    Limits and dtype only (include/bbd_hip.h:1076): no switch, no device - `stem_routed` adds those."""
    return (x.dim() == 4 and x.dtype == torch.float32 and x.shape[3] % 4 == 0 and x.shape[2] >= 1
            and 1 <= rows <= x.shape[0] and x.shape[1] <= MAX_PLANES
            and rows * x.shape[2] * x.shape[3] > _lib.STEM_MIN_ELEMS)


def stem_routed(x):
    """Switches (FUSED_STEM, FUSED_NN), tensor kind and limits: the stem stands for `batch_norm_act` + `maxpool3s2`, so it
    takes what the pool takes and `stem_supported` accepts for the active call groups.  The BatchNorm module's own
    switch and mode are left to the caller (`FusedBatchNorm2d.takes_fused_launches`)."""
    return FUSED_STEM and maxpool3s2_supported(x) and stem_supported(x, call_groups(x.shape[0]).biggest)


class _StemBnReluPool(torch.autograd.Function):
    """`maxpool3s2(batch_norm_act(x, ..., relu=True))` with the pool inside the BatchNorm launches (csrc/bbd_nn.hip,
    bbd_stem_*): two launches each way, y written only on request, no full-size gradient of the pool."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, batches, momentum, eps, want_y, backend):
        x = x.contiguous()
        N, C, H, W = x.shape
        backend._check(x, weight, bias, running_mean, running_var)
        OH, OW = (H - 1) // 2 + 1, W // 2
        y = torch.empty_like(x) if want_y else None
        pooled = torch.empty(N, C, OH, OW, device=x.device, dtype=torch.float32)
        code = torch.empty(N, C, OH, OW, device=x.device, dtype=torch.uint8)
        groups = call_groups(N).check(N)
        mean = torch.empty(groups.G, C, device=x.device, dtype=torch.float32)
        invstd = torch.empty(groups.G, C, device=x.device, dtype=torch.float32)
        scratch = torch.empty(backend.lib.bn_grouped_scratch_doubles(groups.biggest, groups.G, C, H * W), device=x.device,
                              dtype=torch.float64)
        backend.run("bbd_stem%s_fwd" % groups.infix, x, ptr(x), ptr(weight), ptr(bias), ptr(y), ptr(pooled), ptr(code),
                    ptr(mean), ptr(invstd), ptr(running_mean), ptr(running_var), ptr(batches), ptr(scratch),
                    *groups.fwd_args(), N, C, H, W, float(eps), float(momentum))
        ctx.save_for_backward(x, code, weight, bias, mean, invstd)
        ctx.meta = (backend, groups)
        ctx.set_materialize_grads(False)
        return y, pooled

    @staticmethod
    def backward(ctx, grad_y, grad_pooled):
        x, code, weight, bias, mean, invstd = ctx.saved_tensors
        backend, groups = ctx.meta
        N, C, H, W = x.shape
        grad_y = grad_y.contiguous() if grad_y is not None else None
        grad_pooled = grad_pooled.contiguous() if grad_pooled is not None else None
        grad_x = torch.empty_like(x)
        grad_w = torch.empty(C, device=x.device, dtype=torch.float32)
        grad_b = torch.empty(C, device=x.device, dtype=torch.float32)
        scratch = torch.empty(backend.lib.bn_grouped_scratch_doubles(groups.biggest, groups.G, C, H * W), device=x.device,
                              dtype=torch.float64)
        backend.run("bbd_stem%s_bwd" % groups.infix, x, ptr(x), ptr(grad_y), ptr(grad_pooled), ptr(code), ptr(weight),
                    ptr(bias), ptr(mean), ptr(invstd), ptr(grad_x), ptr(grad_w), ptr(grad_b), ptr(scratch),
                    *groups.bwd_args(), N, C, H, W)
        return grad_x, grad_w, grad_b, None, None, None, None, None, None, None


def stem_bn_relu_pool(x, weight, bias, running_mean, running_var, momentum, eps, want_y=True, backend=None,
                      num_batches_tracked=None):
    """The encoder stem's `bn1 + ReLU` and `MaxPool2d(3, 2, 1)` -> (y or None, pooled); see `stem_supported`."""
    return _StemBnReluPool.apply(x, weight, bias, running_mean, running_var, num_batches_tracked, momentum, eps,
                                 bool(want_y), backend or default_backend())


# ---------------------------------------------------------------------------- decoder glue
class _UpCatPad(torch.autograd.Function):
    """ReflectionPad2d(1)(cat(nearest_x2(x), skip)) in one pass each way (decoder glue, csrc/bbd_nn.hip)."""

    @staticmethod
    def forward(ctx, x, skip, backend):
        x = x.contiguous()
        N, C1, h, w = x.shape
        C2 = 0
        if skip is not None:
            skip = skip.contiguous()
            C2 = skip.shape[1]
            assert skip.shape == (N, C2, 2 * h, 2 * w)
        backend._check(x, skip)
        out = torch.empty(N, C1 + C2, 2 * h + 2, 2 * w + 2, device=x.device, dtype=torch.float32)
        backend.run("bbd_upcat_pad1_fwd", x, ptr(x), ptr(skip), ptr(out), N, C1, C2, h, w)
        ctx.meta = (N, C1, C2, h, w, backend)
        return out

    @staticmethod
    def backward(ctx, gout):
        N, C1, C2, h, w, backend = ctx.meta
        gout = gout.contiguous()
        gx = torch.empty(N, C1, h, w, device=gout.device, dtype=torch.float32)
        gs = torch.empty(N, C2, 2 * h, 2 * w, device=gout.device, dtype=torch.float32) if C2 else None
        backend.run("bbd_upcat_pad1_bwd", gout, ptr(gout), ptr(gx), ptr(gs), N, C1, C2, h, w)
        return gx, gs, None


def upcat_pad(x, skip=None, backend=None):
    return _UpCatPad.apply(x, skip, backend or default_backend())


def upcat_pad_supported(x, skip):
    """Switch (FUSED_NN), tensor kind and the plane limit of `bbd_upcat_pad1_*` (include/bbd_hip.h:1139)."""
    n_planes = x.shape[0] * (x.shape[1] + (skip.shape[1] if skip is not None else 0))
    return FUSED_NN and hip_fp32(x, skip) and x.dim() == 4 and n_planes <= MAX_PLANES


class _BiasELU(torch.autograd.Function):
    """ELU(conv_out + bias) in place on the bias-free convolution's output; backward from the saved OUTPUT
    (ELU' = y > 0 ? 1 : y + 1) with the bias gradient in the same pass."""

    @staticmethod
    def forward(ctx, y, bias, backend):
        assert y.is_contiguous()
        N, C, H, W = y.shape
        backend._check(y, bias)
        backend.run("bbd_bias_elu_fwd", y, ptr(y), ptr(bias), N, C, H * W)
        ctx.mark_dirty(y)
        ctx.save_for_backward(y)
        ctx.backend = backend
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        backend = ctx.backend
        N, C, H, W = y.shape
        gy = gy.contiguous()
        gx = torch.empty_like(y)
        gb = torch.empty(C, device=y.device, dtype=torch.float32)
        scratch = torch.empty(backend.lib.bias_elu_scratch_doubles(N, C, H * W), device=y.device, dtype=torch.float64)
        backend.run("bbd_bias_elu_bwd", y, ptr(y), ptr(gy), ptr(gx), ptr(gb), ptr(scratch), N, C, H * W)
        return gx, gb, None


def bias_elu_(conv_out, bias, backend=None):
    return _BiasELU.apply(conv_out, bias, backend or default_backend())


def bias_elu_supported(x, border=0):
    """Switch (FUSED_NN), tensor kind and the limit of `bbd_bias_elu_*` (include/bbd_hip.h:1140: planes of whole float4s).
    `x` [N,C,H,W]: the input of the 3x3 convolution whose output `bias_elu_` is to take, with `border` pixels of padding
    on it already (the output has x's kind and its size without them).  A bias, and a contiguous convolution output, are
    left to the caller (`layers.ConvBlock`)."""
    return FUSED_NN and hip_fp32(x) and ((x.shape[2] - 2 * border) * (x.shape[3] - 2 * border)) % 4 == 0


# ---------------------------------------------------------------------------- decoder glue with bias + ELU inside
# 0: upcat_pad / bias_elu_ / reflect_pad1 one after the other, as before (A/B runs)
FUSED_DECODER_GLUE = switch("BBD_FUSED_DECODER_GLUE")


def _glue_scratch(channels, N, rows, device):
    """the per-workgroup partials of a glue backward's bias gradient (include/bbd_hip.h, BBD_GLUE_ROWS)"""
    n = channels * N * (-(-rows // _lib.GLUE_ROWS))
    return torch.empty(n, device=device, dtype=torch.float64), n


def _glue_tensor(t):
    return hip_fp32(t) and t.is_contiguous()


def upcat_pad_act_supported(z, bias, skip):
    """Does `bbd_upcat_pad_act_*` take the convolution output `z` [N,C1,h,w] with `skip` [N,C2,2h,2w] or None?  Tensor kind
    (contiguous) and limits (include/bbd_hip.h:1164); no switch: `DepthDecoder` asks FUSED_DECODER_GLUE and FUSED_NN first."""
    if z.dim() != 4 or bias is None or not (_glue_tensor(z) and _glue_tensor(bias)):
        return False
    N, C1, h, w = z.shape
    if skip is not None and not (_glue_tensor(skip) and skip.shape == (N, skip.shape[1], 2 * h, 2 * w)):
        return False
    return h >= 1 and w >= 1 and 1 <= N * (C1 + (skip.shape[1] if skip is not None else 0)) <= MAX_PLANES


def bias_elu_pad_supported(z, bias):
    """Does `bbd_bias_elu_pad_*` take the convolution output `z` [N,C,H,W]?  Tensor kind (contiguous) and limits
    (include/bbd_hip.h:1164); no switch, as `upcat_pad_act_supported`."""
    if z.dim() != 4 or bias is None or not (_glue_tensor(z) and _glue_tensor(bias)):
        return False
    N, C, H, W = z.shape
    return H >= 2 and W >= 2 and 1 <= N * C <= MAX_PLANES


class _UpCatPadAct(torch.autograd.Function):
    """`upcat_pad(bias_elu_(z, bias), skip)` in one pass each way; `z` stays as the convolution wrote it and is what the
    backward reads (csrc/bbd_nn.hip, bbd_upcat_pad_act_*)."""

    @staticmethod
    def forward(ctx, z, bias, skip, backend):
        backend._check(z, bias, skip)
        z, bias = z.contiguous(), bias.contiguous()
        N, C1, h, w = z.shape
        C2 = 0
        if skip is not None:
            skip = skip.contiguous()
            C2 = skip.shape[1]
            assert skip.shape == (N, C2, 2 * h, 2 * w)
        out = torch.empty(N, C1 + C2, 2 * h + 2, 2 * w + 2, device=z.device, dtype=torch.float32)
        backend.run("bbd_upcat_pad_act_fwd", z, ptr(z), ptr(bias), ptr(skip), ptr(out), N, C1, C2, h, w)
        ctx.save_for_backward(z, bias)
        ctx.meta = (C2, backend)
        return out

    @staticmethod
    def backward(ctx, gout):
        z, bias = ctx.saved_tensors
        C2, backend = ctx.meta
        N, C1, h, w = z.shape
        gout = gout.contiguous()
        gz = torch.empty_like(z)
        gs = torch.empty(N, C2, 2 * h, 2 * w, device=z.device, dtype=torch.float32) if C2 else None
        gb = torch.empty(C1, device=z.device, dtype=torch.float32)
        scratch, n = _glue_scratch(C1, N, h, z.device)
        backend.run("bbd_upcat_pad_act_bwd", gout, ptr(gout), ptr(z), ptr(bias), ptr(gz), ptr(gs), ptr(gb), ptr(scratch), n,
                    N, C1, C2, h, w)
        return gz, gb, gs, None


def upcat_pad_act(z, bias, skip=None, backend=None):
    """ReflectionPad2d(1)(cat(nearest_x2(ELU(z + bias)), skip)): a ConvBlock's bias + ELU inside `upcat_pad`."""
    return _UpCatPadAct.apply(z, bias, skip, backend or default_backend())


class _BiasEluPad(torch.autograd.Function):
    """`y = bias_elu_(z, bias); yp = reflect_pad1(y)` in one pass each way -> (y, yp); y is z, written in place.  Backward
    takes the gradients of both outputs (either may be missing) in one pass (csrc/bbd_nn.hip, bbd_bias_elu_pad_*)."""

    @staticmethod
    def forward(ctx, z, bias, backend):
        backend._check(z, bias)
        assert z.is_contiguous()
        bias = bias.contiguous()
        N, C, H, W = z.shape
        yp = torch.empty(N, C, H + 2, W + 2, device=z.device, dtype=torch.float32)
        backend.run("bbd_bias_elu_pad_fwd", z, ptr(z), ptr(bias), ptr(yp), N, C, H, W)
        ctx.mark_dirty(z)
        ctx.save_for_backward(z)
        ctx.backend = backend
        ctx.set_materialize_grads(False)
        return z, yp

    @staticmethod
    def backward(ctx, gy, gyp):
        if gy is None and gyp is None:
            return None, None, None
        (y,) = ctx.saved_tensors
        backend = ctx.backend
        N, C, H, W = y.shape
        gy = gy.contiguous() if gy is not None else None
        gyp = gyp.contiguous() if gyp is not None else None
        gz = torch.empty_like(y)
        gb = torch.empty(C, device=y.device, dtype=torch.float32)
        scratch, n = _glue_scratch(C, N, H, y.device)
        backend.run("bbd_bias_elu_pad_bwd", y, ptr(gyp), ptr(gy), ptr(y), ptr(gz), ptr(gb), ptr(scratch), n, N, C, H, W)
        return gz, gb, None


def bias_elu_pad(conv_out, bias, backend=None):
    """(y, yp) = (ELU(conv_out + bias) in place, ReflectionPad2d(1)(y)): a ConvBlock's tail and the next one's border."""
    return _BiasEluPad.apply(conv_out, bias, backend or default_backend())


# ---------------------------------------------------------------------------- ConvBlock weight gradients from NCHW
# 0: every weight gradient stays with MIOpen, as before (A/B runs)
FUSED_WGRAD = switch("BBD_FUSED_WGRAD")

# (C, K, H, W) of a ConvBlock convolution - input channels, output channels, output size - whose weight gradient
# `bbd_conv3x3_wgrad` takes, at any batch size.  A row is here because tools/wgrad_bench.py measured the call's slowest
# repeat faster than MIOpen's fastest at batch 12 (profiles/decoder_wgrad/wgrad_bench.json); every other shape stays with
# MIOpen, those the kernel supports but was not measured on included.
WGRAD_ROUTES = {
    (16, 16, 192, 640),     # DepthDecoder upconv(0,1) at 640 x 192: 1.8 x MIOpen's call
    (32, 16, 96, 320),      # upconv(0,0): 1.7 x
}                           # not here: upconv(1,0) (64, 32, 48, 160), within 10 % either way; upconv(1,1), slower


def conv3x3_wgrad_shape(xp, w):
    """(N, C, K, H, W) of `bbd_conv3x3_wgrad` for the padded input `xp` and the weight `w`, or None where the call does
    not take them: contiguous fp32 GPU tensors, a [K,C,3,3] weight.  Tensor kind and shape; `_routed` adds the rest."""
    if not (xp.dim() == 4 and w.dim() == 4 and _glue_tensor(xp) and _glue_tensor(w)):
        return None
    N, C, Hp, Wp = xp.shape
    if w.shape != (w.shape[0], C, 3, 3) or Hp < 3 or Wp < 3:
        return None
    return N, C, w.shape[0], Hp - 2, Wp - 2


def conv3x3_wgrad_routed(xp, w, backend=None):
    """Does the weight gradient of `F.conv2d(xp, w)` go to `bbd_conv3x3_wgrad`?  Only for the measured rows of
    WGRAD_ROUTES, and never with BBD_FUSED_WGRAD=0 or BBD_FUSED_NN=0.  Switches, tensor kind and the library's limits."""
    if not (FUSED_WGRAD and FUSED_NN):
        return False
    shape = conv3x3_wgrad_shape(xp, w)
    if shape is None or shape[1:] not in WGRAD_ROUTES:
        return False
    return bool((backend or default_backend()).lib.conv3x3_wgrad_supported(*shape))


def conv3x3_wgrad(xp, grad_z, K=None, backend=None):
    """grad_w [K,C,3,3] of `F.conv2d(xp, w)` from xp [N,C,H+2,W+2] and grad_z [N,K,H,W]: two launches, no atomics."""
    backend = backend or default_backend()
    backend._check(xp, grad_z)
    xp, grad_z = xp.contiguous(), grad_z.contiguous()
    N, C, Hp, Wp = xp.shape
    K = grad_z.shape[1] if K is None else K
    H, W = Hp - 2, Wp - 2
    assert grad_z.shape == (N, K, H, W) and xp.dtype == grad_z.dtype == torch.float32
    doubles = backend.lib.conv3x3_wgrad_scratch_doubles(N, C, K, H, W)
    if doubles <= 0:
        raise _lib.BbdError("bbd_conv3x3_wgrad does not take N=%d C=%d K=%d H=%d W=%d" % (N, C, K, H, W))
    scratch = torch.empty(doubles, device=xp.device, dtype=torch.float64)
    grad_w = torch.empty(K, C, 3, 3, device=xp.device, dtype=torch.float32)
    backend.run("bbd_conv3x3_wgrad", xp, ptr(xp), ptr(grad_z), ptr(grad_w), ptr(scratch), N, C, K, H, W)
    return grad_w


class _Conv3x3Valid(torch.autograd.Function):
    """`F.conv2d(xp, w)` of a padded input whose weight gradient comes from `bbd_conv3x3_wgrad`; forward and data gradient
    are MIOpen's, the same problems as without this function."""

    @staticmethod
    def forward(ctx, xp, w, backend):
        ctx.save_for_backward(xp, w)
        ctx.backend = backend
        return torch.nn.functional.conv2d(xp, w, None)

    @staticmethod
    def backward(ctx, grad_z):
        xp, w = ctx.saved_tensors
        grad_x = grad_w = None
        if ctx.needs_input_grad[0]:
            grad_x = torch.ops.aten.convolution_backward(grad_z, xp, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                                                         [True, False, False])[0]
        if ctx.needs_input_grad[1]:
            grad_w = conv3x3_wgrad(xp, grad_z, w.shape[0], ctx.backend)
        return grad_x, grad_w, None


def conv3x3_valid(xp, w, backend=None):
    """`F.conv2d(xp, w)` for a pair `conv3x3_wgrad_routed` accepts."""
    return _Conv3x3Valid.apply(xp, w, backend or default_backend())


# ---------------------------------------------------------------------------- up-sample + pad + 3x3 conv, sub-pixel form
# 0: the finest decoder level keeps upcat_pad_act + convolution, as before (A/B runs)
FUSED_UP2CONV = switch("BBD_FUSED_UP2CONV")

# (C, K, h, w) - channels in and out, size of the low-resolution map - of a decoder level without a skip connection whose
# second ConvBlock `bbd_up2conv3x3_*` takes, at any batch size.  A row is here because tools/up2conv_bench.py measured the
# new call's slowest repeat faster than the composition's fastest at batch 12, forward and full backward each
# (profiles/decoder_up2conv/up2conv_bench.json); every other shape keeps the composition.
UP2CONV_ROUTES = {
    (16, 16, 96, 320),      # DepthDecoder upconv(0,1) at 640 x 192
}


def up2_conv3x3_shape(z, bias, weight):
    """(N, C, K, h, w) of `bbd_up2conv3x3_*` for the convolution output `z`, its bias and the next 3x3 weight, or None
    where the calls do not take them: contiguous fp32 GPU tensors, a [K,C,3,3] weight.  Tensor kind and shape only."""
    if bias is None or not (z.dim() == 4 and weight.dim() == 4 and _glue_tensor(z) and _glue_tensor(bias) and _glue_tensor(weight)):
        return None
    N, C, h, w = z.shape
    if weight.shape != (weight.shape[0], C, 3, 3) or bias.shape != (C,) or min(N, h, w) < 1:
        return None
    return N, C, weight.shape[0], h, w


def up2_conv3x3_routed(z, bias, weight, backend=None):
    """Does `conv2d(upcat_pad_act(z, bias), weight)` go to `bbd_up2conv3x3_*`?  Only for the measured rows of
    UP2CONV_ROUTES, and never with BBD_FUSED_UP2CONV=0, BBD_FUSED_NN=0 or BBD_FUSED_DECODER_GLUE=0.  Switches, tensor kind
    and the library's limits."""
    if not (FUSED_UP2CONV and FUSED_NN and FUSED_DECODER_GLUE):
        return False
    shape = up2_conv3x3_shape(z, bias, weight)
    if shape is None or shape[1:] not in UP2CONV_ROUTES:
        return False
    return bool((backend or default_backend()).lib.up2conv3x3_supported(*shape))


def _weight_grad_of_padded(xp, weight, grad_out, backend):
    """The weight gradient of `conv2d(xp, weight)` as today's composition computes it: `bbd_conv3x3_wgrad` for a routed
    shape, MIOpen otherwise."""
    if conv3x3_wgrad_routed(xp, weight, backend):
        return conv3x3_wgrad(xp, grad_out, weight.shape[0], backend)
    return torch.ops.aten.convolution_backward(grad_out, xp, weight, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                                               [False, True, False])[1]


class _Up2Conv3x3(torch.autograd.Function):
    """`F.conv2d(upcat_pad_act(z, bias, None), weight)` without the up-sampled, padded copy (csrc/bbd_up2conv.hip).  The
    weight gradient is the composition's, bit for bit: the backward writes the copy into a transient buffer for it."""

    @staticmethod
    def forward(ctx, z, bias, weight, backend):
        backend._check(z, bias, weight)
        z, bias, weight = z.contiguous(), bias.contiguous(), weight.contiguous()
        N, C, h, w = z.shape
        K = weight.shape[0]
        if not backend.lib.up2conv3x3_supported(N, C, K, h, w):
            raise _lib.BbdError("bbd_up2conv3x3 does not take N=%d C=%d K=%d h=%d w=%d" % (N, C, K, h, w))
        out = torch.empty(N, K, 2 * h, 2 * w, device=z.device, dtype=torch.float32)
        backend.run("bbd_up2conv3x3_fwd", z, ptr(z), ptr(bias), ptr(weight), ptr(out), N, C, K, h, w)
        ctx.save_for_backward(z, bias, weight)
        ctx.backend = backend
        return out

    @staticmethod
    def backward(ctx, grad_out):
        z, bias, weight = ctx.saved_tensors
        backend = ctx.backend
        N, C, h, w = z.shape
        K = weight.shape[0]
        grad_out = grad_out.contiguous()
        grad_z = grad_bias = grad_w = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            grad_z = torch.empty_like(z)
            grad_bias = torch.empty(C, device=z.device, dtype=torch.float32)
            n = backend.lib.up2conv3x3_scratch_doubles(N, C, K, h, w)
            scratch = torch.empty(n, device=z.device, dtype=torch.float64)
            backend.run("bbd_up2conv3x3_bwd", grad_out, ptr(grad_out), ptr(z), ptr(bias), ptr(weight), ptr(grad_z), ptr(grad_bias),
                        ptr(scratch), n, N, C, K, h, w)
        if ctx.needs_input_grad[2]:
            xp = torch.empty(N, C, 2 * h + 2, 2 * w + 2, device=z.device, dtype=torch.float32)
            backend.run("bbd_upcat_pad_act_fwd", z, ptr(z), ptr(bias), ptr(None), ptr(xp), N, C, 0, h, w)
            grad_w = _weight_grad_of_padded(xp, weight, grad_out, backend)
        return (grad_z if ctx.needs_input_grad[0] else None, grad_bias if ctx.needs_input_grad[1] else None, grad_w, None)


def up2_conv3x3(z, bias, weight, backend=None):
    """conv3x3(ReflectionPad2d(1)(nearest_x2(ELU(z + bias))), weight), bias-free: what `ConvBlock.conv_raw(upcat_pad_act(z,
    bias))` returns, in sub-pixel form."""
    return _Up2Conv3x3.apply(z, bias, weight, backend or default_backend())


# ---------------------------------------------------------------------------- encoder stems: conv1, 7x7 stride 2
# 0: both stems' conv1 stay with MIOpen in both directions, as before (A/B runs)
FUSED_STEMCONV = switch("BBD_FUSED_STEMCONV")

# (C, H, W, direction) - input channels and input size of an encoder's conv1, "fwd" or "wgrad" - that goes to
# `bbd_stem_conv7s2_*`, at any batch size.  A row is here because tools/stemconv_bench.py measured the new call's slowest
# repeat faster than MIOpen's fastest, at batch 12 (C = 3) or 24 (C = 6) (profiles/stem_conv/stemconv_bench.json); every
# other shape and direction stays with MIOpen, those the kernels support but were not measured on included.
STEMCONV_ROUTES = {
    (3, 192, 640, "fwd"),       # depth encoder, N = 12: 100 us against MIOpen's 171 us (medians)
    (3, 192, 640, "wgrad"),     # 143 us against 179 us
    (6, 192, 640, "fwd"),       # pose encoder, N = 24: 359 us against 460 us
}                               # not here: (6, 192, 640, "wgrad"), 419 / 440 / 467 us against MIOpen's 453 / 471 / 506 us
#                                 in one run (slowest repeat above MIOpen's fastest), 413 / 416 / 427 against 452 / 456 /
#                                 471 in a second one (the committed json): passes the rule in one run of two
NORMALIZE_MEAN, NORMALIZE_STD = 0.45, 0.225        # the encoder's input normalisation, folded in by `normalize=True`


def stem_conv_shape(x, w):
    """(N, C, K, H, W, R, S) of `bbd_stem_conv7s2_*` for the image `x` and the weight `w`, or None where the calls cannot
    take them: contiguous fp32 GPU tensors, a [K,C,R,S] weight on x's channels, nothing empty.  Tensor kind and shape only."""
    if not (x.dim() == 4 and w.dim() == 4 and _glue_tensor(x) and _glue_tensor(w)):
        return None
    N, C, H, W = x.shape
    K, Cw, R, S = w.shape
    if Cw != C or min(N, C, H, W, K, R, S) < 1:
        return None
    return N, C, K, H, W, R, S


def stem_conv_routed(x, w, direction, backend=None):
    """Does `direction` ("fwd" or "wgrad") of `conv2d(x, w, stride 2, pad 3)` go to `bbd_stem_conv7s2_*`?  Only for the
    measured rows of STEMCONV_ROUTES, and never with BBD_FUSED_STEMCONV=0 or BBD_FUSED_NN=0.  Switches, tensor kind and
    the library's limits."""
    if not (FUSED_STEMCONV and FUSED_NN):
        return False
    shape = stem_conv_shape(x, w)
    if shape is None or (shape[1], shape[3], shape[4], direction) not in STEMCONV_ROUTES:
        return False
    return bool((backend or default_backend()).lib.stem_conv7s2_supported(*shape))


def _stem_conv_args(x, w, backend):
    backend._check(x, w)
    shape = stem_conv_shape(x, w)
    if shape is None or not backend.lib.stem_conv7s2_supported(*shape):
        raise _lib.BbdError("bbd_stem_conv7s2 does not take x %s, w %s" % (tuple(x.shape), tuple(w.shape)))
    return shape


def stem_conv_fwd(x, w, normalize=False, backend=None):
    """conv2d(x', w, stride 2, pad 3) [N,64,Ho,Wo] in one launch; x' = (x - 0.45) / 0.225 with `normalize`, else x."""
    backend = backend or default_backend()
    N, C, K, H, W, _, _ = _stem_conv_args(x, w, backend)
    out = torch.empty(N, K, (H + 1) // 2, (W + 1) // 2, device=x.device, dtype=torch.float32)
    backend.run("bbd_stem_conv7s2_fwd", x, ptr(x), ptr(w), ptr(out), N, C, K, H, W, int(bool(normalize)))
    return out


def stem_conv_wgrad(x, w, grad_out, normalize=False, backend=None):
    """grad_w [64,C,7,7] of that convolution from x and grad_out [N,64,Ho,Wo] (`w` gives the shape only): two launches,
    no atomics, scratch from the torch allocator."""
    backend = backend or default_backend()
    shape = _stem_conv_args(x, w, backend)
    N, C, K, H, W, _, _ = shape
    backend._check(grad_out)
    grad_out = grad_out.contiguous()
    assert grad_out.shape == (N, K, (H + 1) // 2, (W + 1) // 2) and grad_out.dtype == torch.float32
    doubles = backend.lib.stem_conv7s2_wgrad_scratch_doubles(*shape)
    scratch = torch.empty(doubles, device=x.device, dtype=torch.float64)
    grad_w = torch.empty(K, C, 7, 7, device=x.device, dtype=torch.float32)
    backend.run("bbd_stem_conv7s2_wgrad", x, ptr(x), ptr(grad_out), ptr(grad_w), ptr(scratch), doubles, N, C, K, H, W,
                int(bool(normalize)))
    return grad_w


def _normalized(x):
    return (x - NORMALIZE_MEAN) / NORMALIZE_STD


class _StemConv(torch.autograd.Function):
    """`F.conv2d(x', w, None, 2, 3)` of an encoder's conv1, x' = the normalised image with `normalize`.  Forward and weight
    gradient go to `bbd_stem_conv7s2_*` or to MIOpen independently (`fwd`, `wgrad`); MIOpen's side is the problem it has
    without this function.  An input that requires grad gets MIOpen's data gradient.  With `normalize`, only a function
    routed in BOTH directions never forms x' with torch ops: an unrouted forward forms it as before, and an unrouted weight
    gradient behind a routed forward forms it in the backward (the raw image is what is saved)."""

    @staticmethod
    def forward(ctx, x, w, normalize, fwd, wgrad, backend):
        ctx.normalize, ctx.wgrad, ctx.backend = normalize, wgrad, backend
        if fwd:
            out = stem_conv_fwd(x, w, normalize, backend)
            ctx.save_for_backward(x, w)
            ctx.raw = True
        else:
            xn = _normalized(x) if normalize else x
            out = torch.nn.functional.conv2d(xn, w, None, 2, 3)
            ctx.raw = wgrad                                      # the routed weight gradient re-forms x' from x itself
            ctx.save_for_backward(x if wgrad else xn, w)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, w = ctx.saved_tensors
        grad_x = grad_w = None
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if need_w and ctx.wgrad:
            grad_w = stem_conv_wgrad(x, w, grad_out, ctx.normalize, ctx.backend)
            need_w = False
        if need_x or need_w:
            xn = _normalized(x) if (ctx.normalize and ctx.raw) else x
            gx, gw, _ = torch.ops.aten.convolution_backward(grad_out, xn, w, None, [2, 2], [3, 3], [1, 1], False, [0, 0], 1,
                                                            [need_x, need_w, False])
            if need_x:
                grad_x = gx / NORMALIZE_STD if ctx.normalize else gx
            if need_w:
                grad_w = gw
        return grad_x, grad_w, None, None, None, None


def stem_conv(x, w, normalize=False, backend=None, fwd=None, wgrad=None):
    """An encoder's conv1 on `x` (`normalize`: on `(x - 0.45) / 0.225`), each direction where `stem_conv_routed` sends it
    (`fwd` / `wgrad` override the table: the tests and tools/stemconv_bench.py)."""
    backend = backend or default_backend()
    fwd = stem_conv_routed(x, w, "fwd", backend) if fwd is None else fwd
    wgrad = stem_conv_routed(x, w, "wgrad", backend) if wgrad is None else wgrad
    return _StemConv.apply(x, w, bool(normalize), bool(fwd), bool(wgrad), backend)


# ---------------------------------------------------------------------------- ResNet shortcuts: 1x1, stride 2
# 0: every shortcut convolution stays with MIOpen in all three directions and BasicBlock runs its two entry convolutions
# as separate autograd nodes, as before (A/B runs)
FUSED_CONV1X1 = switch("BBD_FUSED_CONV1X1")

# (C, K, H, W, direction) - channels and INPUT size of a `layer{2,3,4}.0.downsample.0`, "fwd", "dgrad" or "wgrad" - that
# goes to `bbd_conv1x1s2_*`, at any batch size.  A row is here because tools/conv1x1_bench.py measured the new call's
# slowest repeat faster than MIOpen's fastest at batch 12 AND at batch 24 (the depth and the pose encoder share the
# shapes; profiles/conv1x1/conv1x1_bench.json); every other shape and direction stays with MIOpen, those the kernels
# support but were not measured on included.
CONV1X1_ROUTES = {              # whole call, medians in us, new against MIOpen, at N = 12 / N = 24
    (64, 128, 48, 160, "fwd"),      # layer2: 20 against 39 / 28 against 50
    (64, 128, 48, 160, "dgrad"),    # 22 against 48 / 26 against 62
    (64, 128, 48, 160, "wgrad"),    # 36 against 43 / 47 against 58
    (128, 256, 24, 80, "fwd"),      # layer3: 21 against 33 / 26 against 45
    (128, 256, 24, 80, "dgrad"),    # 24 against 43 / 28 against 52
    (256, 512, 12, 40, "fwd"),      # layer4: 22 against 31 / 29 against 41
    (256, 512, 12, 40, "dgrad"),    # 33 against 39 / 34 against 45
}                                   # not here: layer3 "wgrad" (34 against 40 at N = 12, but 45.3 / 46.0 / 49.2 against MIOpen's
#                                     46.6 / 46.8 / 48.9 at N = 24) and layer4 "wgrad" (31.2 / 32.2 / 35.1 against 33.6 / 34.8 / 36.2
#                                     and 41.2 / 44.5 / 46.3 against 44.4 / 45.2 / 46.6): the slowest repeat is above MIOpen's fastest
# (C, K, H, W) of a shortcut whose block takes `block_entry` - its two entry convolutions as one autograd node, the
# shortcut's data gradient added into conv1's in place - where the "dgrad" row above is routed too: the shapes at which
# tools/conv1x1_bench.py measured the joint backward faster than conv1's backward + MIOpen's shortcut gradient + the ATen
# add, by the same rule at both batches.  Elsewhere a routed shortcut runs `conv1x1_s2` beside the module's conv1.
BLOCK_ENTRY_ROUTES = {(64, 128, 48, 160)}      # layer2: 162 against 191 / 248 against 293 us; layers 3 and 4 did not pass
#                                                (164.5 against 178.3 / 242.2 against 267.3 and 166.6 against 166.2 / 231.7
#                                                against 241.7 in the medians, the ranges overlap)


def conv1x1s2_shape(x, w):
    """(N, C, K, H, W) of `bbd_conv1x1s2_*` for the input `x` and the weight `w`, or None where the calls cannot take
    them: contiguous fp32 GPU tensors, a [K,C,1,1] weight on x's channels, nothing empty.  Tensor kind and shape only."""
    if not (x.dim() == 4 and w.dim() == 4 and _glue_tensor(x) and _glue_tensor(w)):
        return None
    N, C, H, W = x.shape
    K, Cw, R, S = w.shape
    if Cw != C or (R, S) != (1, 1) or min(N, C, H, W, K) < 1:
        return None
    return N, C, K, H, W


def conv1x1s2_routed(x, w, direction, backend=None):
    """Does `direction` ("fwd", "dgrad" or "wgrad") of `conv2d(x, w, stride 2)` go to `bbd_conv1x1s2_*`?  Only for the
    measured rows of CONV1X1_ROUTES, and never with BBD_FUSED_CONV1X1=0 or BBD_FUSED_NN=0.  Switches, tensor kind and
    the library's limits."""
    if not (FUSED_CONV1X1 and FUSED_NN):
        return False
    shape = conv1x1s2_shape(x, w)
    if shape is None or (shape[1], shape[2], shape[3], shape[4], direction) not in CONV1X1_ROUTES:
        return False
    return bool((backend or default_backend()).lib.conv1x1s2_supported(*shape))


def block_entry_routed(x, w1, backend=None):
    """Does the block that reads `x` take `block_entry`?  The shortcut's data gradient is routed and its shape is a row of
    BLOCK_ENTRY_ROUTES."""
    if not conv1x1s2_routed(x, w1, "dgrad", backend):
        return False
    return tuple(conv1x1s2_shape(x, w1)[1:]) in BLOCK_ENTRY_ROUTES


def _conv1x1s2_args(x_shape, w, backend, *tensors):
    backend._check(w, *tensors)
    N, C, H, W = x_shape
    K = w.shape[0]
    ok = (w.dim() == 4 and tuple(w.shape[1:]) == (C, 1, 1) and all(_glue_tensor(t) for t in (w,) + tensors)
          and backend.lib.conv1x1s2_supported(N, C, K, H, W))
    if not ok:
        raise _lib.BbdError("bbd_conv1x1s2 does not take x %s, w %s" % (tuple(x_shape), tuple(w.shape)))
    return N, C, K, H, W


def conv1x1s2_fwd(x, w, backend=None):
    """conv2d(x, w, stride 2) [N,K,Ho,Wo] of a [K,C,1,1] weight in one launch."""
    backend = backend or default_backend()
    N, C, K, H, W = _conv1x1s2_args(x.shape, w, backend, x)
    out = torch.empty(N, K, (H + 1) // 2, (W + 1) // 2, device=x.device, dtype=torch.float32)
    backend.run("bbd_conv1x1s2_fwd", x, ptr(x), ptr(w), ptr(out), N, C, K, H, W)
    return out


def conv1x1s2_bwd_data(grad_out, w, x_shape, into=None, backend=None):
    """The data gradient [N,C,H,W] of that convolution in one launch.  `into` None: a new tensor, every element written
    (the zeros of odd rows and columns too).  `into` a contiguous [N,C,H,W] tensor: the gradient is ADDED to its even
    positions in place, nothing else is touched, and `into` is returned."""
    backend = backend or default_backend()
    grad_out = grad_out.contiguous()
    N, C, K, H, W = _conv1x1s2_args(x_shape, w, backend, grad_out)
    assert grad_out.shape == (N, K, (H + 1) // 2, (W + 1) // 2) and grad_out.dtype == torch.float32
    if into is None:
        grad_x = torch.empty(N, C, H, W, device=grad_out.device, dtype=torch.float32)
    else:
        backend._check(into)
        assert tuple(into.shape) == (N, C, H, W) and _glue_tensor(into)
        grad_x = into
    backend.run("bbd_conv1x1s2_bwd_data", grad_out, ptr(grad_out), ptr(w), ptr(grad_x), N, C, K, H, W, int(into is not None))
    return grad_x


def conv1x1s2_wgrad(x, w, grad_out, backend=None):
    """grad_w [K,C,1,1] of that convolution from x and grad_out [N,K,Ho,Wo] (`w` gives the shape only): two launches, no
    atomics, scratch from the torch allocator."""
    backend = backend or default_backend()
    grad_out = grad_out.contiguous()
    N, C, K, H, W = _conv1x1s2_args(x.shape, w, backend, x, grad_out)
    assert grad_out.shape == (N, K, (H + 1) // 2, (W + 1) // 2) and grad_out.dtype == torch.float32
    doubles = backend.lib.conv1x1s2_wgrad_scratch_doubles(N, C, K, H, W)
    scratch = torch.empty(doubles, device=x.device, dtype=torch.float64)
    grad_w = torch.empty(K, C, 1, 1, device=x.device, dtype=torch.float32)
    backend.run("bbd_conv1x1s2_wgrad", x, ptr(x), ptr(grad_out), ptr(grad_w), ptr(scratch), doubles, N, C, K, H, W)
    return grad_w


def _conv_backward(grad_out, x, w, stride, padding, need_x, need_w):
    """MIOpen's side of a bias-free convolution's backward: (grad_x, grad_w), None where not asked for."""
    gx, gw, _ = torch.ops.aten.convolution_backward(grad_out, x, w, None, [stride, stride], [padding, padding], [1, 1],
                                                    False, [0, 0], 1, [need_x, need_w, False])
    return (gx if need_x else None), (gw if need_w else None)


def _conv1x1s2_backward(ctx_dgrad, ctx_wgrad, backend, grad_out, x, w, need_x, need_w):
    """(grad_x, grad_w) of the shortcut, each from `bbd_conv1x1s2_*` or from MIOpen."""
    grad_x = grad_w = None
    if need_w and ctx_wgrad:
        grad_w, need_w = conv1x1s2_wgrad(x, w, grad_out, backend), False
    if need_x and ctx_dgrad:
        grad_x, need_x = conv1x1s2_bwd_data(grad_out, w, x.shape, None, backend), False
    if need_x or need_w:
        gx, gw = _conv_backward(grad_out, x, w, 2, 0, need_x, need_w)
        grad_x, grad_w = (gx if need_x else grad_x), (gw if need_w else grad_w)
    return grad_x, grad_w


class _Conv1x1S2(torch.autograd.Function):
    """`F.conv2d(x, w, None, 2)` of a ResNet shortcut.  Each of the three directions goes to `bbd_conv1x1s2_*` or to
    MIOpen independently (`fwd`, `dgrad`, `wgrad`); MIOpen's side is the problem it has without this function."""

    @staticmethod
    def forward(ctx, x, w, fwd, dgrad, wgrad, backend):
        ctx.dgrad, ctx.wgrad, ctx.backend = dgrad, wgrad, backend
        ctx.save_for_backward(x, w)
        return conv1x1s2_fwd(x, w, backend) if fwd else torch.nn.functional.conv2d(x, w, None, 2)

    @staticmethod
    def backward(ctx, grad_out):
        x, w = ctx.saved_tensors
        grad_x, grad_w = _conv1x1s2_backward(ctx.dgrad, ctx.wgrad, ctx.backend, grad_out, x, w, ctx.needs_input_grad[0],
                                             ctx.needs_input_grad[1])
        return grad_x, grad_w, None, None, None, None


def conv1x1_s2(x, w, backend=None, fwd=None, dgrad=None, wgrad=None):
    """A ResNet shortcut convolution on `x`, each direction where `conv1x1s2_routed` sends it (`fwd` / `dgrad` / `wgrad`
    override the table: the tests and tools/conv1x1_bench.py)."""
    backend = backend or default_backend()
    fwd = conv1x1s2_routed(x, w, "fwd", backend) if fwd is None else fwd
    dgrad = conv1x1s2_routed(x, w, "dgrad", backend) if dgrad is None else dgrad
    wgrad = conv1x1s2_routed(x, w, "wgrad", backend) if wgrad is None else wgrad
    return _Conv1x1S2.apply(x, w, bool(fwd), bool(dgrad), bool(wgrad), backend)


class _BlockEntry(torch.autograd.Function):
    """The two convolutions that read a down-sampling block's input, `F.conv2d(x, w3, None, 2, 1)` (MIOpen's, both ways)
    and the shortcut `F.conv2d(x, w1, None, 2)`, as ONE node: the backward adds the shortcut's data gradient into the even
    positions of the 3x3 convolution's (`bbd_conv1x1s2_bwd_data`, accumulate mode) instead of writing a tensor that is
    three quarters zeros for autograd to add.  The sum has the composition's values: a two-term fp32 add commutes, and
    the odd positions had 0.0 added to them."""

    @staticmethod
    def forward(ctx, x, w3, w1, fwd, wgrad, backend):
        ctx.wgrad, ctx.backend = wgrad, backend
        ctx.save_for_backward(x, w3, w1)
        y3 = torch.nn.functional.conv2d(x, w3, None, 2, 1)
        y1 = conv1x1s2_fwd(x, w1, backend) if fwd else torch.nn.functional.conv2d(x, w1, None, 2)
        return y3, y1

    @staticmethod
    def backward(ctx, g3, g1):
        x, w3, w1 = ctx.saved_tensors
        need_x, need_w3, need_w1 = ctx.needs_input_grad[:3]
        gx = gw3 = gw1 = None
        if g3 is not None and (need_x or need_w3):
            gx, gw3 = _conv_backward(g3, x, w3, 2, 1, need_x, need_w3)
        if g1 is not None:
            if need_x:
                if gx is not None and not gx.is_contiguous():
                    gx = gx.contiguous()
                gx = conv1x1s2_bwd_data(g1, w1, x.shape, gx, ctx.backend)
            if need_w1:
                _, gw1 = _conv1x1s2_backward(False, ctx.wgrad, ctx.backend, g1, x, w1, False, True)
        return gx, gw3, gw1, None, None, None


def block_entry(x, w3, w1, backend=None, fwd=None, wgrad=None):
    """`(conv2d(x, w3, stride 2, pad 1), conv2d(x, w1, stride 2))` of a down-sampling BasicBlock as one autograd node
    (`_BlockEntry`); the caller has asked `block_entry_routed(x, w1)`.  The shortcut's forward and weight gradient
    go where `conv1x1s2_routed` sends them (`fwd` / `wgrad` override the table)."""
    backend = backend or default_backend()
    fwd = conv1x1s2_routed(x, w1, "fwd", backend) if fwd is None else fwd
    wgrad = conv1x1s2_routed(x, w1, "wgrad", backend) if wgrad is None else wgrad
    return _BlockEntry.apply(x, w3, w1, bool(fwd), bool(wgrad), backend)


# ---------------------------------------------------------------------------- disparity head Conv3x3(C -> 1)
DISP_HEAD_MAX_CHANNELS = 256        # DC_MAXC of csrc/bbd_nn.hip (the weights' shared-memory copy); not in the header


def disp_head_supported(x, channels):
    """`dispconv` and `disp_head` alike: switch (FUSED_NN), tensor kind and the limits of `bbd_dispconv_*` / `bbd_disp_head_*`
    for an `x` of `channels` channels: at most DISP_HEAD_MAX_CHANNELS, H and W >= 2 (the argument checks of the dispconv launchers and DC_MAXC in csrc/bbd_nn.hip; include/bbd_hip.h:1103
    declares the calls and is silent on them; a batch above MAX_PLANES is refused there, with an error, not here).  That the
    layer has ONE output channel and a reflection border is the module's to say (`layers.Conv3x3`)."""
    return FUSED_NN and hip_fp32(x) and channels <= DISP_HEAD_MAX_CHANNELS and min(x.shape[2:]) >= 2


class _DispConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, backend):
        x = x.contiguous()
        N, C, H, W = x.shape
        w = weight.contiguous()
        backend._check(x, w, bias)
        y = torch.empty(N, 1, H, W, device=x.device, dtype=torch.float32)
        backend.run("bbd_dispconv_fwd", x, ptr(x), ptr(w), ptr(bias), ptr(y), N, C, H, W)
        ctx.save_for_backward(x, w)
        ctx.meta = (bias is not None, backend)
        return y

    @staticmethod
    def backward(ctx, grad_y):
        x, w = ctx.saved_tensors
        has_bias, backend = ctx.meta
        N, C, H, W = x.shape
        grad_y = grad_y.contiguous()
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2])
        grad_x = torch.empty_like(x) if need_x else None
        grad_w = torch.empty_like(w) if need_w else None
        grad_b = torch.empty(1, device=x.device, dtype=torch.float32) if (need_w and has_bias) else None
        scratch = torch.empty(backend.lib.dispconv_scratch_doubles(C), device=x.device, dtype=torch.float64)
        backend.run("bbd_dispconv_bwd", x, ptr(x), ptr(w), ptr(grad_y), ptr(grad_x), ptr(grad_w), ptr(grad_b),
                    ptr(scratch), N, C, H, W)
        return grad_x, grad_w, grad_b, None


def dispconv(x, weight, bias, backend=None):
    """layers.Conv3x3(C, 1): reflection pad + 3x3 convolution to ONE channel + bias (the decoder's disparity heads)."""
    return _DispConv.apply(x, weight, bias, backend or default_backend())


class _DispHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, backend):
        x = x.contiguous()
        N, C, H, W = x.shape
        w = weight.contiguous()
        backend._check(x, w, bias)
        disp = torch.empty(N, 1, H, W, device=x.device, dtype=torch.float32)
        backend.run("bbd_disp_head_fwd", x, ptr(x), ptr(w), ptr(bias), ptr(disp), N, C, H, W)
        ctx.save_for_backward(x, w, disp)
        ctx.meta = (bias is not None, backend)
        return disp

    @staticmethod
    def backward(ctx, grad_disp):
        x, w, disp = ctx.saved_tensors
        has_bias, backend = ctx.meta
        N, C, H, W = x.shape
        grad_disp = grad_disp.contiguous()
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2])
        grad_x = torch.empty_like(x) if need_x else None
        grad_w = torch.empty_like(w) if need_w else None
        grad_b = torch.empty(1, device=x.device, dtype=torch.float32) if (need_w and has_bias) else None
        scratch = torch.empty(backend.lib.dispconv_scratch_doubles(C), device=x.device, dtype=torch.float64)
        backend.run("bbd_disp_head_bwd", x, ptr(x), ptr(w), ptr(disp), ptr(grad_disp), ptr(grad_x), ptr(grad_w),
                    ptr(grad_b), ptr(scratch), N, C, H, W)
        return grad_x, grad_w, grad_b, None


def disp_head(x, weight, bias, backend=None):
    """sigmoid(dispconv(x, weight, bias)): the decoder's disparity output in one launch, and a backward that takes the
    gradient through the sigmoid inside the two gradient kernels."""
    return _DispHead.apply(x, weight, bias, backend or default_backend())


# ---------------------------------------------------------------------------- colour-mapped disparity
_MAGMA = {}


def _hex_lut(name, n_rows):
    """uint8 [n_rows,3] from a shipped table of one `rrggbb` row per line."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), name)) as f:
        rows = [line.strip() for line in f if line.strip()]
    assert len(rows) == n_rows and all(len(r) == 6 for r in rows)
    return torch.tensor([[int(r[0:2], 16), int(r[2:4], 16), int(r[4:6], 16)] for r in rows], dtype=torch.uint8)


def magma_lut(device="cpu"):
    """uint8 [256,3]: magma as matplotlib's `to_rgba(...)[..., :3] * 255 -> uint8` yields it.  Read from the shipped
    table (magma_lut.hex, written by tools/make_magma_lut.py); matplotlib is never imported."""
    key = str(device)
    if key not in _MAGMA:
        if "cpu" not in _MAGMA:
            _MAGMA["cpu"] = _hex_lut("magma_lut.hex", 256)
        _MAGMA[key] = _MAGMA["cpu"].to(device)
    return _MAGMA[key]


def viz_granule(npx):
    """Pixels an image of `npx` pixels occupies in the buffers of `disp_viz`: 4-pixel granules, so that every image
    starts on a 4-byte boundary of the colour buffer (packed stores)."""
    return (npx + 3) // 4 * 4


def viz_buffer(views):
    """The one buffer the views returned by `disp_viz` point into (images `viz_granule` pixels apart)."""
    return views[0]._base


def disp_viz(disp, sizes, min_depth=0.1, max_depth=80.0, percentile=95.0, want_float=False, backend=None, raw=False):
    """test_simple.py:135-148 for a batch: network disparities `disp` [n,1,h,w] (sigmoid output) -> per image the
    magma-coloured scaled disparity at its original size `sizes[i] = (H0, W0)` (ragged), normalised between its minimum
    and its `percentile`-th percentile (np.percentile, exact).  One `bbd_disp_viz` call, no host synchronisation.

    Returns (colour, floats, stats): `colour` a list of uint8 [H0,W0,3] views into ONE buffer (`colour[0]._base` - a
    single copy brings all of them to the host), `floats` a list of fp32 [H0,W0] views of the scaled disparity (None
    unless `want_float`), `stats` fp32 [n,4] = vmin, vmax and the two order statistics vmax was interpolated from.

    `raw=True` is validation.py:205-212 instead: the network output itself (s = 0 + 1 * d), normalised between its
    minimum and its maximum (the 100th percentile); `min_depth`, `max_depth` and `percentile` are not used."""
    backend = backend or default_backend()
    disp = disp.detach()
    if disp.dim() == 4:
        assert disp.shape[1] == 1
        disp = disp[:, 0]
    disp = disp.contiguous().float()
    backend._check(disp)
    n, h, w = disp.shape
    assert len(sizes) == n and n > 0
    dev = disp.device
    rows, off = [], 0
    for H0, W0 in sizes:
        assert H0 >= 1 and W0 >= 1 and H0 * W0 < 2 ** 31
        rows.append(split64(off) + (int(H0), int(W0)))
        off += viz_granule(H0 * W0)
    desc = upload(torch.tensor(rows, dtype=torch.int32), dev)
    out = torch.empty(off * 3, dtype=torch.uint8, device=dev)
    outf = torch.empty(off, dtype=torch.float32, device=dev) if want_float else None
    stats = torch.empty(n, 4, dtype=torch.float32, device=dev)
    scratch = torch.empty(backend.lib.disp_viz_scratch_ints(n), dtype=torch.int32, device=dev)
    backend.run("bbd_disp_viz", disp, ptr(disp), ptr(desc), ptr(magma_lut(dev)), ptr(out), ptr(outf), ptr(stats),
                ptr(scratch), n, h, w, *((0.0, 1.0, 100.0) if raw else (1.0 / max_depth, 1.0 / min_depth, float(percentile))))
    colour, floats = [], ([] if want_float else None)
    for (lo, hi, H0, W0) in rows:
        o = join64(lo, hi)
        colour.append(out[3 * o:3 * (o + H0 * W0)].view(H0, W0, 3))
        if want_float:
            floats.append(outf[o:o + H0 * W0].view(H0, W0))
    return colour, floats, stats


# ---------------------------------------------------------------------------- comparison sheets (validation.py)
class _GtBatch:
    """Maps `indices` of a `GroundTruthSet` as one call sees them: the set's descriptor rows with their offsets rebased to
    the first element any of the maps uses, so that the pictures (written at 3x the maps' offsets) need a buffer of the
    batch's span only.  Consecutive indices - a batch of a split - span exactly their own pixels."""

    def __init__(self, gts, indices):
        self.idx = [int(i) for i in indices]
        assert self.idx and all(0 <= i < len(gts) for i in self.idx)
        host = gts.desc_host[self.idx].astype("int64")
        offs = join64(host[:, 0], host[:, 1])
        self.shapes = [tuple(int(v) for v in gts.shapes[i]) for i in self.idx]
        sizes = [gh * gw for gh, gw in self.shapes]
        self.base = int(offs.min())
        self.rel = [int(o) - self.base for o in offs]
        self.span = max(r + s for r, s in zip(self.rel, sizes))
        rows = host.copy()
        rows[:, :2] = [split64(r) for r in self.rel]
        self.desc = upload(rows.astype("int32"), gts.buffer.device)
        self.gt = gts.buffer[self.base:]

    def pictures(self, buf):
        return [buf[3 * r:3 * (r + gh * gw)].view(gh, gw, 3) for r, (gh, gw) in zip(self.rel, self.shapes)]

    def planes(self, buf):
        return [buf[r:r + gh * gw].view(gh, gw) for r, (gh, gw) in zip(self.rel, self.shapes)]


def gt_viz(gts, indices, max_inv=80.0, backend=None):
    """validation.py:250-254 for maps `indices` of the `GroundTruthSet` `gts`: the magma-coloured inverse depth
    (1 / gt, values above `max_inv` zeroed) normalised between its minimum and maximum.  One `bbd_gt_viz` call, no host
    synchronisation.  Returns (pictures, stats): uint8 [GH,GW,3] views into ONE buffer (`viz_buffer(pictures)`), picture
    i at 3x the offset map i has from the first map of the batch, and fp32 [n,2] = vmin, vmax."""
    backend = backend or default_backend()
    b = _GtBatch(gts, indices)
    backend._check(gts.buffer)
    dev, n = gts.buffer.device, len(b.idx)
    out = torch.empty(3 * b.span, dtype=torch.uint8, device=dev)
    stats = torch.empty(n, 2, dtype=torch.float32, device=dev)
    scratch = torch.empty(backend.lib.gt_viz_scratch_ints(n), dtype=torch.int32, device=dev)
    backend.run("bbd_gt_viz", out, ptr(b.gt), ptr(b.desc), ptr(magma_lut(dev)), ptr(out), ptr(stats), ptr(scratch), n,
                float(max_inv))
    return b.pictures(out), stats


def error_map(pred_disp, gts, indices, rows, images=None, min_depth=0.1, max_depth=80.0, scale_factor=1.0, err_max=0.5,
              radius=2, median_scaling=True, want_float=False, backend=None):
    """Where a model is wrong: `pred_disp` ([n,1,h,w] or [n,h,w]) is the scaled disparity `evaluation.depth_metrics` was
    given with `pred_is_disp=True` and `rows` that call's output.  Every valid ground-truth pixel (the pixels the metrics
    score) carries its abs_rel summand |gt - pred| / gt; every output pixel shows, in magma between 0 and `err_max`, the
    largest one within Chebyshev distance `radius` (0-4), and where there is none the darkened grey of `images` (uint8
    HWC at the ground-truth sizes: a list, or ONE buffer laid out like the returned pictures) or black.  One
    `bbd_error_map` call, no host synchronisation.  Returns (pictures, planes): uint8 [GH,GW,3] views into one buffer as
    `gt_viz` returns them, and - with `want_float` - fp32 [GH,GW] views holding the error at valid pixels and NaN
    elsewhere (None otherwise)."""
    backend = backend or default_backend()
    if not 0 <= int(radius) <= _lib.ERROR_MAP_MAX_RADIUS:
        raise ValueError("error_map: radius must be 0 ... %d, got %r" % (_lib.ERROR_MAP_MAX_RADIUS, radius))
    pred = pred_disp.detach()
    if pred.dim() == 4:
        assert pred.shape[1] == 1
        pred = pred[:, 0]
    pred = pred.contiguous().float()
    b = _GtBatch(gts, indices)
    n, h, w = pred.shape
    assert n == len(b.idx)
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (n, _lib.EVAL_OUT) and rows.is_contiguous()
    dev = pred.device
    if images is not None and not torch.is_tensor(images):
        packed = torch.zeros(3 * b.span, dtype=torch.uint8, device=dev)
        for view, im in zip(b.pictures(packed), images):
            assert im.dtype == torch.uint8 and tuple(im.shape) == tuple(view.shape), "pictures are HWC uint8 at the ground-truth size"
            view.copy_(im)
        images = packed
    if images is not None:
        assert images.dtype == torch.uint8 and images.dim() == 1 and images.numel() >= 3 * b.span and images.is_contiguous()
    backend._check(pred, gts.buffer, rows, images)
    out = torch.empty(3 * b.span, dtype=torch.uint8, device=dev)
    outf = torch.empty(b.span, dtype=torch.float32, device=dev) if want_float else None
    backend.run("bbd_error_map", pred, ptr(pred), ptr(b.gt), ptr(b.desc), ptr(rows), ptr(images), ptr(magma_lut(dev)),
                ptr(out), ptr(outf), n, h, w, float(min_depth), float(max_depth), float(scale_factor), float(err_max),
                int(radius), 0 if median_scaling else _lib.EVAL_NO_MEDIAN_SCALING)
    return b.pictures(out), (b.planes(outf) if want_float else None)


# ---------------------------------------------------------------------------- Velodyne depth maps
def velo_depth(points, counts, proj, shapes, out=None, offsets=None, vel_depth=False, backend=None):
    """kitti_utils.py:46-98 (generate_depth_map) for a ragged batch of frames in ONE `bbd_velo_depth` call: a memset
    and two launches, no host synchronisation.

    `points` fp32 [sum(counts), 4] holds the scans back to back as the .bin files store them (x, y, z, reflectance - the
    last column is ignored), `proj` [n,3,4] float64 the projection matrices (`kitti_utils.velo_projection`), `shapes[i]
    = (h, w)`.  Frame i is written to `out[offsets[i] : offsets[i] + h*w]`; without `out` a packed buffer is allocated
    and frames follow one another.  Returns (out, offsets)."""
    backend = backend or default_backend()
    points = points.detach()
    assert points.dtype == torch.float32 and points.dim() == 2 and points.shape[1] == 4
    points = points.contiguous()
    n = len(counts)
    assert n > 0 and len(shapes) == n and sum(counts) == points.shape[0]
    dev = points.device
    proj = torch.as_tensor(proj, dtype=torch.float64).reshape(n, 12).contiguous()
    sizes = [int(h) * int(w) for h, w in shapes]
    assert all(h >= 1 and w >= 1 for h, w in shapes) and all(c >= 0 for c in counts)
    if out is None:
        assert offsets is None
        offsets = [0] * n
        for i in range(1, n):
            offsets[i] = offsets[i - 1] + sizes[i - 1]
        out = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
    assert len(offsets) == n and out.dtype == torch.float32 and out.is_contiguous() and out.device == dev
    assert all(0 <= o and o + s <= out.numel() for o, s in zip(offsets, sizes))
    backend._check(points, out)
    rows, first_point, first_pixel = [], 0, 0
    for (h, w), c, o, s in zip(shapes, counts, offsets, sizes):
        rows.append(split64(int(o)) + (int(h), int(w), int(c), first_point, first_pixel, 0))
        first_point += int(c)
        first_pixel += s
    n_ints = backend.lib.velo_depth_scratch_ints(first_pixel, n)
    if n_ints < 0:
        raise _lib.BbdError("velo_depth: %d pixels in one call are more than the scratch contract holds; "
                            "split the batch" % first_pixel)
    desc = upload(torch.tensor(rows, dtype=torch.int32), dev)
    proj = upload(proj, dev)
    scratch = torch.empty(n_ints, dtype=torch.int32, device=dev)
    backend.run("bbd_velo_depth", out, ptr(points), ptr(desc), ptr(proj), ptr(scratch), n_ints, ptr(out), n,
                int(max(counts)), _lib.VELO_VEL_DEPTH if vel_depth else 0)
    return out, list(offsets)


# ---------------------------------------------------------------------------- all-pairs nearest neighbour
def chamfer_nn(a, b, backend=None):
    """Squared distance of every point to its nearest neighbour in the other set, both ways, in ONE `bbd_chamfer_nn`
    call: a [Na,3], b [Nb,3] float32 -> (nn_a [Na], nn_b [Nb]) float32 with nn_a[i] = min_j |a_i - b_j|^2 and
    nn_b[j] = min_i |a_i - b_j|^2.  The distance is (dx*dx + dy*dy) + dz*dz from the differences, so the result is
    defined to the bit; +inf where the other set is empty.  What the reference's `ChamferDistance()` extension
    returns as its first two outputs (evaluate_depth.py:83)."""
    backend = backend or default_backend()
    a, b = a.detach(), b.detach()
    assert a.dim() == 2 and a.shape[1] == 3 and b.dim() == 2 and b.shape[1] == 3
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.device == b.device
    a, b = a.contiguous(), b.contiguous()
    backend._check(a, b)
    nn_a = torch.empty(a.shape[0], dtype=torch.float32, device=a.device)
    nn_b = torch.empty(b.shape[0], dtype=torch.float32, device=a.device)
    backend.run("bbd_chamfer_nn", a, ptr(a), ptr(b), a.shape[0], b.shape[0], ptr(nn_a), ptr(nn_b))
    return nn_a, nn_b


# ---------------------------------------------------------------------------- coloured point clouds
def cloud_rows(shapes, offsets=None, windows=None):
    """Host table int32 [n, 8] of BBD_EVAL_DESC rows for maps of `shapes[i] = (GH, GW)`: element offset (default: the
    maps lie back to back), size, window `windows[i] = (r0, r1, c0, c1)` (default: the whole image)."""
    rows, off = np.zeros((len(shapes), _lib.EVAL_DESC), dtype=np.int32), 0
    for i, (gh, gw) in enumerate(shapes):
        o = off if offsets is None else int(offsets[i])
        rows[i] = split64(o) + (int(gh), int(gw)) + (tuple(int(v) for v in windows[i]) if windows is not None
                                                       else (0, int(gh), 0, int(gw)))
        off += int(gh) * int(gw)
    return rows


def cloud_capacity(row, stride):
    """Candidate pixels of one descriptor row at `stride`: every stride-th pixel of the window (cut to the image) in
    both directions, starting at its first."""
    gh, gw, r0, r1, c0, c1 = (int(v) for v in row[2:8])
    r0, r1, c0, c1 = max(r0, 0), min(r1, gh), max(c0, 0), min(c1, gw)
    if gh < 1 or gw < 1 or r1 <= r0 or c1 <= c0:
        return 0
    return ((r1 - r0 - 1) // stride + 1) * ((c1 - c0 - 1) // stride + 1)


def point_cloud(pred, rows_desc, inv_K, gt=None, rows=None, rgb=None, stride=1, min_depth=1e-3, max_depth=80.0,
                clamp=(1e-3, 80.0), pred_is_disp=False, scale_factor=1.0, from_gt=False, clamp_depth=False,
                mask_gt=False, rays="pixel", out=None, regions=None, backend=None):
    """The coloured point clouds of a ragged batch in ONE `bbd_point_cloud` call (three launches, nothing read back):
    `pred` ([n,1,h,w] or [n,h,w], depth or - `pred_is_disp` - disparity) is resampled at every `stride`-th pixel of the
    window of image i as `evaluation.depth_metrics` resamples it, multiplied by `rows[i][7]` (that call's output; None:
    1), back-projected through `inv_K` ([3,3], [4,4] or one per image) along the pixel's own ray (`rays="pixel"`) or
    the reference's pairing (`rays="reference"`), and coloured from `rgb` (uint8 device buffer, image i as HWC at 3x its
    element offset) or, without it, magma over inverse depth.  Points outside [min_depth, max_depth] are dropped -
    clamped with `clamp_depth`; `mask_gt` keeps only pixels with min_depth < gt < max_depth; `from_gt` exports the
    ground truth `gt` (float32 device buffer at the offsets of `rows_desc`) instead of the prediction.

    `rows_desc` is a host table of BBD_EVAL_DESC rows (`cloud_rows`, or `GroundTruthSet.desc_host[indices]`).  Image
    i's region starts at vertex `regions[i]` of `out` (uint8, 16 bytes per vertex); by default the regions follow one
    another at their capacities in a new buffer.  Returns (vertices, counts, offsets): the device buffer, int32 [n] on
    the device, and the regions' first vertices (host ints).  `pointcloud.cloud_arrays` brings them to the host."""
    backend = backend or default_backend()
    assert rays in ("pixel", "reference")
    pred = pred.detach()
    if pred.dim() == 4:
        assert pred.shape[1] == 1
        pred = pred[:, 0]
    pred = pred.contiguous().float()
    n, h, w = pred.shape
    stride = int(stride)
    if stride < 1:
        raise ValueError("point_cloud: stride must be at least 1, got %r" % (stride,))
    if (from_gt or mask_gt) and gt is None:
        raise ValueError("point_cloud: from_gt and mask_gt read the ground truth, which was not given")
    desc8 = np.asarray(rows_desc, dtype=np.int64).reshape(-1, _lib.EVAL_DESC)
    assert desc8.shape[0] == n and n > 0
    dev = pred.device
    caps = [cloud_capacity(r, stride) for r in desc8]
    if regions is None:
        assert out is None
        regions = [0] * n
        for i in range(1, n):
            regions[i] = regions[i - 1] + caps[i - 1]
        out = torch.empty((regions[-1] + caps[-1]) * _lib.CLOUD_VERTEX, dtype=torch.uint8, device=dev)
    regions = [int(r) for r in regions]
    assert out is not None and out.dtype == torch.uint8 and out.dim() == 1 and out.is_contiguous()
    assert len(regions) == n and all(r >= 0 and (r + c) * _lib.CLOUD_VERTEX <= out.numel() for r, c in zip(regions, caps))
    table = np.zeros((n, _lib.CLOUD_DESC), dtype=np.int32)
    table[:, :_lib.EVAL_DESC] = desc8
    table[:, _lib.EVAL_DESC:] = [split64(r) for r in regions]
    iK = torch.as_tensor(np.asarray(inv_K, dtype=np.float32))
    iK = iK[..., :3, :3].expand(n, 3, 3) if iK.dim() == 2 else iK[:, :3, :3]
    assert tuple(iK.shape) == (n, 3, 3)
    iK = upload(iK.contiguous(), dev)
    if rows is not None:
        assert rows.dtype == torch.float32 and tuple(rows.shape) == (n, _lib.EVAL_OUT) and rows.is_contiguous()
    if rgb is not None:
        assert rgb.dtype == torch.uint8 and rgb.dim() == 1 and rgb.is_contiguous()
    if gt is not None:
        assert gt.dtype == torch.float32 and gt.dim() == 1 and gt.is_contiguous()
    backend._check(pred, gt, rows, rgb, out)
    max_h, max_w = int(desc8[:, 2].max()), int(desc8[:, 3].max())
    n_ints = backend.lib.point_cloud_scratch_ints(n, max_h, max_w, stride)
    if n_ints < 0:
        raise _lib.BbdError("point_cloud: %d images of up to %d x %d pixels are more than one call holds; split the batch"
                            % (n, max_h, max_w))
    desc = upload(table, dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    scratch = torch.empty(n_ints, dtype=torch.int32, device=dev)
    flags = (_lib.EVAL_PRED_IS_DISP if pred_is_disp else 0) | (_lib.CLOUD_FROM_GT if from_gt else 0) | \
            (_lib.CLOUD_CLAMP if clamp_depth else 0) | (_lib.CLOUD_MASK_GT if mask_gt else 0) | \
            (_lib.CLOUD_RAYS_REFERENCE if rays == "reference" else 0)
    backend.run("bbd_point_cloud", pred, ptr(pred), ptr(gt), ptr(desc), ptr(rows), ptr(iK), ptr(rgb),
                ptr(magma_lut(dev)), ptr(out), ptr(counts), ptr(scratch), n_ints, n, h, w, max_h, max_w, stride,
                float(min_depth), float(max_depth), float(clamp[0]), float(clamp[1]), float(scale_factor), flags)
    return out, counts, regions


# ---------------------------------------------------------------------------- metric scale from the ground plane
def ground_scale(pred, inv_K, camera_height=1.65, angle_deg=5.0, pred_is_disp=False, min_count=64, want_mask=False,
                 backend=None):
    """The factor that brings every map of `pred` ([n,1,h,w] or [n,h,w], depth or - `pred_is_disp` - disparity of unknown
    scale) to metres, from the height of the camera above the road, in ONE `bbd_ground_scale` call (two launches, nothing
    read back).  Pixels are back-projected through `inv_K` ([3,3], [4,4] or one per image, on the host or the device;
    for pixels of the h x w map itself: `pointcloud.intrinsics_at`); those whose surface normal lies within `angle_deg`
    of the camera's down axis and that lie below the camera are ground, and the scale is `camera_height` over the median
    distance of their tangent planes from the camera.

    Returns (rows, mask): rows float32 [n, EVAL_OUT] on the device - [0] that median, [1] the number of ground pixels,
    [2] the number of candidates (interior pixels with nine valid depths), [7] the scale, in the slot `point_cloud`
    reads as `rows[i][7]`; [0] and [7] are NaN for an image with fewer than max(min_count, 1) ground pixels - and, with
    `want_mask`, uint8 [n,h,w] (1 = ground), else None."""
    import math
    backend = backend or default_backend()
    pred = pred.detach()
    if pred.dim() == 4:
        assert pred.shape[1] == 1
        pred = pred[:, 0]
    assert pred.dim() == 3 and pred.shape[0] > 0
    pred = pred.contiguous().float()
    n, h, w = pred.shape
    dev = pred.device
    if torch.is_tensor(inv_K):
        iK = inv_K.detach().to(torch.float32)
    else:
        iK = torch.as_tensor(np.asarray(inv_K, dtype=np.float32))
    iK = iK[..., :3, :3].expand(n, 3, 3) if iK.dim() == 2 else iK[:, :3, :3]
    assert tuple(iK.shape) == (n, 3, 3)
    iK = iK.contiguous() if iK.device == dev else upload(iK.contiguous(), dev)
    n_floats = backend.lib.ground_scale_scratch_floats(n, h, w)
    if n_floats < 0:
        raise _lib.BbdError("ground_scale: %d maps of %d x %d pixels are more than one call holds; split the batch"
                            % (n, h, w))
    backend._check(pred, iK)
    rows = torch.empty(n, _lib.EVAL_OUT, dtype=torch.float32, device=dev)
    mask = torch.empty(n, h, w, dtype=torch.uint8, device=dev) if want_mask else None
    scratch = torch.empty(n_floats, dtype=torch.float32, device=dev)
    backend.run("bbd_ground_scale", pred, ptr(pred), ptr(iK), ptr(rows), ptr(mask), ptr(scratch), n, h, w,
                float(camera_height), math.cos(math.radians(float(angle_deg))), int(min_count),
                _lib.EVAL_PRED_IS_DISP if pred_is_disp else 0)
    return rows, mask


# ---------------------------------------------------------------------------- scene map (voxel fusion)
MapState = collections.namedtuple("MapState", "keys pos col counters T")
MapState.__doc__ = """The caller-owned state of the `bbd_map_*` entries for a table of T slots: `keys` int64 [T] (the
uint64 voxel keys, empty = -1), `pos` int64 [T,3], `col` int32 [T,4] (sum r, g, b, count), `counters` int64 [4]
(candidates, kept, out-of-range drops, table-full drops)."""


def map_state(capacity, device, backend=None):
    """A cleared `MapState` of `capacity` slots rounded up to a power of two."""
    backend = backend or default_backend()
    capacity = int(capacity)
    if capacity < 1 or capacity > _lib.MAP_MAX_T:
        raise ValueError("map_state: the capacity must lie in [1, 2^30] slots, got %d" % capacity)
    T = 1 << (capacity - 1).bit_length()
    assert backend.lib.map_state_bytes(T) == T * _lib.MAP_SLOT_BYTES + 8 * _lib.MAP_COUNTERS
    state = MapState(torch.empty(T, dtype=torch.int64, device=device), torch.empty(T, 3, dtype=torch.int64, device=device),
                     torch.empty(T, 4, dtype=torch.int32, device=device),
                     torch.empty(_lib.MAP_COUNTERS, dtype=torch.int64, device=device), T)
    map_clear(state, backend)
    return state


def _map_state_ptrs(state, backend):
    keys, pos, col, counters, T = state
    assert keys.dtype == torch.int64 and pos.dtype == torch.int64 and col.dtype == torch.int32
    assert counters.dtype == torch.int64 and counters.numel() == _lib.MAP_COUNTERS
    assert keys.numel() == T and pos.numel() == 3 * T and col.numel() == 4 * T
    backend._check(keys, pos, col, counters)
    return ptr(keys), ptr(pos), ptr(col), ptr(counters), int(T)


def map_clear(state, backend=None):
    """`bbd_map_clear`: every slot empty, sums and counters zero (one launch)."""
    backend = backend or default_backend()
    backend.run("bbd_map_clear", state.keys, *_map_state_ptrs(state, backend))


def map_accumulate(state, disp, rgb, poses, inv_K, scale=None, stride=1, window=None, min_depth=0.5, max_depth=30.0,
                   voxel=0.2, is_depth=False, merge=True, backend=None):
    """`bbd_map_accumulate` (one launch, nothing read back): the points of n frames go into the voxel table.  `disp`
    float32 [n,h,w] or [n,1,h,w], the scaled disparity (or, `is_depth`, depth); `rgb` float32 [n,3,h,w] in [0,1];
    `poses` float64 [n,4,4] or [n,16] camera to world; `inv_K` float32 [3,3] (host or device); `scale` None or a
    float64 DEVICE tensor of one element that multiplies depths and points (`PoseTrajectory.summary[6:7]`);
    `window` = (r0, r1, c0, c1), default the whole image; every `stride`-th pixel of it is a candidate; the depth
    limits are in world units.  `merge=False` selects the form that adds every point for itself (BBD_MAP_NO_MERGE: the
    same state byte for byte, kept for measurements and tests)."""
    backend = backend or default_backend()
    disp = disp.detach()
    if disp.dim() == 4:
        assert disp.shape[1] == 1
        disp = disp[:, 0]
    if disp.dim() != 3 or disp.dtype != torch.float32:
        raise ValueError("map_accumulate: disp must be float32 [n,h,w] or [n,1,h,w], got %s %s"
                         % (disp.dtype, tuple(disp.shape)))
    n, h, w = disp.shape
    rgb, poses = rgb.detach(), poses.detach()
    if rgb.dtype != torch.float32 or tuple(rgb.shape) != (n, 3, h, w):
        raise ValueError("map_accumulate: rgb must be float32 [%d,3,%d,%d], got %s %s"
                         % (n, h, w, rgb.dtype, tuple(rgb.shape)))
    if poses.dtype != torch.float64 or poses.numel() != 16 * n or poses.shape[0] != n:
        raise ValueError("map_accumulate: poses must be float64 [%d,4,4], got %s %s" % (n, poses.dtype, tuple(poses.shape)))
    stride = int(stride)
    if n < 1 or stride < 1:
        raise ValueError("map_accumulate: at least one frame and a stride of at least 1 are needed")
    if not (float(voxel) > 0.0 and np.isfinite(float(voxel))):
        raise ValueError("map_accumulate: the voxel size must be positive and finite, got %r" % (voxel,))
    if not float(min_depth) <= float(max_depth):
        raise ValueError("map_accumulate: min_depth %r exceeds max_depth %r" % (min_depth, max_depth))
    r0, r1, c0, c1 = (0, h, 0, w) if window is None else (int(v) for v in window)
    dev = disp.device
    disp, rgb, poses = disp.contiguous(), rgb.contiguous(), poses.contiguous()
    iK = inv_K if torch.is_tensor(inv_K) else torch.as_tensor(np.asarray(inv_K, dtype=np.float32))
    assert iK.dtype == torch.float32 and tuple(iK.shape) == (3, 3)
    iK = upload(iK.contiguous(), dev) if iK.device != dev else iK.contiguous()
    if scale is not None:
        assert scale.dtype == torch.float64 and scale.numel() == 1 and scale.device == dev
    backend._check(disp, rgb, poses, iK, scale)
    sp = _map_state_ptrs(state, backend)
    # `scale` may be a view into a larger tensor: its address is taken as it is
    backend.run("bbd_map_accumulate", disp, *sp, ptr(disp), ptr(rgb), ptr(poses), ptr(iK),
                ctypes.c_void_p(0 if scale is None else scale.data_ptr()), n, h, w, r0, r1, c0, c1, stride,
                float(min_depth), float(max_depth), float(voxel),
                (_lib.MAP_INPUT_IS_DEPTH if is_depth else 0) | (0 if merge else _lib.MAP_NO_MERGE))


def map_finish(state, voxel, min_points=1, backend=None):
    """`bbd_map_finish` (three launches, nothing read back): the occupied slots with at least `min_points` points, in
    slot order.  Returns (out_keys int64 [T], vertices uint8 [16 T], out_counts int32 [T], m int32 [1]) on the device;
    the first m records are written.  The state is only read."""
    backend = backend or default_backend()
    min_points = int(min_points)
    if min_points < 1:
        raise ValueError("map_finish: min_points must be at least 1, got %d" % min_points)
    keys_p, pos_p, col_p, _, T = _map_state_ptrs(state, backend)
    dev = state.keys.device
    n_ints = backend.lib.map_finish_scratch_ints(T)
    assert n_ints >= 1
    out_keys = torch.empty(T, dtype=torch.int64, device=dev)
    vertices = torch.empty(T * _lib.CLOUD_VERTEX, dtype=torch.uint8, device=dev)
    out_counts = torch.empty(T, dtype=torch.int32, device=dev)
    m = torch.empty(1, dtype=torch.int32, device=dev)
    scratch = torch.empty(n_ints, dtype=torch.int32, device=dev)
    backend.run("bbd_map_finish", state.keys, keys_p, pos_p, col_p, T, min_points, float(voxel), ptr(out_keys),
                ptr(vertices), ptr(out_counts), ptr(m), ptr(scratch), n_ints)
    return out_keys, vertices, out_counts, m


# ---------------------------------------------------------------------------- depth-pose geometric consistency
Consistency = collections.namedtuple("Consistency", "filtered seen agree err counters transforms")
Consistency.__doc__ = """What `depth_consistency` leaves on the device: `filtered` float32 [n,h,w] or None, `seen` and
`agree` uint8 [n,h,w], `err` float32 [n,h,w] or None, `counters` int64 [n,5] (valid pixels, visible samples, agreeing
samples, the sum of err in units of 2^-24, pixels kept), `transforms` float64 [n,V,12]."""


def _matrix33(m, what, dev):
    m = m if torch.is_tensor(m) else torch.as_tensor(np.asarray(m, dtype=np.float32))
    if m.dtype != torch.float32 or tuple(m.shape) != (3, 3):
        raise ValueError("depth_consistency: %s must be float32 [3,3], got %s %s" % (what, m.dtype, tuple(m.shape)))
    return upload(m.contiguous(), dev) if m.device != dev else m.contiguous()


def depth_consistency(disp, poses, K, inv_K, sources, scale=None, threshold=0.05, min_views=1, is_depth=False,
                      want_err=False, want_filtered=True, backend=None):
    """`bbd_depth_consistency` (two launches, nothing read back): every pixel of every frame is back-projected with its
    depth, moved into each of its source frames with the relative pose and compared with the depth that frame predicts
    there, err = |z - d_b| / (z + d_b).  `disp` float32 [n,h,w] or [n,1,h,w], the scaled disparity (or,
    `is_depth`, depth); `poses` float64 [n,4,4] or [n,16] camera to world; `K`, `inv_K` float32 [3,3] of the h x w map
    (host or device); `sources` int32 [n,V] (host or device; `pointcloud.neighbour_sources`), -1 = none; `scale` None or
    a float64 DEVICE tensor of one element, as `map_accumulate` takes it.  A pixel is kept in `filtered` when it is valid
    and agrees (err < `threshold`, strict) in at least `min_views` sources.  Returns a `Consistency`."""
    backend = backend or default_backend()
    disp = disp.detach()
    if disp.dim() == 4:
        assert disp.shape[1] == 1
        disp = disp[:, 0]
    if disp.dim() != 3 or disp.dtype != torch.float32:
        raise ValueError("depth_consistency: disp must be float32 [n,h,w] or [n,1,h,w], got %s %s"
                         % (disp.dtype, tuple(disp.shape)))
    n, h, w = disp.shape
    poses = poses.detach()
    if n < 1:
        raise ValueError("depth_consistency: at least one frame is needed")
    if poses.dtype != torch.float64 or poses.numel() != 16 * n or poses.shape[0] != n:
        raise ValueError("depth_consistency: poses must be float64 [%d,4,4], got %s %s"
                         % (n, poses.dtype, tuple(poses.shape)))
    sources = sources if torch.is_tensor(sources) else torch.as_tensor(np.asarray(sources))
    if sources.dtype != torch.int32 or sources.dim() != 2 or sources.shape[0] != n \
            or not 1 <= sources.shape[1] <= _lib.CONSIST_MAX_VIEWS:
        raise ValueError("depth_consistency: sources must be int32 [%d,V] with 1 <= V <= %d, got %s %s"
                         % (n, _lib.CONSIST_MAX_VIEWS, sources.dtype, tuple(sources.shape)))
    V = int(sources.shape[1])
    threshold, min_views = float(threshold), int(min_views)
    if not threshold >= 0.0:
        raise ValueError("depth_consistency: the threshold must not be negative, got %r" % (threshold,))
    if min_views < 0:
        raise ValueError("depth_consistency: min_views must not be negative, got %d" % min_views)
    if n * h * w > 0x7fffffff:
        raise ValueError("depth_consistency: %d frames of %d x %d pixels are more than one call holds; split the batch"
                         % (n, h, w))
    dev = disp.device
    disp, poses = disp.contiguous(), poses.contiguous()
    K3, iK = _matrix33(K, "K", dev), _matrix33(inv_K, "inv_K", dev)
    sources = upload(sources.contiguous(), dev) if sources.device != dev else sources.contiguous()
    if scale is not None:
        assert scale.dtype == torch.float64 and scale.numel() == 1 and scale.device == dev
    backend._check(disp, poses, K3, iK, sources, scale)
    transforms = torch.empty(n, V, 12, dtype=torch.float64, device=dev)
    seen = torch.empty(n, h, w, dtype=torch.uint8, device=dev)
    agree = torch.empty(n, h, w, dtype=torch.uint8, device=dev)
    err = torch.empty(n, h, w, dtype=torch.float32, device=dev) if want_err else None
    filtered = torch.empty(n, h, w, dtype=torch.float32, device=dev) if want_filtered else None
    counters = torch.empty(n, _lib.CONSIST_COUNTERS, dtype=torch.int64, device=dev)
    # `scale` may be a view into a larger tensor: its address is taken as it is
    backend.run("bbd_depth_consistency", disp, ptr(disp), ptr(poses),
                ctypes.c_void_p(0 if scale is None else scale.data_ptr()), ptr(K3), ptr(iK), ptr(sources), ptr(transforms),
                ptr(seen), ptr(agree), ptr(err), ptr(filtered), ptr(counters), n, h, w, V, threshold, min_views,
                _lib.CONSIST_INPUT_IS_DEPTH if is_depth else 0)
    return Consistency(filtered, seen, agree, err, counters, transforms)


# ---------------------------------------------------------------------------- geometry-consistency loss (training)
GeometryConsistency = collections.namedtuple("GeometryConsistency", "loss pair_sum pair_count err code")
GeometryConsistency.__doc__ = """What `geometry_consistency` leaves on the device: `loss` float64 scalar (differentiable),
`pair_sum` float64 [V,B] (differentiable), `pair_count` int64 [V,B], `err` float32 [V,B,H,W] or None (0 where the sample
is not visible), `code` uint8 [V,B,H,W] or None (bit 0 = visible, bit 1 = z s > 1)."""


def geo_scratch_words(B, H, W, V, backward):
    """8-byte words of scratch of bbd_geo_fwd / bbd_geo_bwd: the formulas of include/bbd_hip.h."""
    items = (H * W + _lib.GEO_RUN - 1) // _lib.GEO_RUN
    return V * B * H * W + B * items * V * 12 if backward else B * items * V * 2


class _GeometryConsistency(torch.autograd.Function):
    """pair_sum [V,B] of bbd_geo_fwd; bbd_geo_bwd gives the gradients to q_tgt, q_src and T from the upstream gradient
    on the device.  Nothing is read back either way."""

    @staticmethod
    def forward(ctx, q_tgt, q_src, T, K, inv_K, want_err, want_code, backend):
        V, B, H, W = q_src.shape
        dev = q_tgt.device
        pair_sum = torch.empty(V, B, dtype=torch.float64, device=dev)
        pair_count = torch.empty(V, B, dtype=torch.int64, device=dev)
        err = torch.empty(V, B, H, W, dtype=torch.float32, device=dev) if want_err else None
        code = torch.empty(V, B, H, W, dtype=torch.uint8, device=dev) if want_code else None
        words = geo_scratch_words(B, H, W, V, False)
        scratch = torch.empty(words, dtype=torch.int64, device=dev)
        backend.run("bbd_geo_fwd", q_tgt, ptr(q_tgt), ptr(q_src), ptr(T), ptr(K), ptr(inv_K), ptr(pair_sum),
                    ptr(pair_count), ptr(err), ptr(code), ptr(scratch), words, B, H, W, V)
        ctx.save_for_backward(q_tgt, q_src, T, K, inv_K)
        ctx.backend = backend
        outs = [t for t in (pair_count, err, code) if t is not None]
        ctx.mark_non_differentiable(*outs)
        return pair_sum, pair_count, err, code

    @staticmethod
    def backward(ctx, g_sum, *_unused):
        q_tgt, q_src, T, K, inv_K = ctx.saved_tensors
        V, B, H, W = q_src.shape
        g = g_sum.to(torch.float64).contiguous()
        grad_t, grad_s, grad_T = torch.empty_like(q_tgt), torch.empty_like(q_src), torch.empty_like(T)
        words = geo_scratch_words(B, H, W, V, True)
        scratch = torch.empty(words, dtype=torch.int64, device=q_tgt.device)
        ctx.backend.run("bbd_geo_bwd", q_tgt, ptr(q_tgt), ptr(q_src), ptr(T), ptr(K), ptr(inv_K), ptr(g), ptr(grad_t),
                        ptr(grad_s), ptr(grad_T), ptr(scratch), words, B, H, W, V)
        return grad_t, grad_s, grad_T, None, None, None, None, None


def geometry_consistency(q_tgt, q_src, T, K, inv_K, want_err=False, want_code=False, backend=None):
    """The geometry-consistency loss of SC-SfMLearner (Bian et al., NeurIPS 2019) between B target frames
    and V source frames each: a target pixel is back-projected with its inverse depth `q_tgt` float32 [B,H,W], moved with
    `T` float32 [V,B,12] (rows 0..2 of the target-to-source matrix; [V,B,3,4] is taken too) and compared with the
    bilinear sample s of `q_src` float32 [V,B,H,W] there: e = |z s - 1| / (z s + 1), the err `depth_consistency` scores.
    `K`, `inv_K` float32 [B,16] or [B,4,4], not differentiable.  Returns a `GeometryConsistency`; `loss` is the mean of e
    over the visible samples (0 where there is none), formed on the device: no host synchronisation, capturable.
    Gradients reach q_tgt, q_src and T; identical calls give identical bytes."""
    backend = backend or default_backend()
    who = "geometry_consistency: "
    if not torch.is_tensor(q_tgt) or q_tgt.dtype != torch.float32 or q_tgt.dim() != 3:
        raise ValueError(who + "q_tgt must be float32 [B,H,W], got %s %s"
                         % (getattr(q_tgt, "dtype", type(q_tgt)), tuple(getattr(q_tgt, "shape", ()))))
    B, H, W = q_tgt.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError(who + "q_tgt must not be empty, got %s" % (tuple(q_tgt.shape),))
    if not torch.is_tensor(q_src) or q_src.dtype != torch.float32 or q_src.dim() != 4 \
            or tuple(q_src.shape[1:]) != (B, H, W) or not 1 <= q_src.shape[0] <= _lib.GEO_MAX_VIEWS:
        raise ValueError(who + "q_src must be float32 [V,%d,%d,%d] with 1 <= V <= %d, got %s %s"
                         % (B, H, W, _lib.GEO_MAX_VIEWS, getattr(q_src, "dtype", type(q_src)),
                            tuple(getattr(q_src, "shape", ()))))
    V = int(q_src.shape[0])
    if not torch.is_tensor(T) or T.dtype != torch.float32 or tuple(T.shape) not in ((V, B, 12), (V, B, 3, 4)):
        raise ValueError(who + "T must be float32 [%d,%d,12] or [%d,%d,3,4], got %s %s"
                         % (V, B, V, B, getattr(T, "dtype", type(T)), tuple(getattr(T, "shape", ()))))
    mats = []
    for m, what in ((K, "K"), (inv_K, "inv_K")):
        if not torch.is_tensor(m) or m.dtype != torch.float32 or tuple(m.shape) not in ((B, 16), (B, 4, 4)):
            raise ValueError(who + "%s must be float32 [%d,16] or [%d,4,4], got %s %s"
                             % (what, B, B, getattr(m, "dtype", type(m)), tuple(getattr(m, "shape", ()))))
        mats.append(m.detach().reshape(B, 16).contiguous())
    for t, what in ((q_src, "q_src"), (T, "T"), (mats[0], "K"), (mats[1], "inv_K")):
        if t.device != q_tgt.device:
            raise ValueError(who + "%s is on %s, q_tgt on %s" % (what, t.device, q_tgt.device))
    if H * W > 1 << 23 or V * B * H * W > 0x7fffffff:
        raise ValueError(who + "%d x %d pairs of %d x %d pixels are more than one call holds" % (V, B, H, W))
    backend._check(q_tgt, q_src, T, *mats)
    pair_sum, pair_count, err, code = _GeometryConsistency.apply(
        q_tgt.contiguous(), q_src.contiguous(), T.reshape(V, B, 12).contiguous(), mats[0], mats[1], bool(want_err),
        bool(want_code), backend)
    loss = pair_sum.sum() / pair_count.sum().clamp(min=1)
    return GeometryConsistency(loss, pair_sum, pair_count, err, code)


# ---------------------------------------------------------------------------- depth hints (semi-global stereo matching)
def sgm_scratch_bytes(B, H, W, D=128, paths=8):
    """Bytes of scratch of bbd_sgm_hints: the formula of include/bbd_sgm.h (`lib.sgm_scratch_bytes`)."""
    P = B * H * W
    return (2 * P + 7) // 8 * 8 + 16 * P + 3 * P * D + (4 * P + 7) // 8 * 8


def stereo_hints(left, right, side, disparities=128, paths=8, p1=_lib.SGM_P1, p2=_lib.SGM_P2,
                 uniqueness=_lib.SGM_UNIQUENESS, fill=False, scratch=None, backend=None):
    """Semi-global stereo matching of a rectified pair on the device (bbd_sgm_hints): `left`, `right`
    float32 [B,3,H,W] in [0,1] (the frame and its stereo partner), `side` int32 [B] (0 = the partner lies to the right,
    matches at x - d: `stereo_T[b,0,3] < 0`; otherwise mirrored, matches at x + d).  `disparities` 64, 128, 192 or 256,
    `paths` 4 or 8, penalties 1 <= p1 < p2 <= 8129, `uniqueness` OpenCV's ratio in percent (0 = off), `fill` spreads the
    nearest valid value along each row.  `scratch`: a uint8 tensor of at least `sgm_scratch_bytes(...)` bytes that the
    caller keeps (allocated here when None).  Returns (disp16 int16 [B,H,W]: 16 x disparity, -16 = invalid; valid_count
    int64 [B]).  Integer arithmetic: identical calls give identical bytes.  No host synchronisation, capturable."""
    backend = backend or default_backend()
    who = "stereo_hints: "
    if not torch.is_tensor(left) or left.dtype != torch.float32 or left.dim() != 4 or left.shape[1] != 3 or left.numel() == 0:
        raise ValueError(who + "left must be a non-empty float32 [B,3,H,W], got %s %s"
                         % (getattr(left, "dtype", type(left)), tuple(getattr(left, "shape", ()))))
    B, _, H, W = left.shape
    if not torch.is_tensor(right) or right.dtype != torch.float32 or right.shape != left.shape:
        raise ValueError(who + "right must be float32 %s like left, got %s %s"
                         % (tuple(left.shape), getattr(right, "dtype", type(right)), tuple(getattr(right, "shape", ()))))
    if not torch.is_tensor(side) or side.dtype != torch.int32 or tuple(side.shape) != (B,):
        raise ValueError(who + "side must be int32 [%d], got %s %s"
                         % (B, getattr(side, "dtype", type(side)), tuple(getattr(side, "shape", ()))))
    D, paths, p1, p2, uniqueness = int(disparities), int(paths), int(p1), int(p2), int(uniqueness)
    if D not in (64, 128, 192, 256) or paths not in (4, 8):
        raise ValueError(who + "disparities must be 64, 128, 192 or 256 and paths 4 or 8, got %d and %d" % (D, paths))
    if not 1 <= p1 < p2 <= _lib.SGM_MAX_P2:
        raise ValueError(who + "the penalties must satisfy 1 <= p1 < p2 <= %d (8 paths of 62 + p2 must fit 16 bits), got "
                         "%d and %d" % (_lib.SGM_MAX_P2, p1, p2))
    if not 0 <= uniqueness <= 99:
        raise ValueError(who + "uniqueness is a percentage in 0 .. 99, got %d" % uniqueness)
    if B > 65535 or B * H * W > 1 << 26:
        raise ValueError(who + "%d images of %d x %d pixels are more than one call holds" % (B, H, W))
    need = sgm_scratch_bytes(B, H, W, D, paths)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=left.device)
    elif not torch.is_tensor(scratch) or scratch.dtype != torch.uint8 or scratch.dim() != 1 or scratch.numel() < need \
            or not scratch.is_contiguous() or scratch.data_ptr() % 8:
        raise ValueError(who + "scratch must be a contiguous, 8-byte aligned uint8 tensor of at least %d bytes" % need)
    for t, what in ((right, "right"), (side, "side"), (scratch, "scratch")):
        if t.device != left.device:
            raise ValueError(who + "%s is on %s, left on %s" % (what, t.device, left.device))
    left, right, side = left.detach().contiguous(), right.detach().contiguous(), side.contiguous()
    backend._check(left, right, side, scratch)
    disp16 = torch.empty(B, H, W, dtype=torch.int16, device=left.device)
    valid_count = torch.empty(B, dtype=torch.int64, device=left.device)
    backend.run("bbd_sgm_hints", left, ptr(left), ptr(right), ptr(side), ptr(disp16), ptr(valid_count), ptr(scratch),
                scratch.numel(), B, H, W, D, paths, p1, p2, uniqueness, int(bool(fill)))
    return disp16, valid_count


def hint_depth(disp16, K, stereo_T):
    """`stereo_hints` disparities -> (depth float32 [B,H,W], valid bool [B,H,W]) in the units of the depth network's
    `disp_to_depth` output: depth = fx * |t_x| / (disp16 / 16) with fx = K[b,0,0] in pixels and t_x = stereo_T[b,0,3] (0.1
    for every KITTI pair of the loader).  A pixel is valid where disp16 > 0 (an invalid pixel is -16, and a disparity of
    0 has no finite depth); the depth is 0 where it is not.  Plain torch, not a hot path."""
    if disp16.dtype != torch.int16 or disp16.dim() != 3:
        raise ValueError("hint_depth: disp16 must be int16 [B,H,W], got %s %s" % (disp16.dtype, tuple(disp16.shape)))
    B = disp16.shape[0]
    scale = (K.reshape(B, -1)[:, 0] * stereo_T.reshape(B, 16)[:, 3].abs()).to(torch.float32).view(B, 1, 1)
    valid = disp16 > 0
    d = disp16.to(torch.float32) / 16.0
    return torch.where(valid, scale / torch.where(valid, d, torch.ones_like(d)), torch.zeros_like(d)), valid


# ---------------------------------------------------------------------------- views (rasterised points and polylines)
ViewState = collections.namedtuple("ViewState", "cells counters H W")
ViewState.__doc__ = """The caller-owned canvas of the `bbd_view_*` entries: `cells` int64 [H,W] (the uint64 keys, empty =
-1), `counters` int64 [4] (offered, drawn, clipped, rejected points)."""


def pack_rgb(colour, what):
    """(r, g, b) bytes -> r | g << 8 | b << 16."""
    c = [int(v) for v in colour]
    if len(c) != 3 or min(c) < 0 or max(c) > 255:
        raise ValueError("%s: a colour is three bytes, got %r" % (what, colour))
    return c[0] | (c[1] << 8) | (c[2] << 16)


def view_state(height, width, device, backend=None):
    """A cleared `ViewState` of height x width cells."""
    H, W = int(height), int(width)
    if H < 1 or W < 1 or H * W > _lib.VIEW_MAX_CELLS:
        raise ValueError("view_state: a canvas has at least 1 x 1 and at most 2^28 cells, got %d x %d" % (H, W))
    state = ViewState(torch.empty(H, W, dtype=torch.int64, device=device),
                      torch.empty(_lib.VIEW_COUNTERS, dtype=torch.int64, device=device), H, W)
    view_clear(state, backend)
    return state


def _view_state_args(state, backend):
    cells, counters, H, W = state
    assert cells.dtype == torch.int64 and tuple(cells.shape) == (H, W) and cells.is_contiguous()
    assert counters.dtype == torch.int64 and counters.numel() == _lib.VIEW_COUNTERS
    backend._check(cells, counters)
    return ptr(cells), ptr(counters), int(H), int(W)


def _view_matrix(view, device, what):
    """The float64 [4,4] view on `device`: a device tensor is taken as it is, a host array is uploaded."""
    if not torch.is_tensor(view):
        view = torch.as_tensor(np.ascontiguousarray(view, dtype=np.float64))
    if view.dtype != torch.float64 or view.numel() != 16 or tuple(view.shape) not in ((4, 4), (16,)):
        raise ValueError("%s: view must be float64 [4,4], got %s %s" % (what, view.dtype, tuple(view.shape)))
    return view.contiguous() if view.device == device else upload(view.contiguous(), device)


def view_clear(state, backend=None):
    """`bbd_view_clear`: every cell empty, the counters zero (one launch)."""
    backend = backend or default_backend()
    backend.run("bbd_view_clear", state.cells, *_view_state_args(state, backend))


def view_points(state, vertices, view, count=None, size=1, backend=None):
    """`bbd_view_points` (one launch, nothing read back): the 16-byte vertex records of `vertices` (uint8 [16 n], as
    `point_cloud` and `map_finish` leave them) go into the canvas through `view` (float64 [4,4], host or device).
    `count`: None, or an int32 DEVICE tensor of one element - only the first min(count, n) records are read."""
    backend = backend or default_backend()
    if vertices.dtype != torch.uint8 or vertices.dim() != 1 or vertices.numel() % _lib.CLOUD_VERTEX:
        raise ValueError("view_points: vertices must be uint8 [16 n], got %s %s" % (vertices.dtype, tuple(vertices.shape)))
    if int(size) not in (1, 3, 5, 7):
        raise ValueError("view_points: size must be 1, 3, 5 or 7, got %r" % (size,))
    dev = state.cells.device
    if vertices.device != dev or (count is not None and count.device != dev):
        raise ValueError("view_points: vertices and count must be on the canvas's device %s" % dev)
    if count is not None and (count.dtype != torch.int32 or count.numel() != 1):
        raise ValueError("view_points: count must be one int32, got %s %s" % (count.dtype, tuple(count.shape)))
    vertices = vertices.contiguous()
    if vertices.data_ptr() % _lib.CLOUD_VERTEX:
        raise ValueError("view_points: vertices must be 16-byte aligned")
    V = _view_matrix(view, dev, "view_points")
    backend._check(vertices, count, V)
    n = vertices.numel() // _lib.CLOUD_VERTEX
    # `count` may be a view into a larger tensor: its address is taken as it is
    backend.run("bbd_view_points", vertices, *_view_state_args(state, backend), ptr(vertices),
                ctypes.c_void_p(0 if count is None else count.data_ptr()), n, ptr(V), int(size))


def view_lines(state, xyz, view, colour=(0, 0, 0), width=2.0, layer=0, closed=False, backend=None):
    """`bbd_view_lines` (one launch, nothing read back): the polyline through `xyz` (float64 [P,3] world positions, host
    or device) as an overlay of `colour` on `layer` (0 .. 65535; a higher layer covers a lower one, every layer covers
    the points).  One position, or a segment without length, draws a disc of diameter `width` pixels."""
    backend = backend or default_backend()
    dev = state.cells.device
    if not torch.is_tensor(xyz):
        xyz = torch.as_tensor(np.ascontiguousarray(xyz, dtype=np.float64))
    if xyz.dtype != torch.float64 or xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] < 1:
        raise ValueError("view_lines: xyz must be float64 [P,3] with P >= 1, got %s %s" % (xyz.dtype, tuple(xyz.shape)))
    width, layer = float(width), int(layer)
    if not (width > 0.0 and np.isfinite(width)):
        raise ValueError("view_lines: the width must be positive and finite, got %r" % (width,))
    if not 0 <= layer <= _lib.VIEW_MAX_LAYER:
        raise ValueError("view_lines: the layer must lie in [0, %d], got %d" % (_lib.VIEW_MAX_LAYER, layer))
    rgb = pack_rgb(colour, "view_lines")
    xyz = xyz.contiguous() if xyz.device == dev else upload(xyz.contiguous(), dev)
    V = _view_matrix(view, dev, "view_lines")
    backend._check(xyz, V)
    backend.run("bbd_view_lines", xyz, *_view_state_args(state, backend), ptr(xyz), int(xyz.shape[0]), ptr(V), rgb,
                width, layer, 1 if closed else 0)


def view_resolve(state, background=(255, 255, 255), backend=None):
    """`bbd_view_resolve` (one launch): the canvas as uint8 [H,W,3] on the device, `background` where nothing was
    drawn.  The cells are only read."""
    backend = backend or default_backend()
    cells_p, _, H, W = _view_state_args(state, backend)
    out = torch.empty(H, W, 3, dtype=torch.uint8, device=state.cells.device)
    backend.run("bbd_view_resolve", state.cells, cells_p, H, W, pack_rgb(background, "view_resolve"), ptr(out))
    return out


# ---------------------------------------------------------------------------- flip post-processing
def post_process_disp(disp, backend=None):
    """Monodepth2's `batch_post_process_disparity(l, r[:, :, ::-1])` in ONE `bbd_post_process_disp` launch: `disp`
    [2n,1,h,w] or [2n,h,w] float32 holds the predictions for n images followed by the predictions for the same images
    flipped left-right (`torch.cat((x, torch.flip(x, [3])), 0)` through the networks), the second half still flipped.
    Returns the blended disparities, float32 [n,h,w]: the reference's float64 blend rounded once."""
    backend = backend or default_backend()
    disp = disp.detach()
    if disp.dim() == 4:
        assert disp.shape[1] == 1
        disp = disp[:, 0]
    if disp.dim() != 3:
        raise ValueError("post_process_disp: disp must be [2n,1,h,w] or [2n,h,w], got %s" % (tuple(disp.shape),))
    if disp.shape[0] < 2 or disp.shape[0] % 2:
        raise ValueError("post_process_disp: the leading dimension holds n predictions and their n flipped twins; "
                         "%d is not a positive even number" % disp.shape[0])
    disp = disp.contiguous().float()
    backend._check(disp)
    n, h, w = disp.shape[0] // 2, disp.shape[1], disp.shape[2]
    out = torch.empty(n, h, w, dtype=torch.float32, device=disp.device)
    backend.run("bbd_post_process_disp", disp, ptr(disp), ptr(out), n, h, w)
    return out


# ---------------------------------------------------------------------------- uncertainty of the flip pass, sparsification
def post_process_uncert(disp, backend=None):
    """`post_process_disp` and the disagreement it throws away, in ONE `bbd_post_process_uncert` launch: `disp` as that
    function takes it.  Returns (out, uncert), float32 [n,h,w] each: the bytes `post_process_disp` returns, and
    |disp[i] - flip(disp[n+i])|, the "Post" uncertainty of Poggi et al.."""
    backend = backend or default_backend()
    disp = disp.detach()
    if disp.dim() == 4:
        assert disp.shape[1] == 1
        disp = disp[:, 0]
    if disp.dim() != 3:
        raise ValueError("post_process_uncert: disp must be [2n,1,h,w] or [2n,h,w], got %s" % (tuple(disp.shape),))
    if disp.shape[0] < 2 or disp.shape[0] % 2:
        raise ValueError("post_process_uncert: the leading dimension holds n predictions and their n flipped twins; "
                         "%d is not a positive even number" % disp.shape[0])
    disp = disp.contiguous().float()
    backend._check(disp)
    n, h, w = disp.shape[0] // 2, disp.shape[1], disp.shape[2]
    out = torch.empty(n, h, w, dtype=torch.float32, device=disp.device)
    uncert = torch.empty(n, h, w, dtype=torch.float32, device=disp.device)
    backend.run("bbd_post_process_uncert", disp, ptr(disp), ptr(out), ptr(uncert), n, h, w)
    return out, uncert


def sparsification_scratch_bytes(desc_host, n):
    """Bytes of scratch `bbd_sparsification` needs for the `n` BBD_EVAL_DESC rows `desc_host` (a host array): the
    formula of include/bbd_hip.h over the areas of the crop windows cut to their maps."""
    d = np.asarray(desc_host).reshape(-1, _lib.EVAL_DESC).astype(np.int64)
    assert d.shape[0] == n
    rows = np.maximum(np.minimum(d[:, 5], d[:, 2]) - np.maximum(d[:, 4], 0), 0)
    cols = np.maximum(np.minimum(d[:, 7], d[:, 3]) - np.maximum(d[:, 6], 0), 0)
    return _lib.SPARS_SCRATCH_CALL + n * _lib.SPARS_SCRATCH_IMAGE + int((rows * cols).sum()) * _lib.SPARS_SCRATCH_PIXEL


def sparsification(pred_disp, uncert, gts, indices, rows, intervals=50, min_depth=1e-3, max_depth=80.0, scale_factor=1.0,
                   median_scaling=True, backend=None):
    """How good is an uncertainty map (Poggi et al., CVPR 2020)?  `pred_disp` ([n,1,h,w] or [n,h,w]) is the scaled
    disparity `evaluation.depth_metrics` was given with `pred_is_disp=True`, `rows` that call's output and `uncert`
    ([n,h,w]) the uncertainty of every disparity.  The pixels the metrics score are removed in order of falling
    uncertainty and the rest is re-scored at `intervals` fractions; the same with the three oracle orderings.  One
    `bbd_sparsification` call, no host synchronisation.  Returns float64 [n, 8 + 6 * (intervals + 1)] on the device:
    {AUSE abs_rel, rmse, a1, AURG abs_rel, rmse, a1, N, 0}, then the curves [sparse, oracle][abs_rel, rmse, a1]
    [intervals + 1].  An image without a scored pixel has a row of NaN with N = 0."""
    backend = backend or default_backend()
    if not 1 <= int(intervals) <= _lib.SPARS_MAX_INTERVALS:
        raise ValueError("sparsification: intervals must be 1 ... %d, got %r" % (_lib.SPARS_MAX_INTERVALS, intervals))
    pred = pred_disp.detach()
    if pred.dim() == 4:
        assert pred.shape[1] == 1
        pred = pred[:, 0]
    pred = pred.contiguous().float()
    uncert = uncert.detach()
    if uncert.dim() == 4:
        assert uncert.shape[1] == 1
        uncert = uncert[:, 0]
    uncert = uncert.contiguous().float()
    if pred.dim() != 3 or uncert.shape != pred.shape:
        raise ValueError("sparsification: pred_disp and uncert must both be [n,h,w], got %s and %s"
                         % (tuple(pred.shape), tuple(uncert.shape)))
    b = _GtBatch(gts, indices)
    n, h, w = pred.shape
    assert n == len(b.idx)
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (n, _lib.EVAL_OUT) and rows.is_contiguous()
    backend._check(pred, uncert, gts.buffer, rows)
    dev, K = pred.device, int(intervals)
    nbytes = sparsification_scratch_bytes(gts.desc_host[b.idx], n)
    scratch = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    out = torch.empty(n, _lib.SPARS_SUMMARY + 6 * (K + 1), dtype=torch.float64, device=dev)
    backend.run("bbd_sparsification", pred, ptr(pred), ptr(uncert), ptr(b.gt), ptr(b.desc), ptr(rows), ptr(out),
                ptr(scratch), nbytes, n, h, w, K, float(min_depth), float(max_depth), float(scale_factor),
                0 if median_scaling else _lib.EVAL_NO_MEDIAN_SCALING)
    return out


# ---------------------------------------------------------------------------- training-log panel
_PANEL_LUTS = {}


def panel_luts(device="cpu"):
    """uint8 [256 + 256 + 20, 3]: plasma, magma, the categorical palette (`tab20`) - the LUT buffer of `train_panel`.
    Read from the shipped tables (panel_luts.hex, written by tools/make_panel_luts.py, and magma_lut.hex); matplotlib is
    never imported."""
    key = str(device)
    if key not in _PANEL_LUTS:
        if "cpu" not in _PANEL_LUTS:
            own = _hex_lut("panel_luts.hex", 276)
            _PANEL_LUTS["cpu"] = torch.cat([own[:256], magma_lut("cpu"), own[256:]], 0).contiguous()
            assert _PANEL_LUTS["cpu"].shape[0] == _lib.PANEL_LUT_ROWS
        _PANEL_LUTS[key] = _PANEL_LUTS["cpu"].to(device)
    return _PANEL_LUTS[key]


def _addr_words(t):
    return split64(0 if t is None else t.data_ptr())


def train_panel(tiles, pose_table, H, W, rows, cols, backend=None):
    """A grid of `rows` x `cols` tiles of H x W pixels rendered on the device in ONE `bbd_train_panel` call (two
    launches, no host synchronisation) -> (panel uint8 [rows*H, cols*W, 3], stats fp32 [len(tiles), 2]).

    `tiles` is a list of `(row, col, kind, ...)`:
        (r, c, "color", image [3,H,W])                      fp32 in [0,1], rounded to nearest
        (r, c, "warp", source [3,H,W], depth [H,W], p)      the fused forward's warp with row p of `pose_table`
        (r, c, "scalar", plane [H,W], "plasma" | "magma")   colour-mapped between its minimum and maximum; stats[t]
        (r, c, "argmin", ids uint8 [H,W], n_T, n_E)         palette[id] | palette[id - n_T] >> 1 | black
    Cells no tile names are black.  `pose_table` is [NP,40] in the row layout of `pose_table_rows` (None where no tile
    warps)."""
    backend = backend or default_backend()
    if not tiles:
        raise ValueError("train_panel: no tiles")
    dev = tiles[0][3].device
    if pose_table is None:
        pose_table = torch.zeros(1, POSE_STRIDE, dtype=torch.float32, device=dev)
    pose_table = pose_table.detach()
    assert pose_table.dim() == 2 and pose_table.shape[1] == POSE_STRIDE and pose_table.dtype == torch.float32
    pose_table = pose_table.contiguous()
    kinds = {"color": _lib.PANEL_COLOR, "warp": _lib.PANEL_WARP, "scalar": _lib.PANEL_SCALAR, "argmin": _lib.PANEL_ARGMIN}
    desc, keep = [], [pose_table]
    for tile in tiles:
        r, c, kind = int(tile[0]), int(tile[1]), tile[2]
        if not (0 <= r < rows and 0 <= c < cols):
            raise ValueError("train_panel: cell (%d, %d) outside the %d x %d grid" % (r, c, rows, cols))
        src, aux, p0, p1 = tile[3].detach(), None, 0, 0
        if kind in ("color", "warp"):
            assert src.dtype == torch.float32 and tuple(src.shape) == (3, H, W), (kind, tuple(src.shape))
        if kind == "warp":
            aux, p0 = tile[4].detach(), int(tile[5])
            assert aux.dtype == torch.float32 and tuple(aux.shape) == (H, W)
            aux = aux.contiguous()
        elif kind == "scalar":
            assert src.dtype == torch.float32 and tuple(src.shape) == (H, W)
            p0 = {"plasma": 0, "magma": 1}[tile[4]]
        elif kind == "argmin":
            assert src.dtype == torch.uint8 and tuple(src.shape) == (H, W)
            p0, p1 = int(tile[4]), int(tile[5])
        elif kind != "color":
            raise ValueError("train_panel: unknown tile kind %r" % (kind,))
        src = src.contiguous()
        backend._check(src, aux)
        keep += [src, aux]
        desc.append((kinds[kind], r * cols + c) + _addr_words(src) + _addr_words(aux) + (p0, p1))
    backend._check(pose_table)
    n = len(desc)
    desc = upload(torch.tensor(desc, dtype=torch.int32), dev)
    out = torch.empty(rows * H, cols * W, 3, dtype=torch.uint8, device=dev)
    stats = torch.zeros(n, 2, dtype=torch.float32, device=dev)
    scratch = torch.empty(backend.lib.train_panel_scratch_ints(n), dtype=torch.int32, device=dev)
    backend.run("bbd_train_panel", out, ptr(desc), ptr(pose_table), ptr(panel_luts(dev)), ptr(out), ptr(stats), ptr(scratch),
                n, pose_table.shape[0], int(H), int(W), int(rows), int(cols))
    del keep                      # (held until here: a temporary's memory is reused at once, in stream order after the launch)
    return out, stats


def argmin_hist(argmin, backend=None):
    """int32 [B, MAX_CAND]: how many pixels of each sample every arg-min id won (`argmin` uint8 [B,H,W]); ids of
    MAX_CAND and above are not counted.  One `bbd_argmin_hist` call: integer atomics, exact."""
    backend = backend or default_backend()
    argmin = argmin.detach()
    assert argmin.dtype == torch.uint8 and argmin.dim() == 3
    argmin = argmin.contiguous()
    backend._check(argmin)
    B, n_px = argmin.shape[0], argmin.shape[1] * argmin.shape[2]
    counts = torch.empty(B, _lib.MAX_CAND, dtype=torch.int32, device=argmin.device)
    backend.run("bbd_argmin_hist", argmin, ptr(argmin), ptr(counts), B, n_px)
    return counts
