"""float64 reference of the geometry-consistency loss (`bbd_geo_fwd` / `bbd_geo_bwd`) and the scene of
its tests.  Test infrastructure only.

`geometry` restates the definition independently of csrc/bbd_geo_math.h: whole arrays, float64, gradients from torch
autograd.  It is compared with the float32 op within tolerances, not by bytes.  It also says where a sample lies close
to a kink of the loss - an integer coordinate (image edges are integers), or a = z s close to 1 - where a float32
evaluation may stand on the other side and its gradient may differ by a finite amount.

`scene` renders the street of tests/consist_ref.py for B target cameras with V sources each."""
import numpy as np
import torch

import consist_ref

MIN_Z = float(np.float32(0.001))
MIN_S = 2.0 ** -10
KINK = 1e-3


def geometry(q_tgt, q_src, T, K, inv_K, weights=None):
    """dict of numpy arrays: pair_sum float64 [V,B], pair_count int64 [V,B], err float64 [V,B,H,W] (0 where not
    visible), code uint8 [V,B,H,W], and - of sum(weights * pair_sum), weights [V,B], default ones - grad_q_tgt [B,H,W],
    grad_q_src [V,B,H,W], grad_T [V,B,12], all float64; near_kink bool [V,B,H,W] (visible samples within KINK of a
    kink) and x0, y0 int64 [V,B,H,W], the cell of every sample."""
    qt = torch.tensor(np.asarray(q_tgt, np.float64), requires_grad=True)
    qs = torch.tensor(np.asarray(q_src, np.float64), requires_grad=True)
    Tm = torch.tensor(np.asarray(T, np.float64).reshape(qs.shape[0], qs.shape[1], 3, 4), requires_grad=True)
    Km = torch.tensor(np.asarray(K, np.float64).reshape(-1, 4, 4))
    iK = torch.tensor(np.asarray(inv_K, np.float64).reshape(-1, 4, 4))
    V, B, H, W = qs.shape
    w = torch.ones(V, B, dtype=torch.float64) if weights is None else torch.tensor(np.asarray(weights, np.float64))
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    valid = (qt > 0) & torch.isfinite(qt)
    q_safe = torch.where(valid, qt, torch.ones_like(qt))
    p = [(iK[:, j, 0, None, None] * xs + iK[:, j, 1, None, None] * ys + iK[:, j, 2, None, None]) / q_safe
         for j in range(3)]
    bi = torch.arange(B)[:, None, None]
    sums, counts, errs, codes, kinks, cells = [], [], [], [], [], []
    for v in range(V):
        X = [Tm[v, :, r, 0, None, None] * p[0] + Tm[v, :, r, 1, None, None] * p[1] + Tm[v, :, r, 2, None, None] * p[2]
             + Tm[v, :, r, 3, None, None] for r in range(3)]
        z = X[2]
        c = [Km[:, r, 0, None, None] * X[0] + Km[:, r, 1, None, None] * X[1] + Km[:, r, 2, None, None] * X[2]
             for r in range(3)]
        front = valid & torch.isfinite(z) & (z > MIN_Z) & (c[2] != 0)
        c2 = torch.where(front, c[2], torch.ones_like(z))
        u, t = c[0] / c2, c[1] / c2
        inside = front & (u >= 0) & (u <= W - 1) & (t >= 0) & (t <= H - 1) & (H >= 2) & (W >= 2)
        u, t = torch.where(inside, u, torch.zeros_like(u)), torch.where(inside, t, torch.zeros_like(t))
        x0 = torch.clamp(torch.floor(u.detach()).long(), max=max(W - 2, 0))
        y0 = torch.clamp(torch.floor(t.detach()).long(), max=max(H - 2, 0))
        x1, y1 = torch.clamp(x0 + 1, max=W - 1), torch.clamp(y0 + 1, max=H - 1)
        good = (qs[v] > 0) & torch.isfinite(qs[v])
        src = torch.where(good, qs[v], torch.ones_like(qs[v]))
        taps_good = good[bi, y0, x0] & good[bi, y0, x1] & good[bi, y1, x0] & good[bi, y1, x1]
        s00, s01, s10, s11 = src[bi, y0, x0], src[bi, y0, x1], src[bi, y1, x0], src[bi, y1, x1]
        fx, fy = u - x0, t - y0
        s = (s00 * (1 - fx) + s01 * fx) * (1 - fy) + (s10 * (1 - fx) + s11 * fx) * fy
        a = z * s
        visible = inside & taps_good & (s >= MIN_S) & torch.isfinite(a)
        a = torch.where(visible, a, torch.ones_like(a))
        e = torch.where(visible, torch.abs(a - 1) / (a + 1), torch.zeros_like(a))
        sums.append(e.sum((1, 2)))
        counts.append(visible.sum((1, 2)))
        errs.append(e.detach())
        codes.append(visible.to(torch.uint8) + 2 * (visible & (a.detach() > 1)).to(torch.uint8))
        ud, td, ad = u.detach(), t.detach(), a.detach()
        kinks.append(visible & (((ud - torch.round(ud)).abs() < KINK) | ((td - torch.round(td)).abs() < KINK)
                                | ((ad - 1).abs() < KINK)))
        cells.append((x0, y0))
    pair_sum = torch.stack(sums)
    (w * pair_sum).sum().backward()
    out = dict(pair_sum=pair_sum.detach().numpy(), pair_count=torch.stack(counts).numpy(),
               err=torch.stack(errs).numpy(), code=torch.stack(codes).numpy(), grad_q_tgt=qt.grad.numpy(),
               grad_q_src=qs.grad.numpy(), grad_T=Tm.grad.reshape(V, B, 12).numpy(),
               near_kink=torch.stack(kinks).numpy(), x0=torch.stack([c[0] for c in cells]).numpy(),
               y0=torch.stack([c[1] for c in cells]).numpy())
    out["loss"] = np.float64(out["pair_sum"].sum() / max(int(out["pair_count"].sum()), 1))
    return out


def camera(H, W):
    """(K, inv_K) float32 [4,4]: K = diag(0.58 W, 1.92 H) with the centre at half the size."""
    K = np.eye(4)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 0.58 * W, 1.92 * H, 0.5 * W, 0.5 * H
    return K.astype(np.float32), np.linalg.inv(K).astype(np.float32)


def relative(P_tgt, P_src):
    """float32 [12]: rows 0..2 of the target-to-source matrix of two camera-to-world poses."""
    return (np.linalg.inv(P_src) @ P_tgt)[:3].reshape(12).astype(np.float32)


def source_poses(P_args, V):
    """V (tx, ty, tz, yaw) around a target camera: 0.8 m behind and ahead, 0.1 m aside, yawed -+0.03 rad, and - beyond
    two - steps in between and further out."""
    tx, ty, tz, yaw = P_args
    steps = [-1.0, 1.0, -0.5, 0.5, -1.5, 1.5, -0.25, 0.25][:V]
    return [(tx + 0.1 * k, ty, tz + 0.8 * k, yaw + 0.03 * k) for k in steps]


def scene(B, V, H, W, seed):
    """dict(q_tgt [B,H,W], q_src [V,B,H,W], T [V,B,12], K, inv_K [B,16]) float32: target cameras at
    pose(0.05 b, 0, 0.3 b, 0.01 b); rays that hit nothing get depth 80; target depth carries 3 % multiplicative Gaussian
    noise, source depth is times 1.06 with 1 % noise."""
    rng = np.random.default_rng(seed)
    K, inv_K = camera(H, W)
    iK64 = np.linalg.inv(K.astype(np.float64))

    def depth_of(args):
        d = consist_ref.render(consist_ref.pose(*args), iK64, H, W)
        return np.where(d > 0, d, 80.0)

    q_tgt, q_src, T = np.empty((B, H, W), np.float32), np.empty((V, B, H, W), np.float32), np.empty((V, B, 12), np.float32)
    for b in range(B):
        tgt = (0.05 * b, 0.0, 0.3 * b, 0.01 * b)
        q_tgt[b] = 1.0 / (depth_of(tgt) * (1.0 + 0.03 * rng.standard_normal((H, W))))
        for v, args in enumerate(source_poses(tgt, V)):
            q_src[v, b] = 1.0 / (depth_of(args) * 1.06 * (1.0 + 0.01 * rng.standard_normal((H, W))))
            T[v, b] = relative(consist_ref.pose(*tgt), consist_ref.pose(*args))
    return dict(q_tgt=q_tgt, q_src=q_src, T=T, K=np.tile(K.reshape(1, 16), (B, 1)),
                inv_K=np.tile(inv_K.reshape(1, 16), (B, 1)))
