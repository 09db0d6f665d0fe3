"""CPU reference of the SYNS-Patches metrics (test infrastructure only - never imported by the product path).

A numpy-only restatement of evaluate_depth.py:26-102, :244-297 and trainer.py:576-594 / layers.py:252-269: the filters
in float64, a brute-force exact distance transform, a brute-force float32 nearest neighbour.  The reference itself
needs cv2, scipy and the chamfer_distance CUDA extension; cv2 and chamfer_distance are not available, so agreement
with OpenCV's own float32 blur rounding and with the extension's kernel is NOT pinned - what is restated here are the
documented filters (getGaussianKernel(3, 1); Sobel ksize 5 = smoothing 1 4 6 4 1 x derivative -1 -2 0 2 1;
BORDER_REFLECT_101) and the definition of the chamfer distance.  scipy's distance transform is compared directly where
scipy exists (tests/test_syns_port.py)."""
import numpy as np

LOG_FLOOR = 1.1920928955078125e-07
SMOOTH = np.array([1.0, 4.0, 6.0, 4.0, 1.0])
DERIV = np.array([-1.0, -2.0, 0.0, 2.0, 1.0])
SOBEL_ABS_SUM = 96.0            # sum |smooth x deriv| = 16 * 6


def syns_camera(h=376, w=1242, fov=(25.46, 84.10)):
    """syns_dataset.py:20-38: K (float32 3x3) and its pseudo-inverse."""
    fy_deg, fx_deg = fov
    cx, cy = w // 2, h // 2
    fx = cx / np.tan(np.deg2rad(fx_deg) / 2)
    fy = cy / np.tan(np.deg2rad(fy_deg) / 2)
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float32)
    return K, np.linalg.pinv(K)


def to_log(depth):
    return (depth > 0) * np.log(depth.clip(min=LOG_FLOOR))


def _filter(img, kernel, axis):
    r = len(kernel) // 2
    pad = [(0, 0), (0, 0)]
    pad[axis] = (r, r)
    p = np.pad(img, pad, mode="reflect")            # BORDER_REFLECT_101
    out = np.zeros_like(img)
    n = img.shape[axis]
    for i, k in enumerate(kernel):
        out = out + k * np.take(p, np.arange(i, i + n), axis=axis)
    return out


def gaussian_kernel():
    k = np.exp(-np.array([-1.0, 0.0, 1.0]) ** 2 / 2)
    return (k / k.sum()).astype(np.float32)


def edge_magnitude(depth, dtype=np.float64):
    """|Sobel(GaussianBlur(to_log(depth)))| with the blur carried in `dtype` (float64: the reference of the tests;
    float32: a second rounding order, used to measure how many pixels can flip)."""
    L = to_log(depth.astype(np.float32)).astype(np.float32).astype(dtype)
    k = gaussian_kernel().astype(dtype)
    B = _filter(_filter(L, k, 1), k, 0).astype(dtype)
    if dtype == np.float32:
        B = B.astype(np.float32)
    B = B.astype(np.float64)
    dx = _filter(_filter(B, DERIV, 1), SMOOTH, 0)
    dy = _filter(_filter(B, SMOOTH, 1), DERIV, 0)
    return np.sqrt(dx ** 2 + dy ** 2), L


def pred_edges(depth, dtype=np.float64):
    """(edge bool [H,W], mag float64, mean, delta): delta = 96 * sqrt(2) * 4 * 2^-24 * max|L| bounds what four float32
    roundings between L and B can move the magnitude by; pixels with |mag - mean| <= delta may legitimately flip."""
    mag, L = edge_magnitude(depth, dtype)
    mean = mag.mean()
    delta = SOBEL_ABS_SUM * np.sqrt(2.0) * 4 * 2.0 ** -24 * float(np.abs(L).max())
    return mag > mean, mag, mean, delta


def edt_sq(mask):
    """Exact squared Euclidean distance to the nearest True pixel (int64), brute force over rows: column distances
    first, then min over x' of (x - x')^2 + g^2[x'].  2 ** 30 where the mask is empty."""
    mask = np.asarray(mask, bool)
    H, W = mask.shape
    far = 32768
    g = np.full((H, W), far, np.int64)
    d = np.full(W, far, np.int64)
    for y in range(H):
        d = np.where(mask[y], 0, np.minimum(d + 1, far))
        g[y] = d
    d = np.full(W, far, np.int64)
    for y in range(H - 1, -1, -1):
        d = np.where(mask[y], 0, np.minimum(d + 1, far))
        g[y] = np.minimum(g[y], d)
    g2 = np.where(g >= far, 2 ** 30, g * g)
    xs = np.arange(W)
    off = (xs[:, None] - xs[None, :]) ** 2               # [x, x']
    out = np.empty((H, W), np.int64)
    for y in range(H):
        out[y] = (off + g2[y][None, :]).min(1)
    return out


def edge_metrics(pred_edge, gt, gt_edge, lo, hi, th=10.0):
    """evaluate_depth.py:89-95 / layers.py:256-269 -> dict(edge_Acc, edge_comp, n_near, n_tgt, n_edge)."""
    valid = np.logical_and(gt > lo, gt < hi)
    ge = np.asarray(gt_edge)
    ge = (ge[..., 0] if ge.ndim == 3 else ge) != 0
    tgt = np.logical_and(valid, ge)
    pe = np.asarray(pred_edge, bool)
    out = {"n_tgt": int(tgt.sum()), "n_edge": int(pe.sum()), "n_valid": int(valid.sum())}
    if not tgt.any():
        out.update(edge_Acc=np.nan, edge_comp=np.nan, n_near=0)
        return out
    D_t = np.sqrt(edt_sq(tgt).astype(np.float64))
    near = pe & (D_t < th)
    out["n_near"] = int(near.sum())
    if near.sum():
        D_p = np.sqrt(edt_sq(pe).astype(np.float64))
        out.update(edge_Acc=D_t[near].mean(), edge_comp=D_p[tgt].mean())
    else:
        out.update(edge_Acc=float(th), edge_comp=float(th))
    return out


def err(pred_scaled, gt, lo, hi):
    """evaluate_depth.py:72-73 on the median-scaled, clamped prediction (float32 in, float64 mean)."""
    valid = np.logical_and(gt > lo, gt < hi)
    return np.abs(pred_scaled[valid] - gt[valid]).astype(np.float64).mean()


def backproject(depth, inv_K, rays="reference"):
    """evaluate_depth.py:26-41 in float32: flat pixel k -> depth[k] * inv_K (u, v, 1); the reference's grid gives
    (u, v) = (k // H, k % H), the pixel's own ray is (k % W, k // W)."""
    H, W = depth.shape
    k = np.arange(H * W)
    u, v = (k // H, k % H) if rays == "reference" else (k % W, k // W)
    u, v = u.astype(np.float32), v.astype(np.float32)
    iK = np.asarray(inv_K, np.float32)
    d = depth.reshape(-1).astype(np.float32)
    return np.stack([((iK[j, 0] * u + iK[j, 1] * v) + iK[j, 2]) * d for j in range(3)], 1).astype(np.float32)


def nn_sq(a, b, chunk=256):
    """min_j |a_i - b_j|^2 in float32, (dx*dx + dy*dy) + dz*dz from the differences."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    out = np.full(len(a), np.inf, np.float32)
    if len(b) == 0:
        return out
    for s in range(0, len(a), chunk):
        q = a[s:s + chunk]
        dx = q[:, None, 0] - b[None, :, 0]
        dy = q[:, None, 1] - b[None, :, 1]
        dz = q[:, None, 2] - b[None, :, 2]
        out[s:s + chunk] = ((dx * dx + dy * dy) + dz * dz).min(1)
    return out


def f_iou(nn_p, nn_t, th=0.1):
    """evaluate_depth.py:49-55 in float32 -> (f1, iou, P, R)."""
    one = np.float32(1)
    N = np.float32(len(nn_p))
    with np.errstate(invalid="ignore", divide="ignore"):
        P = np.float32((np.sqrt(nn_p) < np.float32(th)).sum()) / N
        R = np.float32((np.sqrt(nn_t) < np.float32(th)).sum()) / np.float32(len(nn_t))
        if P < np.float32(1e-3) and R < np.float32(1e-3):
            return P, P, P, R
        f = (np.float32(2) * P * R) / (P + R)
        iou = (P * R) / ((P + R) - (P * R))
    return f, iou, P, R


def pointcloud_metrics(pred_org, gt, inv_K, lo, hi, rays="reference", th=0.1):
    """`pred_org`: the median-scaled, clamped prediction at ground-truth size (float32)."""
    valid = np.logical_and(gt > lo, gt < hi).reshape(-1)
    P = backproject(pred_org, inv_K, rays)[valid]
    T = backproject(gt, inv_K, rays)[valid]
    nn_p, nn_t = nn_sq(P, T), nn_sq(T, P)
    return f_iou(nn_p, nn_t, th) + (nn_p, nn_t)
