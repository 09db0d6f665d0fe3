"""Reference of the flip post-processing: Monodepth2's `batch_post_process_disparity` in its literal numpy formulation.
Float64 multiply, add and clip only, so it gives the same bits on any host; computed live, no golden file."""
import numpy as np

# (n, h, w): a single pixel; two columns; an odd width with its self-mirrored centre column, below one wavefront, 1 pixel
# per row inside the 0.05-0.1 ramp; more than one column tile with 6 pixels inside the ramp; exactly one wavefront
SHAPES = [(1, 1, 1), (2, 3, 2), (3, 5, 41), (2, 7, 130), (1, 2, 64)]


def batch_post_process_disparity(l_disp, r_disp):
    """l_disp, r_disp float32 [n,h,w], r_disp already flipped back; returns float64 [n,h,w]."""
    _, h, w = l_disp.shape
    m_disp = 0.5 * (l_disp + r_disp)
    l, _ = np.meshgrid(np.linspace(0, 1, w), np.linspace(0, 1, h))
    l_mask = (1.0 - np.clip(20 * (l - 0.05), 0, 1))[None, ...]
    r_mask = l_mask[:, :, ::-1]
    return r_mask * l_disp + l_mask * r_disp + (1.0 - l_mask - r_mask) * m_disp


def reference(disp):
    """disp float32 [2n,h,w] (or [2n,1,h,w]), second half still flipped -> float32 [n,h,w]."""
    disp = np.asarray(disp)
    if disp.ndim == 4:
        disp = disp[:, 0]
    assert disp.dtype == np.float32 and disp.ndim == 3 and disp.shape[0] % 2 == 0
    n = disp.shape[0] // 2
    return batch_post_process_disparity(disp[:n], disp[n:, :, ::-1]).astype(np.float32)


def make_input(n, h, w, seed):
    rng = np.random.default_rng(seed)
    return (0.01 + 9.99 * rng.random((2 * n, h, w))).astype(np.float32)
