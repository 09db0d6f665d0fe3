"""Inputs and tile lists shared by the CPU tier (tests/test_panel_port.py, host port) and the GPU tier
(tests/test_gpu_panel.py, HIP) of the training-log panel.  All inputs are built on the host from fixed seeds, so both
tiers render the same data."""
import numpy as np
import torch

import fused_runner
import panel_ref
from golden_io import Case
from baseboostdepth_amd import ops, synthetic

WARP_CASES = ["md2_b2_32x64", "tri_7765_32x64", "tri_0000_16x32"]
GRID_SIZES = [(5, 7), (17, 33)]
COLS = 4


def luts():
    lut = ops.panel_luts("cpu").numpy()
    return lut[:256], lut[256:512], lut[512:]


def warp_jobs(plan):
    """(kind, frame, row inside the job, sample, pose row) of every warp of a plan, in pose-table order."""
    return [(kind, f, j, b, plan.pose_row(kind, f, b)) for kind, f in plan.pose_jobs for j, b in enumerate(plan.jobs[f])]


def run_case(name, backend, device):
    """A golden case through the fused path with materialised warps -> (case, trainer, inputs, outputs)."""
    case = Case(name, device=device)
    tr, inputs, outputs, _ = fused_runner.run_direct_case(case, backend, device=device)
    return case, tr, inputs, outputs


def render_case_warps(tr, inputs, outputs, backend):
    """One WARP tile per warp job of the case, row-major in a COLS-wide grid -> (panel, jobs, rows)."""
    plan = tr.plan
    jobs = warp_jobs(plan)
    proj = ops.pose_table(plan, inputs[("K", 0)], inputs[("inv_K", 0)],
                          {k: v.detach() for k, v in tr._job_poses(inputs, outputs).items()})
    depth = outputs[("depth", 0, 0)]
    tiles = []
    for i, (kind, f, j, b, p) in enumerate(jobs):
        src = inputs[("color", f, 0)][plan.source_row(f, b)]
        tiles.append((i // COLS, i % COLS, "warp", src, depth[b, 0], p))
    rows = -(-len(jobs) // COLS)
    panel, _ = ops.train_panel(tiles, proj, tr.opt.height, tr.opt.width, rows, COLS, backend)
    return panel, jobs, rows


def scalar_planes():
    ramp = np.arange(35, dtype=np.float32).reshape(5, 7) * np.float32(0.37) - np.float32(3.0)
    one_nan = ramp.copy()
    one_nan[2, 3] = np.nan
    own_max = np.random.RandomState(3).rand(5, 7).astype(np.float32)
    own_max[4, 6] = own_max.max() + np.float32(0.5)
    return {"ramp": ramp, "constant": np.full((5, 7), 0.25, np.float32), "one_nan": one_nan,
            "all_nan": np.full((5, 7), np.nan, np.float32), "own_max": own_max}


BOTH_LUTS = ("ramp", "one_nan", "own_max")


def argmin_map():
    ids = (np.arange(35) % 20).astype(np.uint8).reshape(5, 7)
    assert set(ids.ravel().tolist()) == set(range(20))
    return ids


def grid_inputs(H, W, seed=11):
    """Host tensors of the 3 x 2 test grid: an image, two planes, an arg-min map and one warp (source, depth, pose row 1
    of a 3-row table whose row 0 is garbage - the row offset must be honoured)."""
    g = torch.Generator().manual_seed(seed + H * 131 + W)
    img = torch.rand(3, H, W, generator=g) * 1.2 - 0.1
    plane_a = torch.randn(H, W, generator=g)
    plane_b = torch.rand(H, W, generator=g)
    plane_b[H // 2, W // 2] = float("nan")
    ids = torch.randint(0, 24, (H, W), generator=g).to(torch.uint8)
    src = torch.round(torch.rand(3, H, W, generator=g) * 255) / 255
    depth = 1.0 + 9.0 * torch.rand(H, W, generator=g)
    K, iK = synthetic.kitti_intrinsics(H, W)
    T = torch.eye(4)
    T[0, 3], T[2, 3] = 0.3, -0.05
    rows = ops.pose_table_rows(torch.stack([torch.full((4, 4), 1e3), T, torch.eye(4)]),
                               torch.from_numpy(K)[None].repeat(3, 1, 1), torch.from_numpy(iK)[None].repeat(3, 1, 1))
    return {"img": img, "plane_a": plane_a, "plane_b": plane_b, "ids": ids, "src": src, "depth": depth, "pose": rows}


def grid_tiles(d):
    """3 x 2 grid; cell (2, 0) stays empty."""
    return [(0, 0, "color", d["img"]), (0, 1, "scalar", d["plane_a"], "plasma"), (1, 0, "argmin", d["ids"], 5, 4),
            (1, 1, "scalar", d["plane_b"], "magma"), (2, 1, "warp", d["src"], d["depth"], 1)]


def render_grid(H, W, backend, device):
    d = {k: v.to(device) for k, v in grid_inputs(H, W).items()}
    return ops.train_panel(grid_tiles(d), d["pose"], H, W, 3, 2, backend)


def hist_input(seed=5):
    """uint8 [3, 9, 13] with every id 0..19 and the ids 20 and 255 (which must go uncounted); 117 pixels per sample, so
    the samples start at every alignment of a 4-byte word."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(0, 20, (3, 9, 13), generator=g).to(torch.uint8)
    a.view(3, -1)[0, :20] = torch.arange(20, dtype=torch.uint8)
    a[1, 0, 0], a[2, 8, 12], a[0, 4, 4] = 255, 255, 20
    return a


def bincount(a):
    flat = a.reshape(a.shape[0], -1).long()
    return torch.stack([torch.bincount(r, minlength=256)[:20] for r in flat]).to(torch.int32)


def quantised(t):
    """[n,3,H,W] fp32 -> [n,H,W,3] uint8 (numpy), rounded to nearest."""
    return panel_ref.quantise(t.detach().cpu().numpy()).transpose(0, 2, 3, 1)
