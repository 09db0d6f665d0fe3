"""Ground-truth depth from KITTI's Velodyne scans, on the device (the reference's kitti_utils.py and export_gt_depth.py).

The reference projects one scan at a time with numpy and resolves duplicate pixels in a Python loop (about 0.05 s per
frame); every user runs that over a split once to get `splits/<split>/gt_depths.npz`, which `evaluate_depth.py` and the
trainer's validation need.  Here calibrations are parsed once per directory, the .bin files are read by host threads,
and a batch of frames is uploaded as it lies on disk and turned into depth maps by ONE `bbd_velo_depth` call that
writes straight into the ragged buffer of an `evaluation.GroundTruthSet` - `evaluate()` can score against it without
the maps ever visiting the host, and `export_gt_depth.py` copies it back once to write the npz.

The arithmetic (float64 projection, np.round, "last point wins", the minimum over duplicated sub2ind keys including
the reference's (w - 1) key collision) is restated in csrc/bbd_velo_math.h.
"""
import argparse
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import ops

BATCH_FRAMES = 32          # frames per upload + launch: 32 KITTI frames are 60 MB of points and 240 MB of scratch
_NUMERIC = set("0123456789.e+- ")
_CALIB = {}


def load_velodyne_points(filename):
    """A KITTI scan as float32 [N,4] = x (forward), y (left), z (up), 1 (the reflectance column made homogeneous)."""
    scan = np.fromfile(filename, dtype=np.float32).reshape(-1, 4)
    scan[:, 3] = 1.0
    return scan


def read_calib_file(path):
    """`key: value` lines of a KITTI calibration file; values made of numbers only become float64 arrays, the others
    (dates) stay strings."""
    out = {}
    with open(path, "r") as f:
        for line in f:
            if ":" not in line:
                continue
            name, text = line.split(":", 1)
            text = text.strip()
            out[name] = text
            if _NUMERIC.issuperset(text):
                try:
                    out[name] = np.array([float(t) for t in text.split(" ")])
                except ValueError:
                    pass
    return out


def _calibration(calib_dir):
    key = os.path.abspath(calib_dir)
    if key not in _CALIB:
        _CALIB[key] = (read_calib_file(os.path.join(calib_dir, "calib_cam_to_cam.txt")),
                       read_calib_file(os.path.join(calib_dir, "calib_velo_to_cam.txt")))
    return _CALIB[key]


def velo_projection(calib_dir, cam=2):
    """(P, (h, w)): P = P_rect_0{cam} . R_cam2rect . velo2cam as float64 [3,4], multiplied in the reference's order
    (kitti_utils.py:50-62), and the image size, which is S_rect_02 reversed whichever camera is asked for."""
    cam2cam, velo2cam = _calibration(calib_dir)
    v2c = np.eye(4)
    v2c[:3, :3] = velo2cam["R"].reshape(3, 3)
    v2c[:3, 3] = velo2cam["T"]
    rect = np.eye(4)
    rect[:3, :3] = cam2cam["R_rect_00"].reshape(3, 3)
    p_rect = cam2cam["P_rect_0" + str(cam)].reshape(3, 4)
    P = np.dot(np.dot(p_rect, rect), v2c)
    w, h = (int(s) for s in cam2cam["S_rect_02"].astype(np.int32))
    return P, (h, w)


def _read_scan(filename):
    return np.fromfile(filename, dtype=np.float32).reshape(-1, 4)


def generate_depth_maps(frames, device, vel_depth=False, backend=None, batch_frames=BATCH_FRAMES, workers=8):
    """Depth maps of `frames` = [(calib_dir, velo_filename, cam), ...] as an `evaluation.GroundTruthSet` on `device`
    (maps back to back in `.buffer`, sizes in `.shapes`): generate_depth_map(calib_dir, velo_filename, cam, vel_depth)
    of the reference for every frame, cast to float32.  Scans are read on `workers` host threads one batch ahead of the
    device; every batch of `batch_frames` frames is one upload and one `bbd_velo_depth` call; nothing synchronises."""
    from .evaluation import GroundTruthSet
    device = torch.device(device)
    frames = list(frames)
    geometry = [velo_projection(calib_dir, cam) for calib_dir, _, cam in frames]
    shapes = [g[1] for g in geometry]
    offsets = np.concatenate([[0], np.cumsum([h * w for h, w in shapes], dtype=np.int64)]).tolist()
    out = torch.empty(offsets[-1], dtype=torch.float32, device=device)
    batches = [range(b, min(b + batch_frames, len(frames))) for b in range(0, len(frames), batch_frames)]
    with ThreadPoolExecutor(max_workers=max(1, workers)) as pool:
        def submit(k):
            return [pool.submit(_read_scan, frames[i][1]) for i in batches[k]] if k < len(batches) else None
        pending = submit(0)
        for k, idx in enumerate(batches):
            ahead = submit(k + 1)
            scans = [f.result() for f in pending]
            host = torch.from_numpy(np.concatenate(scans) if scans else np.zeros((0, 4), np.float32))
            if device.type == "cuda":
                host = host.pin_memory()
            ops.velo_depth(host.to(device, non_blocking=True), [len(s) for s in scans],
                           np.stack([geometry[i][0] for i in idx]), [shapes[i] for i in idx], out=out,
                           offsets=[offsets[i] for i in idx], vel_depth=vel_depth, backend=backend)
            pending = ahead
    return GroundTruthSet.from_packed(out, shapes)


def generate_depth_map(calib_dir, velo_filename, cam=2, vel_depth=False, device="cuda:0", backend=None):
    """One frame, as a float32 numpy array [h,w] (the reference returns float64; its export casts to float32)."""
    gts = generate_depth_maps([(calib_dir, velo_filename, cam)], device, vel_depth, backend)
    return gts.buffer.cpu().numpy().reshape(gts.shapes[0])


# ---------------------------------------------------------------------------- export_gt_depth.py
SPLITS = ["eigen", "eigen_zhou", "eigen_benchmark", "SYNS"]


def _split_lines(split_dir, split):
    name = "val_files.txt" if split == "eigen_zhou" else "test_files.txt"          # export_gt_depth.py:32-35
    with open(os.path.join(split_dir, name)) as f:
        return [line.split() for line in f.read().splitlines() if line.strip()]


def split_frames(split_dir, split, data_path):
    """The (calib_dir, velo_filename, 2) triples of a split's file list (export_gt_depth.py:55-59)."""
    return [(os.path.join(data_path, t[0].split("/")[0]),
             os.path.join(data_path, t[0], "velodyne_points/data", "{:010d}.bin".format(int(t[1]))), 2)
            for t in _split_lines(split_dir, split)]


def export_gt_depths(data_path, split, splits_dir="splits", output=None, device="cuda:0", backend=None):
    """Writes what the reference's export_gt_depth.py writes and returns the path."""
    split_dir = os.path.join(splits_dir, split)
    output = output or os.path.join(split_dir, "gt_depths.npz")
    print("Exporting ground truth depths for {}".format(split))
    if split == "eigen_benchmark":                 # improved ground truth: 16-bit PNGs, host only (export_gt_depth.py:60-63)
        from PIL import Image
        maps = []
        for t in _split_lines(split_dir, split):
            png = os.path.join(data_path, t[0], "proj_depth", "groundtruth", "image_02", "{:010d}.png".format(int(t[1])))
            maps.append(np.array(Image.open(png)).astype(np.float32) / 256)
    else:                                          # cam 2, depth = the point's forward distance (export_gt_depth.py:59)
        gts = generate_depth_maps(split_frames(split_dir, split, data_path), device, vel_depth=True, backend=backend)
        flat = gts.buffer.cpu().numpy()            # the one copy to the host
        ends = np.cumsum([h * w for h, w in gts.shapes])
        maps = [m.reshape(s) for m, s in zip(np.split(flat, ends[:-1]), gts.shapes)] if gts.shapes else []
    if len(set(m.shape for m in maps)) == 1:
        data = np.stack(maps)                      # the reference's np.array(list): [N,h,w]
    else:                                          # mixed sizes: numpy >= 1.24 builds no ragged array implicitly
        data = np.empty(len(maps), dtype=object)
        for i, m in enumerate(maps):
            data[i] = m
    print("Saving to {}".format(output))
    np.savez_compressed(output, data=data)
    return output


def export_main(argv=None, backend=None):
    parser = argparse.ArgumentParser(description="export_gt_depth")
    parser.add_argument("--data_path", type=str, required=True, help="path to the root of the KITTI data")
    parser.add_argument("--split", type=str, required=True, choices=SPLITS, help="which split to export gt from")
    parser.add_argument("--splits_dir", type=str, default="splits", help="folder that holds <split>/test_files.txt")
    parser.add_argument("--output", type=str, default=None, help="default: <splits_dir>/<split>/gt_depths.npz")
    parser.add_argument("--device", type=str, default="cuda:0")
    opt = parser.parse_args(argv)
    if opt.split == "SYNS":
        parser.error("--split SYNS selects parts of the reference that are outside this build's scope")
    return export_gt_depths(opt.data_path, opt.split, opt.splits_dir, opt.output, opt.device, backend)
