"""Depth hints of a split as files (`export_depth_hints.py`): the semi-global matcher of the training step
(`ops.stereo_hints`) run over the stereo pairs of a split's file list.

    <splits_dir>/<split>/depth_hints.npy   int16 [N,h,w] at --height x --width: 16 x disparity in pixels of THAT size,
                                           -16 where the matcher rejected the pixel
    --as_disps FILE.npy                    float32 [N,h,w]: the FILLED hints in the convention of the depth network's
                                           scaled disparity, which `evaluate_depth.py --eval_stereo --ext_disp_to_eval
                                           FILE.npy` scores unchanged - a classical stereo row of the KITTI table

The conversion.  The evaluation turns a disparity q into metres as 5.4 / q (`evaluation.STEREO_SCALE_FACTOR`: the
network's unit is a baseline of 0.1, KITTI's is 0.54 m).  A match of d pixels at width w has the depth fx * 0.1 / d
network units with fx = 0.58 w (`synthetic.kitti_intrinsics`, the K of the loader), so q = d / (0.058 w).  A pixel that is
invalid even after the fill (its whole row was) and a disparity of 0 take 1/16 pixel, the matcher's resolution: the
evaluation clamps their depth to 80 m.
"""
import argparse
import os

import numpy as np
import torch

from . import ops
from .kitti_utils import SPLITS, _split_lines

SIDE_DIR = {"l": "image_02", "r": "image_03"}


def split_pairs(split_dir, split, data_path, img_ext=".jpg"):
    """[(frame, partner, side flag)] of a split's file list (`folder frame side` lines): the frame of the line's camera,
    the other camera's frame, and 0 where the partner lies to the right (the line's camera is the left one)."""
    pairs = []
    for t in _split_lines(split_dir, split):
        folder, frame, side = t[0], int(t[1]), (t[2] if len(t) > 2 else "l")
        path = lambda s: os.path.join(data_path, folder, SIDE_DIR[s], "data", "{:010d}{}".format(frame, img_ext))  # noqa: E731
        pairs.append((path(side), path({"l": "r", "r": "l"}[side]), 0 if side == "l" else 1))
    return pairs


def load_image(path, height, width):
    """RGB float32 [3,height,width] in [0,1], resized as the loader resizes (Lanczos)."""
    from PIL import Image
    with Image.open(path) as img:
        arr = np.asarray(img.convert("RGB").resize((width, height), Image.LANCZOS), dtype=np.float32)
    return torch.from_numpy(arr.transpose(2, 0, 1) / np.float32(255.0))


def hints_as_disps(filled16, width):
    """int16 [N,h,w] filled hints -> float32 scaled disparities for `--ext_disp_to_eval` (see the module text)."""
    px = np.maximum(filled16.astype(np.float32), 1.0) / np.float32(16.0)
    return (px / np.float32(0.058 * width)).astype(np.float32)


def export_depth_hints(data_path, split, splits_dir="splits", height=192, width=640, disparities=128, output=None,
                       as_disps=None, device="cuda:0", backend=None, batch_size=12, img_ext=".jpg"):
    """Writes `depth_hints.npy` (and `as_disps`) and returns (path, mean density)."""
    split_dir = os.path.join(splits_dir, split)
    output = output or os.path.join(split_dir, "depth_hints.npy")
    pairs = split_pairs(split_dir, split, data_path, img_ext)
    if not pairs:
        raise ValueError("%s names no frame" % split_dir)
    print("Exporting depth hints for {}: {} pairs at {} x {}, {} disparities".format(split, len(pairs), height, width,
                                                                                    disparities))
    scratch = torch.empty(ops.sgm_scratch_bytes(min(batch_size, len(pairs)), height, width, disparities), dtype=torch.uint8,
                          device=device)
    hints, filled, valid = [], [], 0
    for i in range(0, len(pairs), batch_size):
        chunk = pairs[i:i + batch_size]
        left = torch.stack([load_image(p[0], height, width) for p in chunk]).to(device)
        right = torch.stack([load_image(p[1], height, width) for p in chunk]).to(device)
        side = torch.tensor([p[2] for p in chunk], dtype=torch.int32).to(device)
        disp16, count = ops.stereo_hints(left, right, side, disparities, scratch=scratch, backend=backend)
        hints.append(disp16.cpu().numpy())
        valid += int(count.sum())
        if as_disps:
            filled.append(ops.stereo_hints(left, right, side, disparities, fill=True, scratch=scratch,
                                           backend=backend)[0].cpu().numpy())
    hints = np.concatenate(hints)
    density = valid / hints.size
    print("Saving to {}".format(output))
    np.save(output, hints)
    if as_disps:
        print("Saving the filled hints as scaled disparities to {}".format(as_disps))
        np.save(as_disps, hints_as_disps(np.concatenate(filled), width))
    print("Mean density: {:.4f} of {} pixels valid".format(density, hints.size))
    return output, density


def export_main(argv=None, backend=None):
    parser = argparse.ArgumentParser(description="export_depth_hints")
    parser.add_argument("--data_path", type=str, required=True, help="path to the root of the KITTI data")
    parser.add_argument("--split", type=str, required=True, choices=[s for s in SPLITS if s != "SYNS"])
    parser.add_argument("--splits_dir", type=str, default="splits", help="folder that holds <split>/test_files.txt")
    parser.add_argument("--height", type=int, default=192)
    parser.add_argument("--width", type=int, default=640)
    parser.add_argument("--hint_disparities", type=int, default=128, choices=[64, 128, 192, 256])
    parser.add_argument("--output", type=str, default=None, help="default: <splits_dir>/<split>/depth_hints.npy")
    parser.add_argument("--as_disps", type=str, default=None, metavar="FILE.npy",
                        help="also write the filled hints as scaled disparities for --ext_disp_to_eval")
    parser.add_argument("--batch_size", type=int, default=12)
    parser.add_argument("--device", type=str, default="cuda:0")
    opt = parser.parse_args(argv)
    return export_depth_hints(opt.data_path, opt.split, opt.splits_dir, opt.height, opt.width, opt.hint_disparities,
                              opt.output, opt.as_disps, opt.device, backend, opt.batch_size)
