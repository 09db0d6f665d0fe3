#!/usr/bin/env python3
"""Ground-truth depth maps of a split with the reference's command line:

    python export_gt_depth.py --data_path <kitti> --split eigen [--splits_dir splits] [--output gt_depths.npz]

`eigen` / `eigen_zhou` project the Velodyne scans on the device (baseboostdepth_amd/kitti_utils.py);
`eigen_benchmark` reads the improved ground-truth PNGs.  Writes `<splits_dir>/<split>/gt_depths.npz`.
"""
from baseboostdepth_amd.kitti_utils import export_main

if __name__ == "__main__":
    export_main()
