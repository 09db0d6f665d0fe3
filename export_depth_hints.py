#!/usr/bin/env python3
"""Depth hints of a split from its stereo pairs, matched on the device:

    python export_depth_hints.py --data_path <kitti> --split eigen [--splits_dir splits] [--height 192 --width 640]
                                 [--hint_disparities 128] [--as_disps FILE.npy]

Writes `<splits_dir>/<split>/depth_hints.npy` (int16 [N,h,w], 16 x disparity, -16 = invalid) and prints the mean density.
`--as_disps FILE.npy` also writes the filled hints as scaled disparities:
`python evaluate_depth.py --eval_stereo --eval_split <split> --ext_disp_to_eval FILE.npy` then scores classical stereo
matching like a model (baseboostdepth_amd/hints.py derives the conversion).
"""
from baseboostdepth_amd.hints import export_main

if __name__ == "__main__":
    export_main()
