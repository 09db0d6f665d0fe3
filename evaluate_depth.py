#!/usr/bin/env python3
"""Depth evaluation with the reference's command line:

    python evaluate_depth.py --eval_mono --load_weights_folder <weights> --kt_path <kitti> --eval_split eigen

`--save_clouds DIR [--cloud_count N] [--cloud_stride N] [--cloud_rays pixel|reference]` also writes the point clouds of
the first N images, prediction and ground truth, as binary PLY files.
`--scale_recovery ground [--camera_height 1.65] [--ground_angle 5.0]` scales every mono prediction by the camera's height
above the pixels found to be road instead of by the LiDAR median: the scores of a model that gets no ground truth.
`--scale_recovery lsq` is the protocol of the relative-depth models (MiDaS, DPT, Depth Anything), whose disparity - given
with `--ext_disp_to_eval FILE.npy` - is known up to a scale and a shift: every image is aligned to its inverse ground
truth by least squares before it is scored, the fitted scales and shifts are summarised in place of the ratios, and SILog
and iRMSE follow the seven metrics.  It excludes `--eval_stereo`, `--disable_median_scaling`, `--pred_depth_scale_factor`,
`--eval_split SYNS`, `--save_clouds` and the uncertainty options.
`--uncertainty post [--sparsification_intervals 50] [--save_pred_uncerts] [--save_sparsification FILE.json]` also scores
the ground-truth-free uncertainty map of the flip pass, |d - flip(d')|, by sparsification: a table of AUSE and AURG for
abs_rel, rmse and a1 follows the metrics.  `--ext_uncert_to_eval FILE.npy` scores the maps of `--ext_disp_to_eval`.
"""
from baseboostdepth_amd.evaluation import evaluate
from baseboostdepth_amd.options import MonodepthOptions

if __name__ == "__main__":
    evaluate(MonodepthOptions().parse())
