#!/usr/bin/env python3
"""Pose evaluation on KITTI odometry with the reference's command line:

    python evaluate_pose.py --eval_split odom_9 --load_weights_folder <weights> --kt_path <kitti> [--odom_path <odometry>]
"""
from baseboostdepth_amd.evaluation import evaluate_pose
from baseboostdepth_amd.options import MonodepthOptions

if __name__ == "__main__":
    evaluate_pose(MonodepthOptions().parse())
