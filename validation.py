#!/usr/bin/env python3
"""Checkpoint comparison sheets with the reference's command line (its hard-coded paths are options here):

    python validation.py --model_name A B C --models_dir <dir> --kt_path <KITTI_RAW> [--error_maps] [--output validation_vis]
"""
from baseboostdepth_amd.compare import main

if __name__ == "__main__":
    main()
