#!/usr/bin/env python3
"""Single-image depth prediction with the reference's command line:

    python test_simple.py --image_path <image or folder> --save_path <folder> --ext png --weights <weights folder>

Writes `<name>_Base.jpg` (magma-coloured disparity at the image's own size); `--save_npy` adds `<name>_disp.npy`.
"""
from baseboostdepth_amd.inference import main

if __name__ == "__main__":
    main()
