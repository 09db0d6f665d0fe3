#!/usr/bin/env python3
"""Writes baseboostdepth_amd/magma_lut.hex: the 256 magma colours as the uint8 triples matplotlib's
`ScalarMappable.to_rgba(...)[..., :3] * 255 -> uint8` produces (truncation of the float table times 255), one
`rrggbb` line per entry.  Run once where matplotlib is installed; the product reads the file and never imports
matplotlib.

    python tools/make_magma_lut.py
"""
import os

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "baseboostdepth_amd", "magma_lut.hex")


def magma_u8():
    import matplotlib
    table = matplotlib.colormaps["magma"](np.arange(256))[:, :3]
    return (table * 255).astype(np.uint8)


def main():
    lut = magma_u8()
    assert lut.shape == (256, 3)
    with open(OUT, "w") as f:
        for r, g, b in lut.tolist():
            f.write("%02x%02x%02x\n" % (r, g, b))
    print("wrote", OUT)


if __name__ == "__main__":
    main()
