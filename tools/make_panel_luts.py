#!/usr/bin/env python3
"""Writes baseboostdepth_amd/panel_luts.hex: the colour tables of the training-log panel that magma_lut.hex does not
already hold - the 256 plasma colours (the reference's `colormap()`, trainer.py:1102) followed by the 20 colours of
`tab20` (the arg-min map's palette) - as `trunc(rgb * 255)` uint8 triples, one `rrggbb` line per entry, like
tools/make_magma_lut.py.  Run once where matplotlib is installed; the product reads the file and never imports
matplotlib.

    python tools/make_panel_luts.py
"""
import os

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "baseboostdepth_amd", "panel_luts.hex")


def plasma_u8():
    import matplotlib
    return (matplotlib.colormaps["plasma"](np.arange(256))[:, :3] * 255).astype(np.uint8)


def tab20_u8():
    import matplotlib
    return (matplotlib.colormaps["tab20"](np.arange(20))[:, :3] * 255).astype(np.uint8)


def main():
    lut = np.concatenate([plasma_u8(), tab20_u8()], 0)
    assert lut.shape == (276, 3)
    with open(OUT, "w") as f:
        for r, g, b in lut.tolist():
            f.write("%02x%02x%02x\n" % (r, g, b))
    print("wrote", OUT)


if __name__ == "__main__":
    main()
