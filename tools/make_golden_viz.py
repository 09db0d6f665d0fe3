#!/usr/bin/env python3
"""Golden vectors for the colour-mapped disparity of single-image prediction, from the reference's own tail
(test_simple.py:135-148) executed with torch CPU, numpy and matplotlib: F.interpolate to the original size, the live
reference's `layers.disp_to_depth` (imported unmodified through tools/refshim.py), np.percentile(., 95),
matplotlib's Normalize + ScalarMappable('magma').  Output: tests/golden/viz_cases.npz (data only): per case the input
disparity, the original size, the scaled disparity s, vmin, vmax and the uint8 colours; plus matplotlib's magma table.

    python tools/make_golden_viz.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refshim  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden", "viz_cases.npz")
torch.set_num_threads(1)

# (name, network h, w, original H0, W0, kind).  ATen blends in one of two orders, chosen by H0 + W0 <= 128.
CASES = [("small_up", 24, 40, 48, 76, "smooth"), ("small_down", 32, 64, 7, 9, "smooth"),
         ("small_same", 32, 64, 32, 64, "smooth"), ("big_up", 48, 160, 80, 250, "smooth"),
         ("big_down", 64, 208, 40, 130, "smooth"), ("big_same", 48, 160, 48, 160, "smooth"),
         ("constant", 16, 32, 40, 70, "constant"), ("tied_max", 32, 96, 75, 230, "tied")]


def synth(gen, h, w, kind):
    if kind == "constant":
        return torch.zeros(1, 1, h, w)       # (a non-zero constant does not stay constant: the blend weights round)
    low = torch.rand(1, 1, h // 8 + 1, w // 8 + 1, generator=gen)
    disp = torch.nn.functional.interpolate(low, size=(h, w), mode="bicubic", align_corners=True)
    disp = (disp + 0.02 * torch.rand(1, 1, h, w, generator=gen)).clamp(0.001, 0.999)
    if kind == "tied":                       # a saturated region: far more than 5 % of the pixels at the maximum
        disp[..., : h // 2, : w // 3] = 1.0
    return disp.float().contiguous()


def main():
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib as mpl
    import matplotlib.cm as cm
    _, ref_layers, _ = refshim.import_reference()
    out = {"lut": (mpl.colormaps["magma"](np.arange(256))[:, :3] * 255).astype(np.uint8)}
    gen = torch.Generator().manual_seed(2024)
    for name, h, w, H0, W0, kind in CASES:
        disp = synth(gen, h, w, kind)
        resized = torch.nn.functional.interpolate(disp, (H0, W0), mode="bilinear", align_corners=False)
        scaled, _ = ref_layers.disp_to_depth(resized, 0.1, 80)
        s = scaled.squeeze().cpu().numpy()
        vmax = np.percentile(s, 95)
        mapper = cm.ScalarMappable(norm=mpl.colors.Normalize(vmin=s.min(), vmax=vmax), cmap="magma")
        colour = (mapper.to_rgba(s)[:, :, :3] * 255).astype(np.uint8)
        assert s.dtype == np.float32 and vmax.dtype == np.float32
        out[name + "/disp"] = disp.numpy()
        out[name + "/size"] = np.array([H0, W0], np.int32)
        out[name + "/s"] = s
        out[name + "/vmin"] = np.float32(s.min())
        out[name + "/vmax"] = np.float32(vmax)
        out[name + "/colour"] = colour
        print(name, s.shape, float(s.min()), float(vmax), "share at max %.3f" % float((s == s.max()).mean()))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT) // 1024, "KB")


if __name__ == "__main__":
    main()
