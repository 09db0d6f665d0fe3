"""In-tree build of the C-ABI library: hipcc for gfx950, nothing else.

    python -m baseboostdepth_amd.csrc.build

The .so is git-ignored (history stays source-only) but travels to the GPU box with the tree.
-ffp-contract=off is REQUIRED: bbd_math.h mirrors the reference CPU path's rounding order and
places every FMA explicitly.
"""
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def _here(names):
    return [os.path.join(HERE, n) for n in names.split()]


SRCS = _here("""
    bbd_kernels.hip
    bbd_eval.hip
    bbd_image.hip
    bbd_nn.hip
    bbd_vit.hip
    bbd_pose.hip
    bbd_tokens.hip
    bbd_util.hip
    bbd_viz.hip
    bbd_velo.hip
    bbd_syns.hip
    bbd_odom.hip
    bbd_traj.hip
    bbd_postproc.hip
    bbd_panel.hip
    bbd_compare.hip
    bbd_cloud.hip
    bbd_ground.hip
    bbd_map.hip
    bbd_view.hip
    bbd_consist.hip
    bbd_geo.hip
    bbd_uncert.hip
    bbd_wgrad.hip
    bbd_up2conv.hip
    bbd_sgm.hip
    bbd_align.hip
    bbd_stemconv.hip
    bbd_conv1x1.hip
""")
OUT = os.path.join(HERE, "libbbd_hip.so")
# every header of this directory: one that is forgotten here would leave a stale library behind an edit
DEPS = SRCS + [os.path.abspath(__file__)] + sorted(glob.glob(os.path.join(HERE, "*.h"))) + [
    os.path.join(HERE, "..", "..", "include", "bbd_hip.h"), os.path.join(HERE, "..", "..", "include", "bbd_wgrad.h"),
    os.path.join(HERE, "..", "..", "include", "bbd_up2conv.h"), os.path.join(HERE, "..", "..", "include", "bbd_sgm.h"),
    os.path.join(HERE, "..", "..", "include", "bbd_stemconv.h"), os.path.join(HERE, "..", "..", "include", "bbd_conv1x1.h")]
# -fno-slp-vectorize: hipcc otherwise SLP-packs neighbouring scalar fp32 adds / multiplies into v_pk_add/mul_f32 and
# pays for it in v_mov register shuffles (129 moves in the forward's SSIM phase): measured forward 0.222 -> 0.208 ms,
# identity 0.0365 -> 0.0340 ms, backward 0.348 -> 0.343 ms (profiles/r02/slp_variants.txt).  Same operations, same bits.
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize", "-fPIC", "-shared",
         "-std=c++17"]


def source_sha16():
    """First 16 hex digits of sha256 over the fused kernels' sources (bbd_kernels.hip + bbd_math.h): stamped into the
    committed counter / instruction-mix files (tools/pmc_summary.py, tools/isa_mix.py) so that bench.py can say when the
    constants it quotes from them were taken from other code than the one it is timing."""
    import hashlib
    h = hashlib.sha256()
    for name in ("bbd_kernels.hip", "bbd_math.h"):
        with open(os.path.join(HERE, name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def build(force=False, verbose=False):
    if not force and os.path.isfile(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in DEPS):
        return OUT
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + FLAGS + ["-o", OUT] + SRCS
    if verbose:
        cmd.append("-Rpass-analysis=kernel-resource-usage")
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose="-v" in sys.argv))
