"""Build + bind the host ports (tests/host_port/*.cpp): g++ builds of the kernels' own arithmetic (csrc/*_math.h).

Test infrastructure only.  `PortBackend` plugs into the `backend=` seam of the product, so the CPU tier runs the
product's Python plumbing (plans, descriptor tables, scratch sizing, checks, autograd wrappers) with the exact
arithmetic of the HIP kernels.  All ports live in ONE library, so a flow that crosses features needs no routing:

  port source     seam it serves
  host, image     ops.* of the fused hot path, `datasets.DeviceCollate`, a whole `Trainer` step
  viz             ops.disp_viz
  velo            ops.velo_depth, kitti_utils.generate_depth_maps
  syns            evaluation.pred_edges / distance_transform / edge_metrics / pointcloud_metrics, ops.chamfer_nn
  odom, traj      evaluation.pose_ate / pose_trajectory / evaluate_pose (with stand-ins for gather_pairs, pose_matrix_fwd)
  postproc        ops.post_process_disp
  panel           ops.train_panel / argmin_hist
  compare         ops.gt_viz / error_map, evaluation.depth_metrics, compare.compare_batch
  cloud           ops.point_cloud, evaluation.evaluate(..., save_clouds=)
  map, view       ops.map_* / view_*, pointcloud.SceneMap / Canvas, evaluate_pose(..., save_map=, save_plot=)
"""
import ctypes
import glob
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
PORTS = os.path.join(HERE, "host_port")
LIB_PATH = os.path.join(PORTS, "libbbd_ports.so")


def build():
    """tests/host_port/libbbd_ports.so from every tests/host_port/*.cpp, rebuilt when a source or a header is newer."""
    srcs = sorted(glob.glob(os.path.join(PORTS, "*.cpp")))
    deps = srcs + glob.glob(os.path.join(HERE, "..", "baseboostdepth_amd", "csrc", "*.h")) \
        + [os.path.join(HERE, "..", "include", "bbd_hip.h")]
    if os.path.isfile(LIB_PATH) and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(d) for d in deps):
        return LIB_PATH
    tmp = "%s.%d.tmp" % (LIB_PATH, os.getpid())     # a concurrent test process never loads a half-written library
    cmd = ["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-std=c++17", "-o", tmp] + srcs
    try:
        subprocess.run(cmd, check=True)
        os.replace(tmp, LIB_PATH)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return LIB_PATH


class PortLibrary:
    """`lib.<name>(ints...)` is `hp_<name>` of the port library: the size helpers of the ABI, typed by `HipLibrary`'s rule."""

    def __init__(self, dll):
        self._dll = dll

    def __getattr__(self, name):
        fn = getattr(self._dll, "hp_" + name)
        fn.restype = ctypes.c_long if name.endswith(("_scratch_floats", "_state_bytes")) else ctypes.c_int
        return lambda *ints: fn(*[ctypes.c_int(v) for v in ints])


class PortBackend:
    name = "host-port"

    def __init__(self):
        self.dll = ctypes.CDLL(build())
        self.lib = PortLibrary(self.dll)
        self.calls = []

    def num_tiles(self, H, W):
        return 1

    def num_tiles_fwd(self, H, W):
        return 1

    def num_tiles_bwd(self, H, W):
        return 1

    def smooth_chunks(self):
        return 1

    def fused_work_items(self, plan, S, H, W, backward, device):
        return None       # the work-item table is a launch-order choice of the GPU kernels

    @staticmethod
    def _check(*tensors):
        for t in tensors:
            assert t is None or not t.is_cuda

    def status(self, name, *args):
        """The return code (0 = done, < 0 = the ABI's argument errors) of the port's twin (hp_*) of the ABI function
        `name` (bbd_*): Python floats travel as doubles, ints as C ints, everything else (ctypes pointers) as it is."""
        fn = getattr(self.dll, name.replace("bbd_", "hp_"))
        fn.restype = ctypes.c_int
        return fn(*[ctypes.c_double(a) if isinstance(a, float) else ctypes.c_int(a) if isinstance(a, int) else a
                    for a in args])

    def run(self, name, anchor, *args):
        from baseboostdepth_amd._lib import BbdError
        self.calls.append(name)
        rc = self.status(name, *args)
        if rc != 0:
            raise BbdError("%s failed with status %d" % (name, rc))
