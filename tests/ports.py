"""Build + bind the host ports (tests/host_port/*.cpp): g++ builds of the kernels' own arithmetic (csrc/*_math.h).

Test infrastructure only.  Every `hp_<name>` with a twin `bbd_<name>` in include/bbd_hip.h is typed from that prototype
minus the stream (`baseboostdepth_amd/_abi.py`), so a call is marshalled through a port exactly as through `HipLibrary`.
`PortBackend` plugs into the `backend=` seam of the product, so the CPU tier runs the
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
    """`lib.<name>(...)` is `hp_<name>` of the port library, for the host-side helpers of the ABI (no `stream`)."""

    def __init__(self, dll):
        self._dll = dll

    def __getattr__(self, name):
        from baseboostdepth_amd._lib import PROTOTYPES
        proto = PROTOTYPES.get("bbd_" + name)
        if proto is None or proto.has_stream:
            raise AttributeError("%s is no host-side helper of include/bbd_hip.h" % name)
        return getattr(self._dll, "hp_" + name)


class PortBackend:
    name = "host-port"

    def __init__(self):
        from baseboostdepth_amd._lib import PROTOTYPES
        self.dll = ctypes.CDLL(build())
        # a port marshals like the product: hp_<name> takes what include/bbd_hip.h declares for bbd_<name>, minus the stream
        for name, proto in PROTOTYPES.items():
            fn = getattr(self.dll, "hp_" + name[len("bbd_"):], None)
            if fn is not None:
                fn.argtypes = [ctype for ctype, _ in proto.params[:len(proto.params) - proto.has_stream]]
                fn.restype = proto.restype
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
        `name` (bbd_*), typed by the header like the library's own call."""
        return getattr(self.dll, name.replace("bbd_", "hp_"))(*args)

    def run(self, name, anchor, *args):
        from baseboostdepth_amd._lib import BbdError
        self.calls.append(name)
        rc = self.status(name, *args)
        if rc != 0:
            raise BbdError("%s failed with status %d" % (name, rc))
