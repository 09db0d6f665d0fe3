"""Command-line options with the reference's flag names and defaults (options.py:11-258) for the part
of the system this build covers.  Flags that select other model zoos / datasets of the reference are
accepted so existing command lines still parse, and rejected with a clear message when set."""
import argparse
import os

_HERE = os.path.dirname(os.path.abspath(__file__))

# (flag, kwargs)
_FLAGS = [
    # paths
    ("--data_path", dict(type=str, default="data/KITTI_RAW")),
    ("--kt_path", dict(type=str, default=os.path.join(os.path.dirname(_HERE), "kitti_data"))),
    ("--log_dir", dict(type=str, default=os.path.join(os.path.dirname(_HERE), "paper"))),
    ("--training_file", dict(type=str, default="train_files_baselines")),
    ("--splits_dir", dict(type=str, default=os.path.join(os.path.dirname(_HERE), "splits"))),
    # BaseBoostDepth switches
    ("--rand", dict(action="store_true")), ("--trimin", dict(action="store_true")),
    ("--decomp", dict(action="store_true")), ("--partial_skip", dict(action="store_true")),
    ("--incremental_skip", dict(action="store_true")), ("--pose_error", dict(type=float, default=1)),
    ("--naive_mix", dict(action="store_true")), ("--kt", dict(action="store_true")),
    # model / loss
    ("--model_name", dict(type=str, default="mdp")), ("--num_layers", dict(type=int, default=18, choices=[18, 34, 50, 101, 152])),
    ("--height", dict(type=int, default=192)), ("--width", dict(type=int, default=640)),
    ("--disparity_smoothness", dict(type=float, default=1e-3)), ("--scales", dict(nargs="+", type=int, default=[0, 1, 2, 3])),
    ("--min_depth", dict(type=float, default=0.1)), ("--max_depth", dict(type=float, default=100.0)),
    ("--frame_ids", dict(nargs="+", type=int, default=[0, -1, 1])), ("--no_ssim", dict(action="store_true")),
    ("--weights_init", dict(type=str, default="pretrained", choices=["pretrained", "scratch"])),
    # optimisation
    ("--batch_size", dict(type=int, default=12)), ("--learning_rate", dict(type=float, default=1e-4)),
    ("--num_epochs", dict(type=int, default=20)), ("--pytorch_random_seed", dict(type=int, default=42)),
    # system
    ("--cuda", dict(type=int, default=0)), ("--no_cuda", dict(action="store_true")),
    ("--num_workers", dict(type=int, default=12)),
    # loading / logging
    ("--load_weights_folder", dict(type=str, default="None")),
    ("--models_to_load", dict(nargs="+", type=str, default=["encoder", "depth", "pose_encoder", "pose"])),
    ("--log_frequency", dict(type=int, default=250)), ("--save_frequency", dict(type=int, default=1)),
    # evaluation
    ("--eval_stereo", dict(action="store_true")), ("--eval_mono", dict(action="store_true")),
    ("--disable_median_scaling", dict(action="store_true")), ("--pred_depth_scale_factor", dict(type=float, default=1)),
    ("--eval_split", dict(type=str, default="eigen")), ("--save_pred_disps", dict(action="store_true")),
    ("--post_process", dict(action="store_true")),
    # score a saved disps_<split>_split.npy instead of predictions / stop after predicting (and saving)
    ("--ext_disp_to_eval", dict(type=str, default=None)), ("--no_eval", dict(action="store_true")),
    # this build
    # MonoViT (BASELINE configs[4]): MPViT-small encoder + HR decoder, AdamW with two LR groups
    ("--ViT", dict(action="store_true")), ("--mpvit_checkpoint", dict(type=str, default="./ckpt/mpvit_small.pth")),
    ("--materialize_warps", dict(action="store_true")), ("--synthetic", dict(action="store_true")),
    ("--step_graph", dict(action="store_true")), ("--loader_workers", dict(type=str, default="process", choices=["process", "thread"])),
    # the step's pose-network calls as one batched pass with per-call BatchNorm statistics (default) or one by one
    ("--separate_pose_calls", dict(dest="batched_pose", action="store_false")),
    # --rand recipes run the step in pooled form (pooled.py: one frame pool, static step tables, one step graph per pose-row
    # bucket, captured by Trainer.prewarm() at the start of every epoch) and replay step graphs by default
    ("--per_signature_step", dict(dest="pooled_step", action="store_false", default=None)),
    ("--no_prewarm", dict(dest="prewarm", action="store_false")),
    ("--no_step_graph", dict(action="store_true")),
    # early curriculum: 0 = pad the pose pass to the next measured row count (32 | 48 for batch 12); "max" or a number = ONE
    # row count for the whole phase (one graph; the pass then always runs the phase's largest size)
    ("--early_pose_rows", dict(type=str, default="0")),
    # the training log at every --log_frequency-th step (trainlog.py): off | text = progress lines on stdout + scalars.jsonl |
    # panels = text + pictures rendered on the device (target, disparity, minimum-loss map, arg-min map, the warps)
    ("--train_log", dict(type=str, default="off", choices=["off", "text", "panels"])),
    ("--log_samples", dict(type=int, default=1)),
    # SC-SfMLearner's geometry-consistency term (Bian et al., NeurIPS 2019): the weight of the loss that makes
    # the depth of a frame and the depth of its temporal neighbours agree under the predicted motion.  0 = off: the step is
    # the step it was.  Nothing has been trained with it here: no value is recommended
    ("--geometry_consistency", dict(type=float, default=0.0, metavar="W")),
    # Depth Hints (Watson et al., ICCV 2019): the weight of the log-L1 term that pulls the depth towards a
    # proxy depth from semi-global stereo matching, computed on the device inside the step, wherever the proxy reprojects
    # better than the step's own minimum loss; --hint_disparities is the matcher's search range (64, 128, 192 or 256).
    # 0 = off: the step is the step it was.  Nothing has been trained with it here: no value is recommended
    ("--depth_hints", dict(type=float, default=0.0, metavar="W")), ("--hint_disparities", dict(type=int, default=128)),
    # evaluate_depth.py: write the clouds of the first --cloud_count images of the split, prediction and ground truth, as
    # <index>_pred.ply / <index>_gt.ply into this directory while the batch is in HBM
    ("--save_clouds", dict(type=str, default=None, metavar="DIR")), ("--cloud_count", dict(type=int, default=8)),
    ("--cloud_stride", dict(type=int, default=1)),
    ("--cloud_rays", dict(type=str, default="pixel", choices=["pixel", "reference"])),
    # evaluate_depth.py: where the scale of a mono prediction comes from - the LiDAR median of every image (the
    # reference), or the camera's height above the pixels found to be road, without ground truth, or - for
    # the relative-depth models, whose disparity is known up to a scale AND a shift - the least-squares fit of every
    # image to its inverse ground truth (lsq), which also prints SILog and iRMSE
    ("--scale_recovery", dict(type=str, default="median", choices=["median", "ground", "lsq"])),
    ("--camera_height", dict(type=float, default=1.65)), ("--ground_angle", dict(type=float, default=5.0)),
    # evaluate_depth.py: a ground-truth-free uncertainty map of every prediction, judged by sparsification (AUSE / AURG,
    # DESIGN.md 6n).  post = |d - flip(d')| of the flip pass (implies --post_process); --ext_uncert_to_eval supplies the
    # maps of --ext_disp_to_eval instead
    ("--uncertainty", dict(type=str, default="none", choices=["none", "post"])),
    ("--ext_uncert_to_eval", dict(type=str, default=None, metavar="FILE.npy")),
    ("--save_pred_uncerts", dict(action="store_true")),
    ("--sparsification_intervals", dict(type=int, default=50)),
    ("--save_sparsification", dict(type=str, default=None, metavar="FILE.json")),
]
# other zoos / datasets of the reference: parsed, refused when set
_OUT_OF_SCOPE = ["--SYNS_eval", "--SQL", "--SQL_L", "--CA_depth", "--DIFFNet", "--stereo_guide",
                 "--x_min", "--png", "--use_stereo", "--eval_eigen_to_benchmark"]


SPARSIFICATION_MAX_INTERVALS = 100      # BBD_SPARS_MAX_INTERVALS of include/bbd_hip.h


def uncertainty_conflict(opt):
    """What the uncertainty options of `opt` collide with, as one sentence, or None.  Every field is read with its
    default, so an `opt` without them has no conflict.  `options.parse` and `evaluation.evaluate` both refuse with it."""
    get = lambda name, default: getattr(opt, name, default)      # noqa: E731
    mode, ext_uncert = get("uncertainty", "none"), get("ext_uncert_to_eval", None)
    if mode not in ("none", "post"):
        return "uncertainty is none or post, got %r" % (mode,)
    on = mode == "post" or ext_uncert is not None
    if not on:
        for name in ("save_pred_uncerts", "save_sparsification"):
            if get(name, None):
                return "%s needs an uncertainty: uncertainty post or ext_uncert_to_eval" % name
        return None
    if ext_uncert is not None and mode == "post":
        return "ext_uncert_to_eval supplies the uncertainty maps and uncertainty post computes them: choose one"
    if ext_uncert is not None and get("ext_disp_to_eval", None) is None:
        return "ext_uncert_to_eval holds the uncertainties of the disparities of ext_disp_to_eval, which is not set"
    if mode == "post" and get("ext_disp_to_eval", None) is not None:
        return ("uncertainty post comes from the flip pass of the networks, and ext_disp_to_eval runs none: give the maps "
                "with ext_uncert_to_eval")
    if ext_uncert is not None and get("save_pred_uncerts", False):
        return "save_pred_uncerts saves predicted uncertainties, and ext_uncert_to_eval predicts none"
    for name, set_ in (("eval_split SYNS", get("eval_split", "eigen") == "SYNS"), ("no_eval", bool(get("no_eval", False))),
                       ("scale_recovery ground", get("scale_recovery", "median") == "ground")):
        if set_:
            return ("an uncertainty map is judged on the pixels and with the scale of the KITTI metrics rows: it "
                    "excludes %s" % name)
    K = get("sparsification_intervals", 50)
    if not isinstance(K, int) or not 1 <= K <= SPARSIFICATION_MAX_INTERVALS:
        return "sparsification_intervals must be 1 ... %d, got %r" % (SPARSIFICATION_MAX_INTERVALS, K)
    return None


def alignment_conflict(opt):
    """What `scale_recovery lsq` collides with in `opt`, as one sentence, or None.  Every field is read with its default,
    so an `opt` without them has no conflict.  `options.parse` and `evaluation.evaluate` both refuse with it."""
    get = lambda name, default: getattr(opt, name, default)      # noqa: E731
    if get("scale_recovery", "median") != "lsq":
        return None
    for name in ("eval_stereo", "disable_median_scaling"):
        if get(name, False):
            return ("--scale_recovery lsq fits the scale and the shift of every image to its ground truth: the alignment "
                    "is the scaling, so it excludes --%s" % name)
    if get("pred_depth_scale_factor", 1) != 1:
        return ("--scale_recovery lsq fits the scale of every image itself: a --pred_depth_scale_factor other than 1 "
                "would be fitted away")
    for name, set_ in (("--eval_split SYNS", get("eval_split", "eigen") == "SYNS"),
                       ("--save_clouds", get("save_clouds", None) is not None),
                       ("--uncertainty", get("uncertainty", "none") != "none"),
                       ("--ext_uncert_to_eval", get("ext_uncert_to_eval", None) is not None)):
        if set_:
            return ("--scale_recovery lsq excludes %s: its kernels read the median ratio of a bbd_depth_metrics row and "
                    "know no shift" % name)
    return None


def geometry_consistency_conflict(opt):
    """One sentence on why the geometry-consistency weight cannot be honoured, or None."""
    W = getattr(opt, "geometry_consistency", 0.0)
    if not W >= 0.0:
        return "--geometry_consistency is the weight of a loss term and must not be negative, got %r" % (W,)
    if W > 0.0 and (getattr(opt, "rand", False) or getattr(opt, "trimin", False)):
        return ("--geometry_consistency needs one frame set for the whole batch: with --rand or --trimin the frame sets vary "
                "per sample and the step runs in pooled form, where the term is not routed")
    return None


def depth_hints_conflict(opt):
    """One sentence on why the depth-hint weight cannot be honoured, or None."""
    W = getattr(opt, "depth_hints", 0.0)
    if not W >= 0.0:
        return "--depth_hints is the weight of a loss term and must not be negative, got %r" % (W,)
    D = getattr(opt, "hint_disparities", 128)
    if D not in (64, 128, 192, 256):
        return "--hint_disparities must be 64, 128, 192 or 256, got %r" % (D,)
    if W > 0.0 and (getattr(opt, "rand", False) or getattr(opt, "trimin", False)):
        return ("--depth_hints needs the stereo partner of every sample of the batch: with --rand or --trimin the frame sets "
                "vary per sample and the step runs in pooled form, where the term is not routed")
    if W > 0.0 and getattr(opt, "ViT", False):
        return "--depth_hints is not routed through the --ViT step"
    return None


class MonodepthOptions:
    def __init__(self):
        self.parser = argparse.ArgumentParser(description="BaseBoostDepth options (MI355X build)")
        for flag, kw in _FLAGS:
            self.parser.add_argument(flag, **kw)
        for flag in _OUT_OF_SCOPE:
            self.parser.add_argument(flag, action="store_true", help="not part of this build")
        self.parser.add_argument("--debug", action="store_true")
        self.parser.add_argument("--chamfer", action="store_true",
                                 help="with --eval_split SYNS: also the point-cloud F-score and IoU")
        self.parser.add_argument("--syns_path", type=str, default="data/KITTI_RAW")
        self.parser.add_argument("--x_val", type=int, default=3)
        # evaluate_pose.py (--eval_split odom_<n>): the KITTI odometry tree (default: `odom` next to --kt_path, where the
        # reference's loader looks), and the two constants the reference hard-codes
        self.parser.add_argument("--odom_path", type=str, default=None,
                                 help="KITTI odometry root (sequences/, poses/); default dirname(kt_path)/odom")
        self.parser.add_argument("--skip_frame", type=int, default=2)
        self.parser.add_argument("--track_length", type=int, default=1)
        # the scores of the KITTI odometry tables: the whole trajectory chained from the single steps
        self.parser.add_argument("--trajectory", action="store_true",
                                 help="also print t_rel (%%), r_rel (deg/100m) and the ATE of the aligned full trajectory")
        self.parser.add_argument("--trajectory_align", type=str, default="sim3", choices=["sim3", "se3", "scale", "none"],
                                 help="alignment of the predicted trajectory to ground truth before it is scored")
        self.parser.add_argument("--save_trajectory", type=str, default=None,
                                 help="with --trajectory: write the aligned poses to this file, 12 numbers per row")
        # the scene map of the sequence: depth predictions placed by the aligned trajectory, fused on a voxel grid
        # (DESIGN.md 6j); the depth limits are in the units of the aligned trajectory (metres under sim3)
        self.parser.add_argument("--save_map", type=str, default=None, metavar="FILE.ply",
                                 help="with --trajectory: write the voxel-fused coloured point cloud of the sequence")
        self.parser.add_argument("--map_voxel", type=float, default=0.2, help="edge of a voxel")
        self.parser.add_argument("--map_every", type=int, default=1, help="use every k-th frame")
        self.parser.add_argument("--map_stride", type=int, default=2, help="use every k-th pixel of a frame, both ways")
        self.parser.add_argument("--map_min_depth", type=float, default=0.5)
        self.parser.add_argument("--map_max_depth", type=float, default=30.0)
        self.parser.add_argument("--map_min_points", type=int, default=1, help="drop voxels with fewer points")
        self.parser.add_argument("--map_capacity", type=int, default=1 << 24,
                                 help="slots of the voxel table (rounded up to a power of two, 48 bytes each)")
        # depth-pose geometric consistency: the depth of a frame against the depth of its neighbours under the predicted
        # motion.  The default threshold is a knob, not a finding: neither the score nor the filter has been
        # measured on real KITTI predictions
        self.parser.add_argument("--consistency", action="store_true",
                                 help="with --trajectory: also print the mean depth-pose consistency error of the "
                                      "sequence and the shares of samples that agree (--map_every is honoured)")
        self.parser.add_argument("--consistency_views", type=int, default=1,
                                 help="check every frame against its k neighbours on either side")
        self.parser.add_argument("--consistency_threshold", type=float, default=0.05,
                                 help="a sample agrees when |z - d| / (z + d) is below this (not calibrated)")
        self.parser.add_argument("--consistency_min_views", type=int, default=1,
                                 help="a pixel is kept when it agrees in at least this many neighbours")
        self.parser.add_argument("--map_consistent", action="store_true",
                                 help="with --save_map: fuse only the pixels the consistency check keeps")
        # the bird's-eye plot of the run: both trajectories over the scene map, drawn on the device
        self.parser.add_argument("--save_plot", type=str, default=None, metavar="FILE.png",
                                 help="with --trajectory: write a picture of the ground-truth and the aligned predicted "
                                      "trajectory seen from above, over the scene map where --save_map is given")
        self.parser.add_argument("--plot_view", type=str, default="top", choices=["top", "side"])
        self.parser.add_argument("--plot_size", type=int, default=1024, help="the picture is this many pixels square")
        self.parser.add_argument("--plot_ceiling", type=float, default=3.0,
                                 help="top view: voxels more than this far above the highest camera are left out")
        self.parser.add_argument("--plot_point_size", type=int, default=1, choices=[1, 3, 5, 7],
                                 help="side of a voxel's square in pixels")

    def parse(self, argv=None):
        self.options = self.parser.parse_args(argv)
        bad = [f for f in _OUT_OF_SCOPE if getattr(self.options, f[2:])]
        if bad:
            self.parser.error("%s select parts of the reference that are outside this build's scope" % ", ".join(bad))
        if self.options.save_clouds is not None:
            if self.options.no_eval:
                self.parser.error("--save_clouds needs the evaluation: the clouds are scaled by the median-scaling ratio "
                                  "of each image's metrics row, and --no_eval produces no metrics rows")
            if self.options.cloud_count < 1 or self.options.cloud_stride < 1:
                self.parser.error("--cloud_count and --cloud_stride must be at least 1")
        if self.options.scale_recovery == "ground":
            for flag, set_ in (("--eval_stereo", self.options.eval_stereo),
                               ("--disable_median_scaling", self.options.disable_median_scaling),
                               ("--eval_split SYNS", self.options.eval_split == "SYNS")):
                if set_:
                    self.parser.error("--scale_recovery ground scales a mono prediction on a KITTI split by the camera's "
                                      "height above the road: it excludes %s" % flag)
            if not self.options.camera_height > 0 or not 0.0 <= self.options.ground_angle < 90.0:
                self.parser.error("--camera_height must be positive and --ground_angle lie in [0, 90) degrees")
        conflict = alignment_conflict(self.options)
        if conflict:
            self.parser.error(conflict)
        conflict = uncertainty_conflict(self.options)
        if conflict:
            self.parser.error(conflict)
        conflict = geometry_consistency_conflict(self.options)
        if conflict:
            self.parser.error(conflict)
        conflict = depth_hints_conflict(self.options)
        if conflict:
            self.parser.error(conflict)
        if self.options.rand and not self.options.no_step_graph:
            self.options.step_graph = True
        if self.options.early_pose_rows != "max":
            self.options.early_pose_rows = int(self.options.early_pose_rows)
        return self.options
