"""GPU tier of the Velodyne depth maps: bbd_velo_depth through `ops.velo_depth`, `kitti_utils.generate_depth_maps`,
the root export_gt_depth.py as a child process, and `evaluation.evaluate` without a gt_depths.npz.  Acceptance rules:
tests/velo_checks.py (vel_depth=True bit-equal to the reference; vel_depth=False same non-zero pixels, 1 float32 ulp).
Child processes run under `timeout`; the in-process tests are bounded by the suite's own."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import velo_checks as vc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EVERY = [(c, cam) for c in vc.CASES for cam in vc.CAMS]


@pytest.fixture(scope="module")
def v():
    return vc.load()


@pytest.mark.parametrize("vel_depth", [True, False])
def test_one_ragged_launch_matches_the_reference(v, vel_depth):
    """Every case and both cameras in ONE call; identical calls give identical bytes; single calls give the same bits."""
    from baseboostdepth_amd import ops
    maps, buf = vc.run_batch(v, EVERY, vel_depth, ops.default_backend(), DEV)
    _, again = vc.run_batch(v, EVERY, vel_depth, ops.default_backend(), DEV)
    assert torch.equal(buf.view(torch.int32), again.view(torch.int32))
    for (case, cam), got in zip(EVERY, maps):
        vc.check_map(got, vc.golden_map(v, case, cam, vel_depth), vel_depth, "%s cam %d" % (case, cam))
    for member in [("scan_a", 3), ("crafted", 2), ("empty", 2)]:
        (one,), _ = vc.run_batch(v, [member], vel_depth, ops.default_backend(), DEV)
        assert np.array_equal(vc.bits(one), vc.bits(maps[EVERY.index(member)]))


def test_device_equals_the_host_port_bit_for_bit(v):
    """Same header, same operation order: also where the reference is only matched to an ulp."""
    from ports import PortBackend
    from baseboostdepth_amd import ops
    for vel_depth in (True, False):
        dev_maps, _ = vc.run_batch(v, EVERY, vel_depth, ops.default_backend(), DEV)
        host_maps, _ = vc.run_batch(v, EVERY, vel_depth, PortBackend(), "cpu")
        for a, b in zip(dev_maps, host_maps):
            assert np.array_equal(vc.bits(a), vc.bits(b))


def test_output_offsets_are_honoured_and_every_pixel_is_written(v):
    from baseboostdepth_amd import ops
    members = [("scan_b", 2), ("crafted", 3)]
    sizes = [h * w for h, w in (vc.size(v, c) for c, _ in members)]
    out = torch.full((sum(sizes) + 7,), float("nan"), device=DEV)
    maps, buf = vc.run_batch(v, members, True, ops.default_backend(), DEV, out=out, offsets=[sizes[1] + 7, 0])
    assert buf is out and int(torch.isnan(out).sum()) == 7 and bool(torch.isnan(out[sizes[1]:sizes[1] + 7]).all())
    for (case, cam), got in zip(members, maps):
        vc.check_map(got, vc.golden_map(v, case, cam, True), True)


def _golden_tree(v, root):
    frames = [("2011_09_26", 0, vc.scan(v, "scan_a")), ("2011_09_30", 3, vc.scan(v, "scan_b")),
              ("2011_09_26", 5, vc.scan(v, "crafted")), ("2011_09_30", 4, vc.scan(v, "empty"))]
    return vc.write_tree(v, root, frames), ["scan_a", "scan_b", "crafted", "empty"]


def test_generate_depth_maps_is_the_ground_truth_set_of_the_golden_maps(v, tmp_path):
    from baseboostdepth_amd import kitti_utils
    from baseboostdepth_amd.evaluation import GroundTruthSet
    root = str(tmp_path)
    lines, cases = _golden_tree(v, root)
    vc.write_split(root, "eigen", lines)
    frames = kitti_utils.split_frames(os.path.join(root, "eigen"), "eigen", root)
    want = GroundTruthSet([vc.golden_map(v, c, 2, True) for c in cases], DEV)
    for batch_frames in (32, 3):
        gts = kitti_utils.generate_depth_maps(frames, DEV, vel_depth=True, batch_frames=batch_frames)
        assert isinstance(gts, GroundTruthSet) and gts.buffer.is_cuda and gts.shapes == want.shapes
        assert torch.equal(gts.desc, want.desc)
        assert torch.equal(gts.buffer.view(torch.int32), want.buffer.view(torch.int32))
    one = kitti_utils.generate_depth_map(frames[1][0], frames[1][1], cam=3, vel_depth=False)
    vc.check_map(one, vc.golden_map(v, "scan_b", 3, False), False, "generate_depth_map")


def test_export_command_line_as_a_child_process(v, tmp_path):
    root, splits = str(tmp_path / "kitti"), str(tmp_path / "splits")
    lines, cases = _golden_tree(v, root)
    vc.write_split(splits, "eigen", lines)
    vc.write_split(splits, "eigen_zhou", lines[::2])             # both 375 x 1242: the homogeneous form
    base = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "export_gt_depth.py"), "--data_path", root,
            "--splits_dir", splits]
    for split, names in (("eigen", cases), ("eigen_zhou", cases[::2])):
        r = subprocess.run(base + ["--split", split], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        data = np.load(os.path.join(splits, split, "gt_depths.npz"), allow_pickle=True)["data"]
        assert (data.dtype == object) == (split == "eigen") and len(data) == len(names)
        for got, c in zip(data, names):
            vc.check_map(got, vc.golden_map(v, c, 2, True), True, c)
    r = subprocess.run(base + ["--split", "SYNS"], capture_output=True, text=True)
    assert r.returncode == 2 and "scope" in r.stderr


def test_evaluate_without_the_npz_equals_evaluate_with_the_exported_npz(v, tmp_path, capsys):
    """The split has no gt_depths.npz: evaluate() projects the scans itself.  Then export_gt_depth.py writes the file
    and evaluate() reads it: the same seven errors and the same ratios."""
    import image_checks
    from baseboostdepth_amd import datasets, evaluation, networks
    H, W = 96, 320
    root, splits = str(tmp_path / "kitti"), str(tmp_path / "splits")
    lines = [l.rsplit(" ", 2)[0] for l in image_checks.make_kitti_tree(root, frames=20)][::2]
    assert len(lines) == 8 and len(set(l.split()[0] for l in lines)) == 2            # both drives: ragged sizes
    clouds = {"2011_09_26": vc.scan(v, "scan_a"), "2011_09_30": vc.scan(v, "scan_b")}
    frames = []
    for k, l in enumerate(lines):
        folder, t, _ = l.split()
        frames.append((folder.split("/")[0], int(t), clouds[folder.split("/")[0]][k % 3::2]))     # a different scan per frame
    vc.write_tree(v, root, frames)
    split_dir = vc.write_split(splits, "eigen", lines)
    torch.manual_seed(5)
    encoder = networks.ResnetEncoder(18, False)
    models = (encoder, networks.DepthDecoder(encoder.num_ch_enc))
    opt = types.SimpleNamespace(eval_mono=True, eval_stereo=False, cuda=0, kt_path=root, splits_dir=splits, eval_split="eigen",
                                disable_median_scaling=False, pred_depth_scale_factor=1, min_depth=0.1, max_depth=100.0,
                                height=H, width=W)

    def loader():
        ds = datasets.KITTIRAWDataset(lines, 0, H, W, kt_path=root, is_train=False, kt=True, naive_mix=True)
        return datasets.DeviceLoader(ds, 3, datasets.DeviceCollate(H, W, [0], DEV), shuffle=False, drop_last=False,
                                     num_workers=2)

    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True          # same convolution sums in both runs (see DepthPredictor.disparity)
    try:
        assert not os.path.exists(os.path.join(split_dir, "gt_depths.npz"))
        errors, ratios = evaluation.evaluate(opt, dataloader=loader(), models=models)
        said = capsys.readouterr().out
        assert "gt_depths.npz not found" in said and "8 frames" in said
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "export_gt_depth.py"),
                            "--data_path", root, "--splits_dir", splits, "--split", "eigen"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert os.path.isfile(os.path.join(split_dir, "gt_depths.npz"))
        errors_npz, ratios_npz = evaluation.evaluate(opt, dataloader=loader(), models=models)
        assert "not found" not in capsys.readouterr().out
    finally:
        torch.backends.cudnn.deterministic = was
    print("errors", errors, "ratios", ratios)
    assert np.isfinite(errors).all() and ratios.shape == (8,) and np.isfinite(ratios).all()
    assert np.array_equal(errors, errors_npz) and np.array_equal(ratios, ratios_npz)
