"""CPU tier of the ground-plane scale recovery: the host port of `bbd_ground_scale` (tests/host_port/bbd_ground_port.cpp,
the kernels' own arithmetic) against the numpy float32 reference (tests/ground_ref.py) bit for bit, the accuracy of the
recovered scale on synthetic roads, `pointcloud.intrinsics_at`, the argument rules on both sides of the ABI."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ground_checks  # noqa: E402
import ground_ref  # noqa: E402
from baseboostdepth_amd import _lib, ops, pointcloud  # noqa: E402


@pytest.fixture(scope="module")
def port():
    from ports import PortBackend
    return PortBackend()


@pytest.mark.parametrize("number", ground_checks.CASES)
def test_port_equals_the_reference_bit_for_bit(port, number):
    calls, refs = ground_checks.case(number)
    for call, (want_rows, want_mask) in zip(calls, refs):
        rows, mask = ground_checks.run(call, port, "cpu")
        assert ground_checks.same_bytes(mask, want_mask)
        assert ground_checks.same_bytes(rows, want_rows), (rows, want_rows)


SIZES = [(19, 67), (33, 130), (192, 640)]


@pytest.mark.parametrize("h,w", SIZES)
def test_recovered_scale_on_synthetic_roads(port, h, w):
    """Noise-free scenes give the scale back within 1e-5 relative (ten times the 8.4e-7 the specification's prototype
    measured), scenes with 0.2 % multiplicative depth noise within 2e-2 (measured there: 5.1e-3); between 0.18 and
    0.41 of the candidates are ground."""
    combos = [(p, s) for p in (0.0, 2.0, -3.0) for s in (1.0, 7.3)]
    for noise, bound in ((0.0, 1e-5), (0.002, 2e-2)):
        depth = np.stack([ground_ref.scene(h, w, pitch_deg=p, scale=s, noise=noise, seed=k)
                          for k, (p, s) in enumerate(combos)])
        rows, _ = ops.ground_scale(torch.from_numpy(depth), pointcloud.intrinsics(h, w), backend=port)
        rows = rows.numpy().astype(np.float64)
        for (p, s), row in zip(combos, rows):
            print("h=%d w=%d pitch=%g s=%g noise=%g: scale error %.3g, ground share %.3f"
                  % (h, w, p, s, noise, abs(row[7] / s - 1.0), row[1] / row[2]))
        assert (np.abs(rows[:, 7] / np.array([s for _, s in combos]) - 1.0) <= bound).all()
        if noise == 0.0:
            share = rows[:, 1] / rows[:, 2]             # 0.18 - 0.41 to the two digits the prototype's figures have
            assert (share >= 0.175).all() and (share < 0.415).all()


def test_intrinsics_at_against_a_float64_restatement():
    for (H0, W0), (h, w) in (((375, 1242), (192, 640)), ((370, 1226), (320, 1024)), ((192, 640), (192, 640)),
                             ((37, 91), (19, 67))):
        inv_K = pointcloud.intrinsics(H0, W0)
        got = pointcloud.intrinsics_at(inv_K, (H0, W0), (h, w))
        assert got.dtype == np.float32 and got.shape == (3, 3) and got.flags["C_CONTIGUOUS"]
        # a map pixel (x, y) lies at image position ((x + 0.5) W0 / w - 0.5, (y + 0.5) H0 / h - 0.5)
        k = inv_K.astype(np.float64)
        for x, y in ((0, 0), (w - 1, h - 1), (5, 3)):
            at_image = k @ np.array([(x + 0.5) * W0 / w - 0.5, (y + 0.5) * H0 / h - 0.5, 1.0])
            np.testing.assert_allclose(got.astype(np.float64) @ np.array([x, y, 1.0]), at_image, rtol=0, atol=1e-6)
        sx, sy = W0 / w, H0 / h
        want = np.array([[k[0, 0] * sx, k[0, 1] * sy, k[0, 0] * (0.5 * sx - 0.5) + k[0, 1] * (0.5 * sy - 0.5) + k[0, 2]],
                         [k[1, 0] * sx, k[1, 1] * sy, k[1, 0] * (0.5 * sx - 0.5) + k[1, 1] * (0.5 * sy - 0.5) + k[1, 2]],
                         [k[2, 0] * sx, k[2, 1] * sy, k[2, 0] * (0.5 * sx - 0.5) + k[2, 1] * (0.5 * sy - 0.5) + k[2, 2]]])
        np.testing.assert_allclose(got, want.astype(np.float32), rtol=2e-7, atol=1e-12)
    same = pointcloud.intrinsics(192, 640)
    assert np.array_equal(pointcloud.intrinsics_at(same, (192, 640), (192, 640)), same)
    four = np.eye(4, dtype=np.float32)
    four[:3, :3] = same
    assert np.array_equal(pointcloud.intrinsics_at(four, (375, 1242), (192, 640)),
                          pointcloud.intrinsics_at(same, (375, 1242), (192, 640)))
    for bad in ((np.eye(2), (4, 4), (2, 2)), (same, (0, 4), (2, 2)), (same, (4, 4), (2, 0))):
        with pytest.raises(ValueError):
            pointcloud.intrinsics_at(*bad)


def test_ops_accepts_four_dimensions_and_both_shapes_of_inv_K(port):
    (call, _), ((want_rows, want_mask), _) = ground_checks.case(1)
    pred = torch.from_numpy(call.pred)
    n = pred.shape[0]
    four = np.eye(4, dtype=np.float32)
    four[:3, :3] = call.inv_K
    before = len(port.calls)
    for p, k in ((pred[:, None], call.inv_K), (pred, four), (pred, np.stack([call.inv_K] * n)),
                 (pred, np.stack([four] * n)), (pred, torch.from_numpy(call.inv_K))):
        rows, mask = ops.ground_scale(p, k, camera_height=ground_checks.HEIGHT, want_mask=True, backend=port)
        assert rows.dtype == torch.float32 and tuple(rows.shape) == (n, _lib.EVAL_OUT)
        assert ground_checks.same_bytes(rows.numpy(), want_rows) and ground_checks.same_bytes(mask.numpy(), want_mask)
    assert port.calls[before:] == ["bbd_ground_scale"] * 5              # one call each
    rows, mask = ops.ground_scale(pred, call.inv_K, camera_height=ground_checks.HEIGHT, backend=port)
    assert mask is None and ground_checks.same_bytes(rows.numpy(), want_rows)
    # a per-image matrix is used for its image: another camera for image 1 changes row 1 only
    per = np.stack([call.inv_K] * n)
    per[1, 1, 1] *= 1.5
    rows = ops.ground_scale(pred, per, camera_height=ground_checks.HEIGHT, backend=port)[0].numpy()
    assert ground_checks.same_bytes(rows[[0, 2]], want_rows[[0, 2]]) and rows[1, 0] != want_rows[1, 0]


def test_rows_feed_the_cloud_export_in_metres(port):
    """Column 7 is the slot `ops.point_cloud` multiplies depths by: the ground of the scaled cloud lies a camera height
    below the camera."""
    (call, _), ((rows, mask), _) = ground_checks.case(1)
    h, w = call.pred.shape[1:]
    got_rows, _ = ops.ground_scale(torch.from_numpy(call.pred), call.inv_K, camera_height=ground_checks.HEIGHT, backend=port)
    verts, counts, offs = ops.point_cloud(torch.from_numpy(call.pred), ops.cloud_rows([(h, w)] * 3), call.inv_K,
                                          rows=got_rows, min_depth=0.0, max_depth=80.0, backend=port)
    clouds = pointcloud.cloud_arrays(verts, counts, offs)
    assert len(clouds[0]) == len(clouds[1]) == h * w and len(clouds[2]) == 0        # NaN scale: an empty cloud
    for i in (0, 1):
        y = clouds[i]["y"][mask[i].reshape(-1) == 1]
        assert len(y) >= 64 and (np.abs(y / ground_checks.HEIGHT - 1.0) < 1e-4).all()


def test_argument_errors_are_the_same_on_both_sides_of_the_abi(port):
    """Nothing is launched for a refused call, so the library's status can be asked for on a machine without a GPU."""
    ground_checks.case7(port)
    with pytest.raises(_lib.BbdError, match="bbd_ground_scale failed with status -1"):
        ops.ground_scale(torch.ones(1, 3, 3), np.eye(3), camera_height=0.0, backend=port)
