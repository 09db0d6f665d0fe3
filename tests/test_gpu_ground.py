"""GPU tier of the ground-plane scale recovery (bbd_ground.hip through the C ABI): rows and masks of the cases of
tests/ground_checks.py byte for byte those of the host port, twice, and the rows as the ratio of the cloud export."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ground_checks  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    from baseboostdepth_amd import ops
    return ops.default_backend()


@pytest.fixture(scope="module")
def port():
    from ports import PortBackend
    return PortBackend()


@pytest.mark.parametrize("number", ground_checks.CASES)
def test_kernel_equals_the_port_byte_for_byte(hip, port, number):
    """A difference here with equal masks would point at the square root or a division: the device's and the host's must
    both be correctly rounded (the specification wants such a finding written down, not covered by a tolerance)."""
    calls, refs = ground_checks.case(number)
    for call, (ref_rows, ref_mask) in zip(calls, refs):
        want_rows, want_mask = ground_checks.run(call, port, "cpu")
        assert ground_checks.same_bytes(want_rows, ref_rows) and ground_checks.same_bytes(want_mask, ref_mask)
        rows, mask = ground_checks.run(call, hip, DEV)
        print("case %d: count %s, candidates %s, scale %s" % (number, rows[:, 1], rows[:, 2], rows[:, 7]))
        assert ground_checks.same_bytes(mask, want_mask)
        assert ground_checks.same_bytes(rows, want_rows), (rows, want_rows)
        again_rows, again_mask = ground_checks.run(call, hip, DEV)
        assert ground_checks.same_bytes(again_rows, rows) and ground_checks.same_bytes(again_mask, mask)


def test_rows_scale_the_cloud_export_to_metres(hip):
    """`ops.point_cloud(rows=ground_rows)` on case 1: the ground points of the cloud lie a camera height below the camera
    (y within 1e-4 relative); the image without ground has a NaN ratio and exports nothing."""
    from baseboostdepth_amd import ops, pointcloud
    (call, _), ((_, mask), _) = ground_checks.case(1)
    h, w = call.pred.shape[1:]
    pred = torch.from_numpy(call.pred).to(DEV)
    rows, _ = ops.ground_scale(pred, call.inv_K, camera_height=ground_checks.HEIGHT, backend=hip)
    assert rows.is_cuda
    cloud = ops.point_cloud(pred, ops.cloud_rows([(h, w)] * 3), call.inv_K, rows=rows, min_depth=0.0, max_depth=80.0,
                            backend=hip)
    clouds = pointcloud.cloud_arrays(*cloud)
    assert len(clouds[0]) == len(clouds[1]) == h * w and len(clouds[2]) == 0
    for i in (0, 1):
        y = clouds[i]["y"][mask[i].reshape(-1) == 1]
        assert len(y) >= 64 and (np.abs(y / ground_checks.HEIGHT - 1.0) < 1e-4).all()


def test_argument_errors_are_the_same_on_both_sides_of_the_abi(port):
    """Case 7 on the machine with the GPU: a refused call launches nothing and returns the port's status."""
    ground_checks.case7(port)
