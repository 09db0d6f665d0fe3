"""CPU tier of the point-cloud export: the host port of bbd_cloud.hip (the same bbd_cloud_math.h) driven through
`ops.point_cloud`, under the checks of tests/cloud_checks.py - bit for bit against tests/cloud_ref.py.  The GPU tier
(tests/test_gpu_cloud.py) runs the same checks through the kernels."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cloud_checks as C  # noqa: E402
import cloud_ref  # noqa: E402
from ports import PortBackend  # noqa: E402
from baseboostdepth_amd import _lib, ops, pointcloud  # noqa: E402


@pytest.fixture(scope="module")
def port():
    return PortBackend()


@pytest.mark.parametrize("check", C.ALL_CHECKS, ids=lambda f: f.__name__)
def test_port(port, check):
    check(port, "cpu")


def test_library_returns_the_abi_argument_errors_without_a_launch():
    """The refusals from the HIP library itself: they return before anything touches a device."""
    lib = _lib.get_lib()
    fn = lib._dll.bbd_point_cloud
    one = 64                                             # never dereferenced: every call below is refused
    good = [one] * 10 + [8, 1, 4, 4, 16, 16, 1, 1e-3, 80.0, 1e-3, 80.0, 1.0, 0]
    for k in (0, 2, 4, 7, 8, 9):
        assert fn(*[None if j == k else v for j, v in enumerate(good)], None) == -1
    for k in (11, 12, 13, 14, 15, 16):
        assert fn(*[0 if j == k else v for j, v in enumerate(good)], None) == -1
    assert fn(*good[:22], 256, None) == -1 and fn(*good[:22], 2, None) == -1
    assert fn(*[None if j == 1 else v for j, v in enumerate(good[:22])], _lib.CLOUD_MASK_GT, None) == -1
    assert fn(*[72 if j == 7 else v for j, v in enumerate(good)], None) == -1
    assert fn(*[65536 if j == 11 else v for j, v in enumerate(good)], None) == -2
    assert lib.point_cloud_scratch_ints(16, 375, 1242, 1) == 16 * ((375 * 1242 + 255) // 256)


def test_constants_match_the_header():
    import re
    text = open(os.path.join(ROOT, "include", "bbd_hip.h")).read()
    for macro, val in (("BBD_CLOUD_DESC", _lib.CLOUD_DESC), ("BBD_CLOUD_VERTEX", _lib.CLOUD_VERTEX),
                       ("BBD_CLOUD_FROM_GT", _lib.CLOUD_FROM_GT), ("BBD_CLOUD_CLAMP", _lib.CLOUD_CLAMP),
                       ("BBD_CLOUD_MASK_GT", _lib.CLOUD_MASK_GT), ("BBD_CLOUD_RAYS_REFERENCE", _lib.CLOUD_RAYS_REFERENCE)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % macro, text).group(1)) == val
    assert pointcloud.VERTEX_DTYPE.itemsize == _lib.CLOUD_VERTEX == 16
    assert _lib.ABI_VERSION >= 15


def test_cloud_arrays_are_views_of_one_copy(port):
    rng = np.random.default_rng(2)
    shapes = [(5, 7), (9, 4)]
    pred = torch.from_numpy(np.stack([C.depth_like(rng, 3, 4) for _ in shapes]))
    out = ops.point_cloud(pred, ops.cloud_rows(shapes), C.camera(0, 5, 7), stride=2, backend=port)
    clouds = pointcloud.cloud_arrays(*out)
    assert [len(c) for c in clouds] == [3 * 4, 5 * 2] and all(c.dtype == pointcloud.VERTEX_DTYPE for c in clouds)
    assert all(c.base is not None for c in clouds) and (clouds[0]["alpha"] == 255).all()
    host = out[0].numpy()                                # on the CPU tier the "copy" is the buffer itself
    assert all(np.shares_memory(c, host) for c in clouds)
    want, _ = cloud_ref.cloud(pred[1].numpy(), shapes[1], C.camera(0, 5, 7), C.lut(), stride=2)
    assert np.array_equal(clouds[1].view(np.uint8), want.view(np.uint8))


def test_wrapper_refuses_what_it_can_see(port):
    pred = torch.ones(1, 2, 2)
    with pytest.raises(ValueError):
        ops.point_cloud(pred, ops.cloud_rows([(3, 3)]), np.eye(3), stride=0, backend=port)
    with pytest.raises(ValueError):
        ops.point_cloud(pred, ops.cloud_rows([(3, 3)]), np.eye(3), mask_gt=True, backend=port)
    with pytest.raises(_lib.BbdError):
        ops.point_cloud(pred, ops.cloud_rows([(3, 3)]), np.eye(3), backend=ops.HipBackend())     # no CPU path
