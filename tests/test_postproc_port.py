"""CPU tier of the flip post-processing: the host port of bbd_postproc.hip (same bbd_postproc_math.h) driven through
`ops.post_process_disp`, against the literal numpy formulation of Monodepth2's batch_post_process_disparity
(tests/postproc_ref.py, computed live).  The kernel's arithmetic is the float64 blend rounded once, spelled operation by
operation, so the tolerance is equality."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import postproc_ref  # noqa: E402
from ports import PortBackend  # noqa: E402
from baseboostdepth_amd import _lib, ops  # noqa: E402
from baseboostdepth_amd._lib import ptr  # noqa: E402


@pytest.fixture(scope="module")
def port():
    return PortBackend()


def test_shapes_cover_the_ramp_and_the_centre_column():
    """What the shape list is chosen for: pixels strictly inside the 0.05-0.1 ramp, an odd width, n > 1."""
    inside = {}
    for n, h, w in postproc_ref.SHAPES:
        l = np.linspace(0, 1, w)
        inside[w] = int(((l > 0.05) & (l < 0.1)).sum())
    assert inside[41] == 1 and inside[130] == 6
    assert any(w % 2 for _, _, w in postproc_ref.SHAPES) and any(n > 1 for n, _, _ in postproc_ref.SHAPES)
    assert any(w == 1 for _, _, w in postproc_ref.SHAPES) and any(1 < w < 64 for _, _, w in postproc_ref.SHAPES)


@pytest.mark.parametrize("shape", postproc_ref.SHAPES)
@pytest.mark.parametrize("four_dim", [False, True])
def test_host_port_equals_numpy_reference(port, shape, four_dim):
    n, h, w = shape
    disp = postproc_ref.make_input(n, h, w, seed=100 + w)
    x = torch.from_numpy(disp)
    got = ops.post_process_disp(x[:, None] if four_dim else x, backend=port)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, h, w)
    want = postproc_ref.reference(disp)
    assert want.dtype == np.float32
    assert np.array_equal(got.numpy(), want)


def test_flipped_half_is_read_mirrored(port):
    """Where the mask is 1 the flipped image's prediction wins, mirrored back; at the other border the plain one."""
    n, h, w = 2, 3, 200
    disp = postproc_ref.make_input(n, h, w, seed=7)
    got = ops.post_process_disp(torch.from_numpy(disp), backend=port).numpy()
    assert np.array_equal(got[:, :, 0], disp[n:, :, w - 1]) and np.array_equal(got[:, :, w - 1], disp[:n, :, w - 1])
    mid = np.float32(0.5) * (disp[:n, :, 100] + disp[n:, :, w - 1 - 100])
    assert np.array_equal(got[:, :, 100], mid)


def test_port_returns_the_abi_argument_errors(port):
    disp, out = torch.ones(2, 3, 4), torch.zeros(1, 3, 4)
    null = ctypes.c_void_p(0)
    assert port.status("bbd_post_process_disp", ptr(disp), ptr(out), 1, 3, 4) == 0
    assert port.status("bbd_post_process_disp", null, ptr(out), 1, 3, 4) == -1
    assert port.status("bbd_post_process_disp", ptr(disp), null, 1, 3, 4) == -1
    for bad in ((0, 3, 4), (1, 0, 4), (1, 3, 0)):
        assert port.status("bbd_post_process_disp", ptr(disp), ptr(out), *bad) == -1


def test_library_returns_the_abi_argument_errors_without_a_launch():
    """The same refusals from the HIP library itself: they return before anything touches a device."""
    lib = _lib.get_lib()
    fn = lib._dll.bbd_post_process_disp
    one = ctypes.c_void_p(64)                           # never dereferenced: every call below is refused
    assert fn(None, one, 1, 3, 4, None) == -1 and fn(one, None, 1, 3, 4, None) == -1
    for bad in ((0, 3, 4), (1, 0, 4), (1, 3, 0), (-1, 3, 4)):
        assert fn(one, one, *bad, None) == -1


def test_odd_leading_dimension_is_refused(port):
    for shape in ((3, 4, 5), (1, 1, 4, 5), (0, 4, 5)):
        with pytest.raises(ValueError):
            ops.post_process_disp(torch.ones(*shape), backend=port)
    with pytest.raises(ValueError):
        ops.post_process_disp(torch.ones(4, 5), backend=port)


def test_hip_backend_refuses_cpu_tensors():
    from baseboostdepth_amd.csrc.build import build
    build()
    with pytest.raises(_lib.BbdError):
        ops.post_process_disp(torch.rand(2, 1, 8, 8), backend=ops.HipBackend())


def test_options_carry_the_four_flags():
    from baseboostdepth_amd.options import MonodepthOptions
    o = MonodepthOptions().parse(["--ext_disp_to_eval", "x.npy", "--no_eval", "--post_process", "--save_pred_disps"])
    assert o.ext_disp_to_eval == "x.npy" and o.no_eval is True and o.post_process is True and o.save_pred_disps is True
    d = MonodepthOptions().parse([])
    assert d.ext_disp_to_eval is None and d.no_eval is False and not d.post_process and not d.save_pred_disps
    with pytest.raises(SystemExit):
        MonodepthOptions().parse(["--eval_eigen_to_benchmark"])


def test_predict_cli_parses_post_process():
    from baseboostdepth_amd import inference
    base = ["--image_path", "a", "--save_path", "b", "--weights", "c"]
    assert inference.parse_args(base + ["--post_process"]).post_process is True
    assert inference.parse_args(base).post_process is False


def test_save_without_a_weights_folder_is_refused_before_any_prediction():
    """`save_pred_disps` with load_weights_folder unset: ValueError before a model, a loader or a device is touched."""
    import types
    from baseboostdepth_amd import evaluation

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("nothing may be used before the refusal")

    for folder in ("None", None):
        opt = types.SimpleNamespace(eval_mono=True, eval_stereo=False, cuda=0, eval_split="eigen", splits_dir="nowhere",
                                    save_pred_disps=True, load_weights_folder=folder)
        with pytest.raises(ValueError):
            evaluation.evaluate(opt, dataloader=Untouchable(), models=(Untouchable(), Untouchable()))


def test_external_file_must_be_a_numeric_stack_of_maps(tmp_path):
    import types
    from baseboostdepth_amd import evaluation
    opt = types.SimpleNamespace(eval_mono=True, eval_stereo=False, cuda=0, eval_split="eigen", splits_dir="nowhere")
    for name, arr in (("two_dim.npy", np.ones((4, 5), np.float32)), ("strings.npy", np.array([[["a"]]]))):
        np.save(tmp_path / name, arr)
        opt.ext_disp_to_eval = str(tmp_path / name)
        with pytest.raises(ValueError):
            evaluation.evaluate(opt)
