"""The cases both tiers of the ground-scale tests run (tests/test_ground_port.py on the host port, tests/test_gpu_ground.py
on the MI355X), each with the precondition that keeps it from going hollow, asserted on the numpy reference
(tests/ground_ref.py).  A case is a list of calls; a call is the arguments of `ops.ground_scale` as numpy arrays.

  1  n = 3 at 19 x 67 (a tile edge is crossed both ways): a level road, a road at scale 7.3, a wall only (no ground: NaN
     scale, empty mask) - the batch once as depths and once as disparities (the flag belongs to the call)
  2  n = 2 at 33 x 130, 0.2 % noise, about 5 % of the pixels 0, NaN, +inf or negative: each removes exactly its 3 x 3
     neighbourhood from the candidates
  3  2 x 9 and 9 x 2: no candidates; 3 x 3: one
  4  an even number of ground pixels with two different middle values, and exactly one ground pixel: the lower median
  5  min_count = count + 1: NaN with the counts kept; min_count = count: a scale
  6  n = 2 at 192 x 640: the select sweeps many pixels per thread
  7  every argument error: the status from the port equals the status from the library (`case7`)
"""
import collections
import functools

import numpy as np

import ground_ref

Call = collections.namedtuple("Call", "pred inv_K kw")
F = np.float32
HEIGHT = 1.65


def _call(pred, inv_K=None, **kw):
    pred = np.ascontiguousarray(pred, F)
    inv_K = ground_ref.kitti_inv_K(*pred.shape[1:]) if inv_K is None else np.asarray(inv_K, F)
    return Call(pred, inv_K, kw)


def _ref(call):
    return ground_ref.ground_scale(call.pred, call.inv_K, **call.kw)


def _is_nan_bits(v):
    return np.asarray(v, F).view(np.uint32) == ground_ref.NAN_BITS


def _case1():
    h, w = 19, 67
    depth = np.stack([ground_ref.scene(h, w), ground_ref.scene(h, w, scale=7.3), ground_ref.scene(h, w, plane=False)])
    calls = [_call(depth), _call(F(1) / depth, pred_is_disp=True)]
    for call in calls:
        rows, mask, cand, _ = _ref(call)
        assert (rows[:2, 1] >= 64).all() and (rows[:, 2] == (h - 2) * (w - 2)).all()
        assert mask[0, :, :63].any() and mask[0, :, 64:].any() and mask[0, :16].any() and mask[0, 16:].any()
        assert abs(rows[0, 7] - 1.0) < 1e-5 and abs(rows[1, 7] / 7.3 - 1.0) < 1e-5
        assert rows[2, 1] == 0 and _is_nan_bits(rows[2, [0, 7]]).all() and not mask[2].any()
    return calls


def _spoil(pred, share, seed):
    """`share` of the pixels of every map become 0, NaN, +inf or a negative value; returns the map of spoilt pixels."""
    rng = np.random.default_rng(seed)
    bad = rng.random(pred.shape) < share
    kind = rng.integers(0, 4, pred.shape)
    for k, value in enumerate((0.0, np.nan, np.inf, -3.0)):
        pred[bad & (kind == k)] = value
    return bad


def _case2():
    h, w = 33, 130
    depth = np.stack([ground_ref.scene(h, w, pitch_deg=2.0, noise=0.002, seed=1),
                      ground_ref.scene(h, w, pitch_deg=-3.0, scale=7.3, noise=0.002, seed=2)])
    bad = _spoil(depth, 0.05, 3)
    call = _call(depth)
    rows, mask, cand, _ = _ref(call)
    near = np.zeros_like(bad)                                  # pixels with a spoilt pixel among their nine
    padded = np.pad(bad, ((0, 0), (1, 1), (1, 1)))
    for dy in range(3):
        for dx in range(3):
            near |= padded[:, dy:dy + h, dx:dx + w]
    interior = np.zeros_like(bad)
    interior[:, 1:-1, 1:-1] = True
    assert np.array_equal(cand, interior & ~near) and 0.03 < bad.mean() < 0.07
    spoilt = depth[bad]
    assert (spoilt == 0).any() and np.isnan(spoilt).any() and np.isposinf(spoilt).any() and (spoilt < 0).any()
    assert (rows[:, 1] >= 64).all() and abs(rows[0, 7] - 1.0) < 2e-2 and abs(rows[1, 7] / 7.3 - 1.0) < 2e-2
    return [call]


def _case3():
    calls = [_call(ground_ref.scene(2, 9)[None]), _call(ground_ref.scene(9, 2)[None])]
    for call in calls:
        rows, mask, _, _ = _ref(call)
        assert rows[0, 1] == 0 and rows[0, 2] == 0 and _is_nan_bits(rows[0, [0, 7]]).all() and not mask.any()
    # a camera that looks down on the road: the one interior pixel of a 3 x 3 map is ground
    K = np.array([[4.0, 0, 1.0], [0, 4.0, -1.0], [0, 0, 1.0]])
    inv_K = np.linalg.inv(K).astype(F)
    one = _call(ground_ref.scene(3, 3, inv_K=inv_K)[None], inv_K, min_count=1)
    rows, mask, _, _ = _ref(one)
    assert rows[0, 1] == 1 and rows[0, 2] == 1 and mask[0, 1, 1] == 1 and mask.sum() == 1
    assert abs(rows[0, 7] - 1.0) < 1e-5
    return calls + [one]


def _case4():
    h, w = 19, 67
    base = ground_ref.scene(h, w, noise=0.002, seed=4)
    even = base.copy()
    ys, xs = np.nonzero(_ref(_call(base[None]))[1][0])
    for y, x in zip(ys[::7], xs[::7]):                          # cut ground pixels out until the count is even
        heights = _ref(_call(even[None]))[3][0]
        c = heights.size
        if c >= 2 and c % 2 == 0 and heights[(c - 1) // 2] != heights[c // 2]:
            break
        even[y, x] = np.nan
    call_even = _call(even[None], min_count=1)
    rows, _, _, (heights,) = _ref(call_even)
    c = heights.size
    assert c >= 2 and c % 2 == 0 and heights[(c - 1) // 2] < heights[c // 2] and rows[0, 0] == heights[c // 2 - 1]
    single = np.full((h, w), np.nan, F)
    y, x = int(ys[len(ys) // 2]), int(xs[len(xs) // 2])
    single[y - 1:y + 2, x - 1:x + 2] = ground_ref.scene(h, w)[y - 1:y + 2, x - 1:x + 2]
    call_single = _call(single[None], min_count=1)
    rows, mask, _, _ = _ref(call_single)
    assert rows[0, 1] == 1 and rows[0, 2] == 1 and mask[0, y, x] == 1 and abs(rows[0, 7] - 1.0) < 1e-5
    return [call_even, call_single]


def _case5():
    depth = ground_ref.scene(19, 67)[None]
    count = int(_ref(_call(depth))[0][0, 1])
    assert count >= 64
    refused, taken = _call(depth, min_count=count + 1), _call(depth, min_count=count)
    rows = _ref(refused)[0]
    assert _is_nan_bits(rows[0, [0, 7]]).all() and rows[0, 1] == count and rows[0, 2] == 17 * 65
    assert abs(_ref(taken)[0][0, 7] - 1.0) < 1e-5
    return [refused, taken]


def _case6():
    h, w = 192, 640
    depth = np.stack([ground_ref.scene(h, w, pitch_deg=2.0, scale=7.3),
                      ground_ref.scene(h, w, pitch_deg=-3.0, noise=0.002, seed=6)])
    call = _call(F(1) / depth, pred_is_disp=True)
    rows = _ref(call)[0]
    assert (rows[:, 1] > 16 * 1024).all() and abs(rows[0, 7] / 7.3 - 1.0) < 1e-5 and abs(rows[1, 7] - 1.0) < 2e-2
    return [call]


BUILDERS = {1: _case1, 2: _case2, 3: _case3, 4: _case4, 5: _case5, 6: _case6}
CASES = sorted(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(number):
    """(calls, reference results) of a case: built, checked against its precondition and referenced once per process."""
    calls = BUILDERS[number]()
    return calls, [_ref(c)[:2] for c in calls]


def case7(port):
    """Case 7: every argument error of the ABI; the status from the port equals the status from the library (nothing is
    launched for a refused call, so the library can be asked on a machine without a GPU), and the size helpers agree."""
    import ctypes
    import torch
    from baseboostdepth_amd import _lib
    from baseboostdepth_amd._lib import ptr
    from baseboostdepth_amd.csrc.build import build
    dll = ctypes.CDLL(build())
    fn = dll.bbd_ground_scale
    fn.argtypes, fn.restype = _lib.SIGNATURES["bbd_ground_scale"], ctypes.c_int
    buf = torch.zeros(64)
    m8 = torch.zeros(64, dtype=torch.uint8)
    good = dict(pred=ptr(buf), inv_K=ptr(buf), rows=ptr(buf), mask=ptr(m8), scratch=ptr(buf), n=1, h=3, w=3,
                camera_height=1.65, cos_threshold=0.99, min_count=1, flags=0)
    null = ctypes.c_void_p(0)
    E_BADARG, E_TOOMANY = -1, -2
    bad = [(dict(pred=null), E_BADARG), (dict(inv_K=null), E_BADARG), (dict(rows=null), E_BADARG),
           (dict(scratch=null), E_BADARG), (dict(n=0), E_BADARG), (dict(h=0), E_BADARG), (dict(w=0), E_BADARG),
           (dict(n=-1), E_BADARG), (dict(camera_height=0.0), E_BADARG), (dict(camera_height=-1.0), E_BADARG),
           (dict(camera_height=float("nan")), E_BADARG), (dict(cos_threshold=0.0), E_BADARG),
           (dict(cos_threshold=1.0000001), E_BADARG), (dict(cos_threshold=-0.5), E_BADARG),
           (dict(cos_threshold=float("nan")), E_BADARG), (dict(min_count=-1), E_BADARG), (dict(flags=2), E_BADARG),
           (dict(flags=1 | 16), E_BADARG), (dict(n=65536), E_TOOMANY), (dict(h=65536, w=32768), E_TOOMANY),
           (dict(h=1 << 30, w=4), E_TOOMANY)]
    for change, want in bad:
        args = tuple(dict(good, **change).values())
        assert port.status("bbd_ground_scale", *args) == want, change
        assert fn(*args, null) == want, change
    # the accepted edges, on the port (the library would launch): a NULL mask, cos_threshold 1, min_count 0, the flag
    for change in (dict(mask=null), dict(cos_threshold=1.0), dict(min_count=0), dict(flags=1), dict(n=4, h=4, w=4)):
        assert port.status("bbd_ground_scale", *tuple(dict(good, **change).values())) == 0, change
    sizes = dll.bbd_ground_scale_scratch_floats
    sizes.argtypes, sizes.restype = [ctypes.c_int] * 3, ctypes.c_long
    for n, h, w in ((3, 19, 67), (1, 1, 1), (65535, 1, 1), (2, 32768, 65535), (0, 4, 4), (1, 0, 4), (1, 4, -1),
                    (65536, 1, 1), (1, 65536, 32768)):
        want = n * h * w if min(n, h, w) >= 1 and n <= 65535 and h * w <= 0x7FFFFFFF else (-1 if min(n, h, w) < 1 else -2)
        assert port.lib.ground_scale_scratch_floats(n, h, w) == sizes(n, h, w) == want


def run(call, backend, device):
    """The call through `ops.ground_scale` on `device`: (rows, mask) as numpy arrays."""
    import torch
    from baseboostdepth_amd import ops
    rows, mask = ops.ground_scale(torch.from_numpy(call.pred).to(device), call.inv_K, camera_height=HEIGHT,
                                  want_mask=True, backend=backend, **call.kw)
    return rows.cpu().numpy(), mask.cpu().numpy()


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
