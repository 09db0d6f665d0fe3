"""Shared pieces of the full-trajectory odometry tests (CPU tier through the host port, GPU tier through the HIP backend).

Inputs are synthetic and seeded (`make`): ground-truth steps of about 1 m with 10 % jitter and small random rotations
from an arbitrary first pose, printed to 7 digits and parsed by `evaluation.read_poses_file`; the network's steps are
derived from the parsed ground truth, their translation scaled by `s`, optionally perturbed, and cast to float32.
lengths = (5, 10, 20, 40), step = 4.  The reference is tests/traj_ref.py (numpy float64, two independent alignments).

`last` is a discrete choice, so `make` asserts on the reference alone that no (first, L) of a case has a frame within
1e-6 of the threshold; the indices and every count are then compared exactly.

Acceptance rules - every bound follows from the arithmetic, is computed per case and printed with the measured worst:
  traj, gt_traj, dist   tau_T = 8 F 2^-52 max(1, max |translation|), absolute: one inverse and one product per step are
                        fewer than 8 roundings of that size, accumulated linearly over F frames (the largest
                        translation is taken over the poses file, gt_traj and traj)
  aligned, transform,   tau = max(tau_T max(1, c), 16 spread), spread = the largest difference between the reference
  ATE figures           with Umeyama's alignment and with Horn's on that case; c relatively at tau / sigma_g
  t_err L               16 tau; means of t_err: 16 tau / the (smallest) length
  clamped cosine        kappa = 16 * 8 F 2^-52 (recovered from r_err as cos(r_err L), whose own rounding adds 4 * 2^-52)
  r_err L               acos(1 - kappa): acos is ill-conditioned at 1 and this is the largest change a cosine gap of
                        kappa can cause; means of r_err: the same over the (smallest) length
  NaN                   at exactly the reference's positions, as 0x7ff8000000000000
  last, counts, F       exact
Rank-1 cases (kind "collinear", and the two frames of J = 1): R is not unique, and `transform` and the rotation blocks
of `aligned`, which are R R_j, share its freedom; the aligned POSITIONS, c, the ATE figures and every sub-sequence error
(which depends on the alignment through c alone) are compared, and spread is taken over those.

Measured worst values over this file's cases, as a fraction of the bound, the same on the host port and on an MI355X
(their outputs are equal bit for bit outside the r_err columns):
  traj 0.005 tau_T;  gt_traj 0.040 tau_T;  dist 0.003 tau_T;  aligned 0.12 tau;  transform 0.10 tau;  ATE 0.010 tau;
  c 0.001;  t_err L 0.0004 of 16 tau;  cosine 0.0007 kappa;  r_err L below 1e-4 of acos(1 - kappa);
  device against host port in the r_err columns: at most 2.8e-17 rad."""
import os

import numpy as np
import torch

import traj_ref as ref

LENGTHS = (5.0, 10.0, 20.0, 40.0)
STEP = 4
EPS = 2.0 ** -52
FIELDS = ("traj", "gt_traj", "aligned", "transform", "dist", "pairs", "per_length", "summary")
CANON = 0x7FF8000000000000

#        name: J, s, noise (rad, and metres per metre), kind, surplus ground-truth rows, seed, modes
CASES = {
    "exact": (63, 0.037, 0.0, "general", 0, 11, ("sim3",)),
    "noisy63": (63, 0.5, 1e-3, "general", 0, 12, ref.MODES),
    "noisy257": (257, 2.0, 2e-3, "general", 0, 13, ("sim3",)),
    "noisy699": (699, 0.25, 1.5e-3, "general", 0, 14, ("sim3",)),
    "scan255": (255, 1.0, 1e-3, "general", 0, 15, ("sim3",)),
    "scan256": (256, 1.0, 1e-3, "general", 0, 16, ("se3",)),
    "single": (1, 0.5, 0.0, "collinear", 0, 17, ("sim3", "scale")),
    "no_pair": (2, 0.5, 1e-3, "general", 0, 18, ("sim3",)),
    "planar": (63, 0.5, 1e-3, "planar", 0, 19, ("sim3",)),
    "collinear": (63, 0.5, 0.0, "collinear", 0, 20, ("sim3", "se3")),
    "mirrored": (63, 0.5, 0.0, "mirrored", 0, 21, ("sim3", "se3")),
    "zero": (63, 1.0, 0.0, "zero", 0, 22, ref.MODES),
    "surplus": (63, 0.5, 1e-3, "general", 5, 12, ("sim3",)),
}
EVERY = [(name, mode) for name, spec in CASES.items() for mode in spec[6]]
# what the entry refuses: J, M, lengths, n_len (None: all of them), step, mode
BAD = [
    (0, 64, LENGTHS, None, 4, 0), (63, 63, LENGTHS, None, 4, 0), (63, 64, LENGTHS, 0, 4, 0),
    (63, 64, LENGTHS + (50.0, 60.0, 70.0, 80.0, 90.0), None, 4, 0), (63, 64, LENGTHS, None, 0, 0),
    (63, 64, (5.0, 5.0, 20.0, 40.0), None, 4, 0), (63, 64, (10.0, 5.0, 20.0, 40.0), None, 4, 0),
    (63, 64, (0.0, 5.0, 20.0, 40.0), None, 4, 0), (63, 64, (-1.0, 5.0, 20.0, 40.0), None, 4, 0),
    (63, 64, (5.0, float("nan"), 20.0, 40.0), None, 4, 0), (63, 64, (5.0, 10.0, 20.0, float("inf")), None, 4, 0),
    (63, 64, LENGTHS, None, 4, 4), (63, 64, LENGTHS, None, 4, -1)]


def rotation(v):
    """Rodrigues: the rotation of axis-angle v."""
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def rigid(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def ground_truth(rng, F, kind):
    """F ground-truth poses [F,4,4] (before they are printed)."""
    if kind == "planar":                     # motion in the plane y = 0, rotations about y: every y is exactly 0
        G = [rigid(rotation(np.array([0.0, rng.uniform(-3, 3), 0.0])), np.array([rng.uniform(-80, 80), 0.0, rng.uniform(-80, 80)]))]
    elif kind == "collinear":                # a first pose without rotation, so that the printed line is exactly straight
        G = [rigid(np.eye(3), np.array([0.0, 0.0, rng.uniform(-80, 80)]))]
    else:
        G = [rigid(rotation(rng.uniform(-1, 1, 3) * 2.0), rng.uniform(-80, 80, 3))]
    for _ in range(F - 1):
        length = 1.0 + 0.1 * rng.uniform(-1, 1)
        if kind == "planar":
            D = rigid(rotation(np.array([0.0, rng.normal() * 0.03, 0.0])), np.array([rng.normal() * 0.02, 0.0, length]))
        elif kind == "collinear":            # the camera turns a little, the path does not: positions stay on the z axis
            D = rigid(np.eye(3), np.array([0.0, 0.0, length]))
        else:
            D = rigid(rotation(rng.normal(size=3) * (0.06 if kind == "mirrored" else 0.03)),
                      np.array([rng.normal() * 0.02, rng.normal() * 0.02, length]))
        G.append(G[-1] @ D)
    G = np.stack(G)
    if kind == "collinear":
        for j in range(1, F):
            G[j, :3, :3] = rotation(rng.normal(size=3) * 0.03)
    return G


def print_poses(G):
    return "".join(" ".join("%.6e" % x for x in g[:3].reshape(-1)) + "\n" for g in G)


def derive_steps(gt, J, s, noise, kind, rng):
    """float32 [J,16]: steps[j] plays inv(inv(G_j) G_{j+1}) with the translation scaled by s."""
    if kind == "zero":
        return np.tile(np.eye(4, dtype=np.float32).reshape(16), (J, 1))
    G = ref.rows_to_4x4(gt)
    if kind == "mirrored":                   # the mirror image y -> -y of the path, still made of proper rotations
        Mi = np.diag([1.0, -1.0, 1.0, 1.0])
        G = Mi @ G @ Mi
    steps = np.empty((J, 16), np.float32)
    for j in range(J):
        rel = np.linalg.inv(G[j]) @ G[j + 1]
        rel[:3, 3] *= s
        if noise:
            rel = rel @ rigid(rotation(rng.normal(size=3) * noise), rng.normal(size=3) * noise * s)
        steps[j] = np.linalg.inv(rel).reshape(16).astype(np.float32)
    return steps


_MADE = {}


def make(name):
    """The case's inputs, built once per process: dict with `steps` float32 [J,16], `gt` float64 [M,12] (parsed from the
    7-digit text by the product's parser), `text`, J, s, kind."""
    if name in _MADE:
        return _MADE[name]
    import tempfile
    from baseboostdepth_amd import evaluation
    J, s, noise, kind, surplus, seed, _ = CASES[name]
    rng = np.random.default_rng(seed)
    text = print_poses(ground_truth(rng, J + 1 + surplus, kind))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "%s.txt" % name)
        with open(path, "w") as f:
            f.write(text)
        gt = evaluation.read_poses_file(path)
    assert gt.shape == (J + 1 + surplus, 12)
    case = {"steps": derive_steps(gt, J, s, noise, kind, rng), "gt": gt, "text": text, "J": J, "s": s, "kind": kind,
            "name": name}
    dist = ref.path_length(ref.gt_trajectory(gt, J + 1)[:, :3, 3])
    gaps = [np.abs(dist - dist[first] - L).min() for first in range(0, J + 1, STEP) for L in LENGTHS]
    assert min(gaps) > 1e-6, "%s: a frame lies within 1e-6 of a sub-sequence threshold (%.3e): choose another seed" \
        % (name, min(gaps))
    _MADE[name] = case
    return case


_REFS = {}


def reference(name, mode):
    """(Umeyama-aligned reference, spread over the compared outputs) of the case, computed once."""
    if (name, mode) not in _REFS:
        case = make(name)
        a = ref.evaluate(case["steps"], case["gt"], LENGTHS, STEP, mode, ref.umeyama)
        b = ref.evaluate(case["steps"], case["gt"], LENGTHS, STEP, mode, ref.horn)
        rank1 = case["kind"] == "collinear"
        diffs = [np.abs(a["aligned"][:, :3, 3] - b["aligned"][:, :3, 3]), np.abs(a["summary"][3:6] - b["summary"][3:6])]
        if not rank1:
            diffs += [np.abs(a["aligned"] - b["aligned"]), np.abs(a["transform"] - b["transform"])]
        spread = max([float(np.nanmax(d)) for d in diffs if not np.isnan(d).all()] + [0.0])
        _REFS[(name, mode)] = (a, spread)
    return _REFS[(name, mode)]


def run(name, mode, backend, device, gt_rows=None):
    """One `evaluation.pose_trajectory` call on the case."""
    from baseboostdepth_amd import evaluation
    case = make(name)
    gt = case["gt"] if gt_rows is None else case["gt"][:gt_rows]
    steps = torch.from_numpy(case["steps"]).to(device)
    return evaluation.pose_trajectory(steps.view(-1, 4, 4), gt, align=mode, lengths=LENGTHS, step=STEP, backend=backend)


def host(res):
    return {k: getattr(res, k).cpu().numpy() for k in FIELDS}


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


WORST = {}          # what -> largest measured difference / bound of this process


def _within(got, want, tol, what, label):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (label, what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s %s: NaNs at other positions than the reference's" % (label, what)
    nan = np.isnan(got)
    assert (got.view(np.uint64)[nan] == CANON).all(), "%s %s: a NaN with other bits than the canonical ones" % (label, what)
    ok = ~nan
    worst = float(np.abs(got - want)[ok].max()) if ok.any() else 0.0
    tol = float(tol)
    print("%s %s: max |difference| %.3e (bound %.3e)" % (label, what, worst, tol))
    if tol > 0:
        WORST[what] = max(WORST.get(what, 0.0), worst / tol)
    assert worst <= tol, (label, what, worst, tol)


def tolerances(name, mode):
    case = make(name)
    want, spread = reference(name, mode)
    F = case["J"] + 1
    big = max(1.0, float(np.abs(case["gt"][:F].reshape(-1, 3, 4)[:, :, 3]).max()),
              float(np.abs(want["gt_traj"][:, :3, 3]).max()), float(np.abs(want["traj"][:, :3, 3]).max()))
    tau_T = 8 * F * EPS * big
    c = want["summary"][6]
    tau = max(tau_T * (max(1.0, abs(c)) if np.isfinite(c) else 1.0), 16 * spread)
    kappa = 16 * 8 * F * EPS
    return {"tau_T": tau_T, "tau": tau, "kappa": kappa, "r": float(np.arccos(1 - kappa)), "spread": spread}


def check(name, mode, out):
    """`out` (dict of numpy arrays, `host(res)`) against the reference under the rules of this file's docstring."""
    case = make(name)
    want, _ = reference(name, mode)
    tol = tolerances(name, mode)
    label = "%s/%s" % (name, mode)
    print("%s: tau_T %.3e, spread %.3e, tau %.3e, kappa %.3e" % (label, tol["tau_T"], tol["spread"], tol["tau"], tol["kappa"]))
    F, n_len = case["J"] + 1, len(LENGTHS)
    n_first = -(-F // STEP)
    shapes = {"traj": (F, 4, 4), "gt_traj": (F, 4, 4), "aligned": (F, 4, 4), "transform": (4, 4), "dist": (F,),
              "pairs": (n_first, n_len, 4), "per_length": (n_len, 3), "summary": (8,)}
    for k in FIELDS:
        assert out[k].shape == shapes[k] and out[k].dtype == np.float64, (label, k, out[k].shape, out[k].dtype)
    lens = np.asarray(LENGTHS)
    _within(out["traj"], want["traj"], tol["tau_T"], "traj", label)
    _within(out["gt_traj"], want["gt_traj"], tol["tau_T"], "gt_traj", label)
    _within(out["dist"], want["dist"], tol["tau_T"], "dist", label)
    assert (np.diff(out["dist"]) >= 0).all() and out["dist"][0] == 0
    rank1 = case["kind"] == "collinear"
    if rank1:
        _within(out["aligned"][:, :3, 3], want["aligned"][:, :3, 3], tol["tau"], "aligned", label)
        assert np.array_equal(out["aligned"][:, 3], np.tile([0.0, 0, 0, 1], (F, 1)))
    else:
        _within(out["aligned"], want["aligned"], tol["tau"], "aligned", label)
        _within(out["transform"], want["transform"], tol["tau"], "transform", label)
    R = out["transform"][:3, :3]                         # whatever the rank: a proper rotation over (0 0 0 1)
    assert np.abs(R @ R.T - np.eye(3)).max() < 64 * EPS and abs(np.linalg.det(R) - 1) < 64 * EPS
    assert np.array_equal(out["transform"][3], [0.0, 0, 0, 1])
    _within(out["summary"][3:6], want["summary"][3:6], tol["tau"], "ate", label)
    c_want = want["summary"][6]
    if np.isnan(c_want):
        _within(out["summary"][6:7], [c_want], 0.0, "c", label)
    else:
        _within(out["summary"][6:7] / c_want, [1.0], tol["tau"] / want["sigma_g"], "c", label)
    assert np.array_equal(out["pairs"][:, :, 0], want["pairs"][:, :, 0]), "%s: another `last`" % label
    assert np.array_equal(out["pairs"][:, :, 3], np.zeros((n_first, n_len)))
    assert np.array_equal(out["per_length"][:, 2], want["per_length"][:, 2]) and out["summary"][2] == want["summary"][2]
    assert out["summary"][7] == F
    _within(out["pairs"][:, :, 1] * lens, want["pairs"][:, :, 1] * lens, 16 * tol["tau"], "t_err L", label)
    _within(out["pairs"][:, :, 2] * lens, want["pairs"][:, :, 2] * lens, tol["r"], "r_err L", label)
    _within(np.cos(out["pairs"][:, :, 2] * lens), np.clip(want["cosines"], -1, 1), tol["kappa"] + 4 * EPS, "cosine", label)
    _within(out["per_length"][:, 0] * lens, want["per_length"][:, 0] * lens, 16 * tol["tau"], "t_err L", label)
    _within(out["per_length"][:, 1] * lens, want["per_length"][:, 1] * lens, tol["r"], "r_err L", label)
    _within(out["summary"][0:1] * lens[0], want["summary"][0:1] * lens[0], 16 * tol["tau"], "t_err L", label)
    _within(out["summary"][1:2] * lens[0], want["summary"][1:2] * lens[0], tol["r"], "r_err L", label)
    return tol


def behind_acos(out, lengths=LENGTHS):
    """(the outputs that must agree bit for bit between the device and the host port, those behind acos)."""
    exact = {k: out[k] for k in ("traj", "gt_traj", "aligned", "transform", "dist")}
    exact["pairs"] = np.ascontiguousarray(out["pairs"][:, :, [0, 1, 3]])
    exact["per_length"] = np.ascontiguousarray(out["per_length"][:, [0, 2]])
    exact["summary"] = np.ascontiguousarray(out["summary"][[0, 2, 3, 4, 5, 6, 7]])
    lens = np.asarray(lengths, np.float64)
    angles = {"pairs": out["pairs"][:, :, 2] * lens, "per_length": out["per_length"][:, 1] * lens,
              "summary": out["summary"][1:2] * lens[0]}
    return exact, angles
