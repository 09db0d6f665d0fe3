"""numpy float64 restatement of the full-trajectory odometry scores, written from the definitions and not
from csrc/bbd_traj_math.h: plain loops, np.linalg.inv, np.cumsum, np.mean, a linear search for `last`.  It holds two
independent alignments - Umeyama's through np.linalg.svd and Horn's unit quaternion through np.linalg.eigh - whose
difference (`spread`) tells how well a case determines its alignment (tests/traj_checks.py).

Test infrastructure only."""
import numpy as np

MODES = ("sim3", "se3", "scale", "none")


def rows_to_4x4(rows):
    rows = np.asarray(rows, np.float64).reshape(-1, 3, 4)
    out = np.tile(np.eye(4), (rows.shape[0], 1, 1))
    out[:, :3, :] = rows
    return out


def trajectory(steps):
    """C_0 = I, C_{j+1} = C_j inv(steps[j])."""
    steps = np.asarray(steps, np.float64).reshape(-1, 4, 4)
    C = [np.eye(4)]
    for T in steps:
        C.append(C[-1] @ np.linalg.inv(T))
    return np.stack(C)


def gt_trajectory(gt, F):
    G = rows_to_4x4(gt)[:F]
    inv0 = np.linalg.inv(G[0])
    return np.stack([inv0 @ g for g in G])


def path_length(g):
    return np.concatenate([[0.0], np.cumsum(np.linalg.norm(g[1:] - g[:-1], axis=1))])


def umeyama(p, g, with_scale):
    """(c, R, t, branch): Umeyama 1991, eq. 34-42; branch = -1 where the reflection had to be undone."""
    mu_p, mu_g = p.mean(0), g.mean(0)
    dp, dg = p - mu_p, g - mu_g
    var_p = (dp ** 2).sum(1).mean()
    Sigma = (dg[:, :, None] * dp[:, None, :]).mean(0)
    if not Sigma.any():
        R, trace, branch = np.eye(3), 0.0, 1.0
    else:
        U, D, Vt = np.linalg.svd(Sigma)
        branch = -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0
        S = np.diag([1.0, 1.0, branch])
        R = U @ S @ Vt
        trace = float((D * np.diag(S)).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.float64(trace) / np.float64(var_p) if with_scale else 1.0
    return float(c), R, mu_g - c * (R @ mu_p), branch


def horn(p, g, with_scale):
    """(c, R, t, 0): Horn 1987 - the rotation is the eigenvector of the largest eigenvalue of the 4x4 matrix N built from
    M = sum p' g'^T; the scale is the one of his asymmetric form, sum g'.(R p') / sum |p'|^2."""
    mu_p, mu_g = p.mean(0), g.mean(0)
    dp, dg = p - mu_p, g - mu_g
    M = dp.T @ dg
    if not M.any():
        R = np.eye(3)
    else:
        (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = M
        N = np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                      [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                      [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                      [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])
        w, v = np.linalg.eigh(N)
        q0, qx, qy, qz = v[:, -1]
        R = np.array([[q0 * q0 + qx * qx - qy * qy - qz * qz, 2 * (qx * qy - q0 * qz), 2 * (qx * qz + q0 * qy)],
                      [2 * (qy * qx + q0 * qz), q0 * q0 - qx * qx + qy * qy - qz * qz, 2 * (qy * qz - q0 * qx)],
                      [2 * (qz * qx - q0 * qy), 2 * (qz * qy + q0 * qx), q0 * q0 - qx * qx - qy * qy + qz * qz]])
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.float64((dg * (dp @ R.T)).sum()) / np.float64((dp ** 2).sum()) if with_scale else 1.0
    return float(c), R, mu_g - c * (R @ mu_p), 0.0


def alignment(p, g, mode, method=umeyama):
    if mode in ("sim3", "se3"):
        return method(p, g, mode == "sim3")
    if mode == "scale":
        with np.errstate(invalid="ignore", divide="ignore"):
            c = np.float64((g * p).sum()) / np.float64((p * p).sum())
        return float(c), np.eye(3), np.zeros(3), 1.0
    assert mode == "none"
    return 1.0, np.eye(3), np.zeros(3), 1.0


def evaluate(steps, gt, lengths, step, mode, method=umeyama, extra=None):
    """Every output of `evaluation.pose_trajectory` as numpy arrays, plus `branch` (the sign Umeyama's S33 took) and
    `sigma_g`.  `extra` (a 4x4 rigid transform) is applied to the aligned trajectory before the sub-sequence errors."""
    steps = np.asarray(steps).reshape(-1, 4, 4)
    J = steps.shape[0]
    F = J + 1
    C = trajectory(steps)
    G = gt_trajectory(gt, F)
    p, g = C[:, :3, 3], G[:, :3, 3]
    dist = path_length(g)
    c, R, t, branch = alignment(p, g, mode, method)
    aligned = np.tile(np.eye(4), (F, 1, 1))
    aligned[:, :3, :3] = R @ C[:, :3, :3]
    aligned[:, :3, 3] = c * (p @ R.T) + t
    e = np.linalg.norm(aligned[:, :3, 3] - g, axis=1)
    transform = np.eye(4)
    transform[:3, :3], transform[:3, 3] = R, t
    scored = aligned if extra is None else np.stack([extra @ a for a in aligned])
    firsts = list(range(0, F, step))
    pairs = np.zeros((len(firsts), len(lengths), 4))
    cosines = np.full((len(firsts), len(lengths)), np.nan)
    for a, first in enumerate(firsts):
        for b, L in enumerate(lengths):
            last = next((i for i in range(first, F) if dist[i] > dist[first] + L), -1)
            if last < 0:
                pairs[a, b] = (-1, np.nan, np.nan, 0)
                continue
            dG = np.linalg.inv(G[first]) @ G[last]
            if np.isnan(c):                  # every number that depends on the scale is NaN
                pairs[a, b] = (last, np.nan, np.nan, 0)
                continue
            dP = np.linalg.inv(scored[first]) @ scored[last]
            E = np.linalg.inv(dP) @ dG
            cosines[a, b] = 0.5 * (E[0, 0] + E[1, 1] + E[2, 2] - 1)
            pairs[a, b] = (last, np.linalg.norm(E[:3, 3]) / L, np.arccos(np.clip(cosines[a, b], -1, 1)) / L, 0)
    valid = pairs[:, :, 0] >= 0

    def mean(x):
        return float(np.mean(x)) if x.size else np.nan

    per_length = np.array([[mean(pairs[valid[:, b], b, 1]), mean(pairs[valid[:, b], b, 2]), valid[:, b].sum()]
                           for b in range(len(lengths))], np.float64)
    summary = np.array([mean(pairs[valid][:, 1]), mean(pairs[valid][:, 2]), valid.sum(), np.sqrt(np.mean(e ** 2)),
                        np.mean(e), np.max(e) if not np.isnan(e).any() else np.nan, c, F], np.float64)
    return {"traj": C, "gt_traj": G, "aligned": aligned, "transform": transform, "dist": dist, "pairs": pairs,
            "per_length": per_length, "summary": summary, "branch": branch, "cosines": cosines,
            "sigma_g": float(np.sqrt(((g - g.mean(0)) ** 2).sum(1).mean()))}
