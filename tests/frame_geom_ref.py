"""What the frame chain has to stage and decide, in mpmath at 60 digits on the exact float32 / fp64 inputs, restated from the reference's rules and not from
csrc/frame_geom.hip:

compaction     `exp_uv[k][kp_mask]`, `cov_uv[k][kp_mask]`, `model_kps[k][kp_mask].astype(np.float64)` (lib/object_slam.py:1124-1137): a keypoint counts when
               its mask byte is non-zero; boolean indexing keeps ascending slot order.
normalisation  `points_2d @ KinvT[:2,:2] + KinvT[2:3,:2]` (:34-36), KinvT given (the host inverts K_bbox): ys = (u k0 + v k1 + k2, u k3 + v k4 + k5), exact.
information    `Inf = np.linalg.inv(cov_uv[k])`, `np.eye(2)` without network covariance (:825-828): the inverse by LU in mp (no closed form), of which g2o's
               chi2 = e' Inf e sees the symmetric part (xx, (xy + yx) / 2, yy).
measurement    the project's rule where the reference raises (include/suo_hip.h, suo_frame_geom_launch): with use_cov a keypoint whose covariance has a
               determinant that is not finite or is <= 0 is not a measurement and counts as masked out.  det of four float32 entries is exact here; the kernel's
               fp64 det is that value rounded once, which keeps its sign and cannot reach 0 or infinity from finite float32 entries, so both agree on every input.
acceptance     `ret_pnp is not None and T_OtoC[2,3] > 0.5 * diameter and count >= 4` (:31, :38, :1145-1148) on the PnP result the caller passes in.
graph          one vertex per crop, fixed unless accepted; one edge per counted keypoint of an accepted crop (:795-837); crop `lane` of a frame owns slots
               lane * 41 ... of its frame."""
from __future__ import annotations

import mpmath as mp
import numpy as np

DPS = 60
NUM_KP = 41
U = mp.mpf(2) ** -53


def _m(x):
    return mp.mpf(float(x))


def is_measurement(cov):
    """cov: 2x2 float32.  The rule above, exact."""
    v = [float(x) for x in np.asarray(cov, np.float32).reshape(4)]
    if not all(np.isfinite(v)):
        return False
    with mp.workdps(DPS):
        a, b, c, d = (_m(x) for x in v)
        return bool(a * d - b * c > 0)


def information(cov):
    """inv(cov) as a full 2x2 mp matrix, by LU."""
    with mp.workdps(DPS):
        M = mp.matrix([[_m(cov[0][0]), _m(cov[0][1])], [_m(cov[1][0]), _m(cov[1][1])]])
        return mp.inverse(M)


def stage(uv, cov, mask, model_kps, kinv, camk, use_cov=True):
    """One launch's staging.  uv [L,41,2] f32, cov [L,41,2,2] f32, mask [L,41] (any integer type), model_kps [L,41,3] f32, kinv [L,6], camk [L,4] f64.
    Returns a dict: valid [L,41] bool, n [L], idx (per crop the counted slots, ascending), xs / edge_uv / edge_k: float64 arrays [L,41,.] with the counted
    keypoints compacted to the front (exact: widening only; NaN behind them), ys / info: [L][n] lists of mp tuples, ys_bound / ixy_bound: the derived error
    bounds of the issue as floats, det [L][n] mp."""
    L = len(mask)
    with mp.workdps(DPS):
        valid = np.zeros((L, NUM_KP), bool)
        out = {"xs": np.full((L, NUM_KP, 3), np.nan), "edge_uv": np.full((L, NUM_KP, 2), np.nan), "edge_k": np.full((L, NUM_KP, 4), np.nan), "ys": [], "info": [],
               "ys_bound": [], "ixy_bound": [], "idx": []}
        for l in range(L):
            for k in range(NUM_KP):
                valid[l, k] = mask[l][k] != 0 and (not use_cov or is_measurement(cov[l][k]))
            idx = [k for k in range(NUM_KP) if valid[l, k]]
            ys, info, yb, ib = [], [], [], []
            for j, k in enumerate(idx):
                out["xs"][l, j] = model_kps[l][k].astype(np.float64)
                out["edge_uv"][l, j] = uv[l][k].astype(np.float64)
                out["edge_k"][l, j] = camk[l]
                u, v = _m(uv[l][k][0]), _m(uv[l][k][1])
                kk = [_m(x) for x in kinv[l]]
                ys.append((u * kk[0] + v * kk[1] + kk[2], u * kk[3] + v * kk[4] + kk[5]))
                yb.append((float(3 * U * (abs(u * kk[0]) + abs(v * kk[1]) + abs(kk[2]))), float(3 * U * (abs(u * kk[3]) + abs(v * kk[4]) + abs(kk[5])))))
                if use_cov:
                    I = information(cov[l][k])
                    info.append((I[0, 0], (I[0, 1] + I[1, 0]) / 2, I[1, 1]))
                    a, b, c, d = (_m(x) for x in np.asarray(cov[l][k]).reshape(4))
                    ib.append(float(4 * U * (abs(b) + abs(c)) / (2 * abs(a * d - b * c))))
                else:
                    info.append((mp.mpf(1), mp.mpf(0), mp.mpf(1)))
                    ib.append(0.0)
            out["idx"].append(idx)
            out["ys"].append(ys); out["info"].append(info); out["ys_bound"].append(yb); out["ixy_bound"].append(ib)
        out["valid"] = valid
        out["n"] = valid.sum(1).astype(np.int32)
        return out


def accept(n, status, T_pnp, min_depth):
    """[L] bool: the acceptance rule on a PnP result (status 1 = the identity pose = `pnp() returned None`)."""
    return np.array([bool(status[l] == 0 and n[l] >= 4 and T_pnp[l][2][3] > min_depth[l]) for l in range(len(n))])


def graph(frame_first, n, accepted):
    """pair_start, pair_end, obj_fixed [L] and header [F,4] = n_cam, n_obj, n_edge, n_pair."""
    L = len(n)
    ps, pe, fx, hdr = np.zeros(L, np.int32), np.zeros(L, np.int32), np.zeros(L, bool), []
    for f in range(len(frame_first) - 1):
        g0, g1 = int(frame_first[f]), int(frame_first[f + 1])
        for g in range(g0, g1):
            ps[g] = (g - g0) * NUM_KP
            pe[g] = ps[g] + (int(n[g]) if accepted[g] else 0)
            fx[g] = not accepted[g]
        hdr.append([1, g1 - g0, int(sum(int(n[g]) for g in range(g0, g1) if accepted[g])), g1 - g0])
    return ps, pe, fx, np.array(hdr, np.int32).reshape(-1, 4)
