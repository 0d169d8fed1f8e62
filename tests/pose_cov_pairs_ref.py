"""Test-only fp64 numpy reference of the cross blocks and relative-pose covariances of vertex pairs (include/suo_hip.h: suo_pose_covariances_pairs), sharing no
code with the library: the joint covariance of the two vertices is cut out of tests/pose_cov_ref.py's dense Sigma (zeros for a fixed vertex), the Jacobian of the
relative pose comes from CENTRAL DIFFERENCES of log_se3(T' T^-1) (step 1e-6) -- not the adjoint formulas --, and the result is J Sigma_joint J^T.

Vertices are coded as the library codes them: camera c is c, object o is n_cam + o.  Relative poses: (camera, object) in either order T_c T_o, (object a, object b)
T_b^-1 T_a; the perturbation of every pose is the left update exp(delta) T, delta = [omega, upsilon]."""
import numpy as np

from tests import pose_cov_ref as R

STEP = 1e-6


def log_se3(T):
    """4x4 -> [omega, upsilon], the inverse of pose_cov_ref.exp_se3; written for the small motions the differences produce (any angle below pi works)."""
    Rm, t = T[:3, :3], T[:3, 3]
    w = 0.5 * np.array([Rm[2, 1] - Rm[1, 2], Rm[0, 2] - Rm[2, 0], Rm[1, 0] - Rm[0, 1]])      # sin(theta) * axis
    s = float(np.linalg.norm(w))
    th = float(np.arctan2(s, 0.5 * (np.trace(Rm) - 1.0)))                                     # (arccos loses half the digits next to 1)
    om = w * (th / s) if s > 1e-15 else w
    Om = R._skew(om)
    if th < 1e-3:
        b, c = 0.5 - th * th / 24.0, 1.0 / 6.0 - th * th / 120.0
    else:
        b, c = (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    V = np.eye(3) + b * Om + c * Om @ Om
    return np.r_[om, np.linalg.solve(V, t)]


def adjoint(T):
    """Ad(T) = [[R, 0], [[t]x R, R]] of a 4x4 pose, for the [omega, upsilon] ordering (the tests compare the differences with it; relative() does not use it)."""
    A = np.zeros((6, 6))
    A[:3, :3] = A[3:, 3:] = T[:3, :3]
    A[3:, :3] = R._skew(T[:3, 3]) @ T[:3, :3]
    return A


def vertex_pose(g, v):
    C = len(g["cam_T"])
    return R.to4(g["cam_T"][v]) if v < C else R.to4(g["obj_T"][v - C])


def relative_pose(Ta, Tb, a_cam, b_cam):
    if a_cam and b_cam:
        raise ValueError("(camera, camera) pairs are not defined")
    if a_cam:
        return Ta @ Tb
    if b_cam:
        return Tb @ Ta
    return np.linalg.inv(Tb) @ Ta


def relative_jacobian(Ta, Tb, a_cam, b_cam):
    """[6,12]: d delta_rel / d (delta_a, delta_b) by central differences, delta_rel = log_se3(T_rel' T_rel^-1)"""
    inv0 = np.linalg.inv(relative_pose(Ta, Tb, a_cam, b_cam))
    J = np.zeros((6, 12))
    for i in range(12):
        d = np.zeros(6)
        d[i % 6] = STEP
        p, m = R.exp_se3(d), R.exp_se3(-d)
        Tp = relative_pose(p @ Ta, Tb, a_cam, b_cam) if i < 6 else relative_pose(Ta, p @ Tb, a_cam, b_cam)
        Tm = relative_pose(m @ Ta, Tb, a_cam, b_cam) if i < 6 else relative_pose(Ta, m @ Tb, a_cam, b_cam)
        J[:, i] = (log_se3(Tp @ inv0) - log_se3(Tm @ inv0)) / (2 * STEP)
    return J


def _columns(g, ref):
    """vertex -> first column in ref["Sigma"] (cameras first, then objects, each in index order: pose_cov_ref.covariances), None: fixed, "nan": left out"""
    col, n = {}, 0
    blocks = [(c, bool(g["cam_fixed"][c]), ref["cam_cov"][c]) for c in range(len(g["cam_T"]))]
    blocks += [(len(g["cam_T"]) + o, bool(g["obj_fixed"][o]), ref["obj_cov"][o]) for o in range(len(g["obj_T"]))]
    for v, fixed, blk in blocks:
        if fixed:
            col[v] = None
        elif np.isnan(blk).any():
            col[v] = "nan"
        else:
            col[v] = n
            n += 6
    assert n == ref["Sigma"].shape[0]
    return col


def relative(g, ref, pairs):
    """(cross [P,6,6], rel [P,6,6], number of NaN pairs) of the vertex pairs [P,2] of graph g whose pose_cov_ref.covariances(g) is ref"""
    col = _columns(g, ref)
    C = len(g["cam_T"])
    S = ref["Sigma"]
    cross, rel = np.zeros((len(pairs), 6, 6)), np.zeros((len(pairs), 6, 6))
    n_nan = 0
    for q, (a, b) in enumerate(pairs):
        a, b = int(a), int(b)
        if col[a] == "nan" or col[b] == "nan":
            cross[q] = rel[q] = np.nan
            n_nan += 1
            continue
        joint = np.zeros((12, 12))
        for i, u in enumerate((a, b)):
            for j, w in enumerate((a, b)):
                if col[u] is not None and col[w] is not None:
                    joint[6 * i:6 * i + 6, 6 * j:6 * j + 6] = S[col[u]:col[u] + 6, col[w]:col[w] + 6]
        J = relative_jacobian(vertex_pose(g, a), vertex_pose(g, b), a < C, b < C)
        cross[q] = joint[:6, 6:]
        rel[q] = J @ joint @ J.T
    return cross, rel, n_nan
