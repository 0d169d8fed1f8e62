"""Test-only fp64 numpy reference of the pairs of suo_pose_covariances_graph (include/suo_hip.h), sharing no code with the library.  (camera a, camera b): the
relative pose is T_b T_a^-1, the joint 12x12 of the two cameras is cut out of tests/pose_cov_ref.py's dense Sigma (zeros for a fixed vertex), the Jacobian comes from
CENTRAL DIFFERENCES of log_se3(T_rel' T_rel^-1) (step 1e-6) -- not the adjoint formula --, and the result is J Sigma_joint J^T.  Every other pair is
tests/pose_cov_pairs_ref.py's.  Vertices are coded as the library codes them: camera c is c, object o is n_cam + o."""
import numpy as np

from tests import pose_cov_pairs_ref as PR
from tests import pose_cov_ref as R
from tests.pose_cov_pairs_ref import _columns, adjoint, log_se3      # noqa: F401  (adjoint: for the tests, not for relative())
from tests.pose_cov_ref import exp_se3

STEP = 1e-6


def camera_pair_pose(Ta, Tb):
    return Tb @ np.linalg.inv(Ta)


def camera_pair_jacobian(Ta, Tb):
    """[6,12]: d delta_rel / d (delta_a, delta_b) by central differences, delta_rel = log_se3(T_rel' T_rel^-1), T_rel = T_b T_a^-1"""
    inv0 = np.linalg.inv(camera_pair_pose(Ta, Tb))
    J = np.zeros((6, 12))
    for i in range(12):
        d = np.zeros(6)
        d[i % 6] = STEP
        p, m = exp_se3(d), exp_se3(-d)
        Tp = camera_pair_pose(p @ Ta, Tb) if i < 6 else camera_pair_pose(Ta, p @ Tb)
        Tm = camera_pair_pose(m @ Ta, Tb) if i < 6 else camera_pair_pose(Ta, m @ Tb)
        J[:, i] = (log_se3(Tp @ inv0) - log_se3(Tm @ inv0)) / (2 * STEP)
    return J


def relative(g, ref, pairs):
    """(cross [P,6,6], rel [P,6,6], number of NaN pairs) of the vertex pairs [P,2] of graph g whose pose_cov_ref.covariances(g) is ref; (camera, camera) allowed"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    C = len(g["cam_T"])
    both = (pairs[:, 0] < C) & (pairs[:, 1] < C)
    cross, rel = np.zeros((len(pairs), 6, 6)), np.zeros((len(pairs), 6, 6))
    cross[~both], rel[~both], n_nan = PR.relative(g, ref, pairs[~both])
    col = _columns(g, ref)
    S = ref["Sigma"]
    for q in np.nonzero(both)[0]:
        a, b = int(pairs[q, 0]), int(pairs[q, 1])
        if col[a] == "nan" or col[b] == "nan":
            cross[q] = rel[q] = np.nan
            n_nan += 1
            continue
        joint = np.zeros((12, 12))
        for i, u in enumerate((a, b)):
            for j, w in enumerate((a, b)):
                if col[u] is not None and col[w] is not None:
                    joint[6 * i:6 * i + 6, 6 * j:6 * j + 6] = S[col[u]:col[u] + 6, col[w]:col[w] + 6]
        J = camera_pair_jacobian(R.to4(g["cam_T"][a]), R.to4(g["cam_T"][b]))
        cross[q] = joint[:6, 6:]
        rel[q] = J @ joint @ J.T
    return cross, rel, n_nan
