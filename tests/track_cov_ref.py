"""Test-only fp64 numpy restatement of the tracking covariances (include/suo_hip.h: suo_tracking_covariances), sharing no code with the library: Jacobians by
CENTRAL DIFFERENCES of tests/pose_cov_ref.residual (J_o is taken for the fixed objects too), Ad(T) from tests/pose_cov_pairs_ref.adjoint, np.linalg.inv.

The differences are those of pose_cov_ref.edge_jacobians at two larger steps, Richardson-extrapolated (edge_jacobians below).  At that function's own step of 1e-6
the rounding of the residual leaves eps / STEP = 2e-10 of relative error in J and twice that in Hcc^-1.  The derived tolerance 1e3 eps cond(Hcc) is 2e-11 .. 1e-10
for the 6x6 block of a camera that sees several objects (cond 1e2 .. 5e2; the coupled systems of the older tests have cond 1e5 and more), so that reference
would be less exact than the bound it is used under: the first device run measured error / tolerance 0.89 (16 objects) and 1.5 (64 objects) on fixed_map_cov, which
has the bits of suo_pose_covariances.  With steps 3e-4 and 6e-4 the rounding is eps / h = 7e-13 and the extrapolated truncation h^4 f^(5) / 30 is below it;
tests/test_track_cov_ref.py holds the two functions together.

    P_c = Hcc^-1 + G Sigma G^T,   G = Hcc^-1 [B_c1 ... B_cn],   B_co = sum of J_c^T Omega J_o over the counted edges of (c, o)
    Sigma_co = -(G Sigma)[:, o],   rel_co = P_c + A Sigma_oo A^T + Sigma_co A^T + A Sigma_oc,   A = Ad(T_c)

A graph is the dict of tests/pose_cov_ref.py with every object fixed; map_cov [6 O, 6 O] is read by its upper triangle, and an object whose block has NaN at (0, 0)
is not in the map."""
import numpy as np

from tests import pose_cov_pairs_ref as PR
from tests import pose_cov_ref as R


STEP = 3e-4


def edge_jacobians(g, e):
    """(J_cam [2,6], J_obj [2,6]) of edge e: (4 D(h) - D(2 h)) / 3 of the central differences D of pose_cov_ref.residual under the left update"""
    Tc, To = R.to4(g["cam_T"][g["edge_cam"][e]]), R.to4(g["obj_T"][g["edge_obj"][e]])
    k, p, uv = g["edge_camk"][e], g["edge_p"][e], g["edge_uv"][e]

    def diff(h):
        Jc, Jo = np.zeros((2, 6)), np.zeros((2, 6))
        for i in range(6):
            d = np.zeros(6)
            d[i] = h
            Jc[:, i] = (R.residual(R.exp_se3(d) @ Tc, To, k, p, uv) - R.residual(R.exp_se3(-d) @ Tc, To, k, p, uv)) / (2 * h)
            Jo[:, i] = (R.residual(Tc, R.exp_se3(d) @ To, k, p, uv) - R.residual(Tc, R.exp_se3(-d) @ To, k, p, uv)) / (2 * h)
        return Jc, Jo
    (c1, o1), (c2, o2) = diff(STEP), diff(2 * STEP)
    return (4 * c1 - c2) / 3, (4 * o1 - o2) / 3


def mirrored_map(map_cov, n_obj):
    """(Sigma [6 O, 6 O] from the upper triangle, rows and columns of the objects that are not in the map zeroed; in_map [O])"""
    M = np.asarray(map_cov, float).reshape(6 * n_obj, 6 * n_obj)
    in_map = np.array([not np.isnan(M[6 * o, 6 * o]) for o in range(n_obj)], bool)
    S = np.triu(M) + np.triu(M, 1).T
    out = np.repeat(~in_map, 6)
    S[out, :] = 0.0
    S[:, out] = 0.0
    return S, in_map


def tracking(g, map_cov):
    """dict: cam_cov / fixed_map_cov [C,6,6], cross / rel [C,O,6,6], status [2] = NaN cameras, objects not in the map; and, per camera, what the derived
    tolerances of tests/test_gpu_track_cov.py are made of: cond [C] = cond(Hcc), hinv_max [C] = max|Hcc^-1|, gsg_max [C] = max(|G| |Sigma| |G|^T),
    gs_max [C] = max(|G| |Sigma|), a_max [C] = max|Ad(T_c)| (ones / zeros for a fixed camera)."""
    C, O, E = len(g["cam_T"]), len(g["obj_T"]), len(g["edge_cam"])
    assert np.asarray(g["obj_fixed"]).all(), "the tracking graph holds every object fixed"
    S, in_map = mirrored_map(map_cov, O)
    out = {"cam_cov": np.zeros((C, 6, 6)), "fixed_map_cov": np.zeros((C, 6, 6)), "cross": np.zeros((C, O, 6, 6)), "rel": np.zeros((C, O, 6, 6)),
           "cond": np.ones(C), "hinv_max": np.zeros(C), "gsg_max": np.zeros(C), "gs_max": np.zeros(C), "a_max": np.zeros(C)}
    n_nan = 0
    for c in range(C):
        A = PR.adjoint(R.to4(g["cam_T"][c]))
        out["a_max"][c] = np.abs(A).max()
        Hinv, G = np.zeros((6, 6)), np.zeros((6, 6 * O))
        if not g["cam_fixed"][c]:
            counted = [e for e in range(E) if g["edge_inlier"][e] and g["edge_cam"][e] == c and in_map[g["edge_obj"][e]]]
            if not counted:
                for k in ("cam_cov", "fixed_map_cov", "cross", "rel"):
                    out[k][c] = np.nan
                n_nan += 1
                continue
            H, B = np.zeros((6, 6)), np.zeros((6, 6 * O))
            for e in counted:
                Jc, Jo = edge_jacobians(g, e)
                i, o = g["edge_info"][e], int(g["edge_obj"][e])
                Om = np.array([[i[0], i[1]], [i[1], i[2]]])
                H += Jc.T @ Om @ Jc
                B[:, 6 * o:6 * o + 6] += Jc.T @ Om @ Jo
            Hinv = np.linalg.inv(H)
            G = Hinv @ B
            out["cond"][c] = np.linalg.cond(H)
        Z = G @ S
        P = Hinv + Z @ G.T
        out["fixed_map_cov"][c], out["cam_cov"][c] = Hinv, 0.5 * (P + P.T)
        out["hinv_max"][c] = np.abs(Hinv).max()
        out["gsg_max"][c] = (np.abs(G) @ np.abs(S) @ np.abs(G).T).max()
        out["gs_max"][c] = (np.abs(G) @ np.abs(S)).max() if O else 0.0
        for o in range(O):
            if not in_map[o]:
                out["cross"][c, o] = out["rel"][c, o] = np.nan
                continue
            X = -Z[:, 6 * o:6 * o + 6]
            Soo = S[6 * o:6 * o + 6, 6 * o:6 * o + 6]
            rel = P + A @ Soo @ A.T + X @ A.T + A @ X.T
            out["cross"][c, o], out["rel"][c, o] = X, 0.5 * (rel + rel.T)
    out["status"] = np.array([n_nan, int((~in_map).sum())])
    return out
