"""Test-only fp64 numpy reference of suo_residual_statistics (include/suo_hip.h), sharing no code with the library: built on tests/pose_cov_ref.py -- covariances(g)
(the dense Sigma = inv(H)), edge_jacobians (central differences) and residual.  Every quantity of the header's definitions, the two NaN rules included, plus what the
tests need to derive their tolerances (the Jacobians, det R_e, the stacked design matrix)."""
import numpy as np

from tests import pose_cov_ref as R

MIN_DET = 1e-9          # the no-redundancy rule of the header: part of the definition


def columns(g):
    """(col, n, counted): the column of every vertex in the system, as pose_cov_ref.covariances deals them (cameras, then objects; free vertices a counted edge
    reaches), the number of rows of H, and the counted flag of every edge"""
    C, O, E = len(g["cam_T"]), len(g["obj_T"]), len(g["edge_cam"])
    cfix, ofix = np.asarray(g["cam_fixed"]).astype(bool), np.asarray(g["obj_fixed"]).astype(bool)
    counted = np.array([bool(g["edge_inlier"][e]) and not (cfix[g["edge_cam"][e]] and ofix[g["edge_obj"][e]]) for e in range(E)], bool)
    col, n = {}, 0
    for c in range(C):
        if not cfix[c] and counted[np.asarray(g["edge_cam"]) == c].any():
            col[("c", c)] = n
            n += 6
    for o in range(O):
        if not ofix[o] and counted[np.asarray(g["edge_obj"]) == o].any():
            col[("o", o)] = n
            n += 6
    return col, n, counted


def statistics(g, ref=None):
    """dict of every output of the entry (edge_chi2, edge_pcov, edge_lev, edge_t, cam_stat, obj_stat, summary, status) and, for the tolerances: J [E,2,12] (zero
    columns for a fixed vertex), v [E,2], det [E] = det(I + s P Omega) (NaN on a NaN vertex), counted [E], A [2m,n] / W [2m,2m] the stacked design of the counted edges"""
    ref = R.covariances(g) if ref is None else ref
    C, O, E = len(g["cam_T"]), len(g["obj_T"]), len(g["edge_cam"])
    cfix, ofix = np.asarray(g["cam_fixed"]).astype(bool), np.asarray(g["obj_fixed"]).astype(bool)
    col, n, counted = columns(g)
    assert n == ref["H"].shape[0]
    Sigma = ref["Sigma"]
    chi2, pcov, lev, t, det = np.zeros(E), np.zeros((E, 3)), np.zeros(E), np.zeros(E), np.zeros(E)
    J12, V = np.zeros((E, 2, 12)), np.zeros((E, 2))
    rows, n_nan, n_nored = [], 0, 0
    for e in range(E):
        c, o = int(g["edge_cam"][e]), int(g["edge_obj"][e])
        Jc, Jo = R.edge_jacobians(g, e)
        if cfix[c]:
            Jc = np.zeros((2, 6))
        if ofix[o]:
            Jo = np.zeros((2, 6))
        J12[e] = np.c_[Jc, Jo]
        v = R.residual(R.to4(g["cam_T"][c]), R.to4(g["obj_T"][o]), g["edge_camk"][e], g["edge_p"][e], g["edge_uv"][e])
        V[e] = v
        i = g["edge_info"][e]
        Om = np.array([[i[0], i[1]], [i[1], i[2]]])
        chi2[e] = v @ Om @ v
        if (not cfix[c] and ("c", c) not in col) or (not ofix[o] and ("o", o) not in col):       # a vertex that is NaN in the marginal call
            pcov[e], lev[e], t[e], det[e] = np.nan, np.nan, np.nan, np.nan
            n_nan += 1
            continue
        J = np.zeros((2, n))
        if ("c", c) in col:
            J[:, col[("c", c)]:col[("c", c)] + 6] = Jc
        if ("o", o) in col:
            J[:, col[("o", o)]:col[("o", o)] + 6] = Jo
        if counted[e]:
            rows.append((J, Om))
        P = J @ Sigma @ J.T
        P = 0.5 * (P + P.T)
        pcov[e] = P[0, 0], P[0, 1], P[1, 1]
        lev[e] = np.trace(P @ Om)
        s = -1.0 if counted[e] else 1.0
        Rm = np.eye(2) + s * P @ Om
        det[e] = np.linalg.det(Rm)
        if det[e] <= MIN_DET or Rm[0, 0] <= 0 or Rm[1, 1] <= 0:
            t[e] = np.nan
            n_nored += 1
        else:
            t[e] = v @ np.linalg.solve(np.linalg.inv(Om) + s * P, v)
    ec, eo = np.asarray(g["edge_cam"]), np.asarray(g["edge_obj"])

    def vertex(mask):
        k = np.flatnonzero(mask & counted)
        return [len(k), chi2[k].sum(), (2.0 - lev[k]).sum()]
    cam_stat = np.array([vertex(ec == c) for c in range(C)], float).reshape(C, 3)
    obj_stat = np.array([vertex(eo == o) for o in range(O)], float).reshape(O, 3)
    m = int(counted.sum())
    dof = 2 * m - n
    any_nan = bool(np.isnan(lev[counted]).any())
    s0 = chi2[counted].sum() / dof if dof > 0 and not any_nan else np.nan
    summary = np.array([m, n, chi2[counted].sum(), lev[counted].sum(), dof, s0], float)
    A = np.vstack([r[0] for r in rows]) if rows else np.zeros((0, n))
    W = np.zeros((2 * len(rows), 2 * len(rows)))
    for k, r in enumerate(rows):
        W[2 * k:2 * k + 2, 2 * k:2 * k + 2] = r[1]
    return {"edge_chi2": chi2, "edge_pcov": pcov, "edge_lev": lev, "edge_t": t, "cam_stat": cam_stat, "obj_stat": obj_stat, "summary": summary,
            "status": np.array(list(ref["status"]) + [n_nan, n_nored]), "J": J12, "v": V, "det": det, "counted": counted, "A": A, "W": W}
