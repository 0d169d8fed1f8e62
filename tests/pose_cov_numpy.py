"""Test-only float64 numpy restatement of the covariance entries of include/suo_hip.h with ANALYTIC Jacobians and the header's adjoint formulas, on two routes:
"dense" (one Cholesky of the whole H, inverted by substitution) and "schur" (the coupled kernels' route: S = Hoo - sum_c Hco^T Hcc^-1 Hco, Sigma_OO = S^-1,
Sigma_cc' = [c == c'] Hcc^-1 + Y_c Sigma_OO Y_c'^T, Sigma_cO = -Y_c Sigma_OO).  tests/test_pose_cov_mp_ref.py measures it against tests/pose_cov_mp_ref.py: that
is where K_REF, and with it the kernels' tolerance, comes from.  It shares no code with the mp reference, the finite-difference references or the library."""
import numpy as np

MIN_DET = 1e-9


def _skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def _to4(T34):
    T = np.eye(4)
    T[:3] = np.asarray(T34, float).reshape(3, 4)
    return T


def adjoint(T):
    A = np.zeros((6, 6))
    A[:3, :3] = A[3:, 3:] = T[:3, :3]
    A[3:, :3] = _skew(T[:3, 3]) @ T[:3, :3]
    return A


def chol_inv(A):
    """A^-1 of a symmetric positive definite A through its Cholesky factor: L^-1 by forward substitution, L^-T L^-1."""
    n = len(A)
    L = np.linalg.cholesky(A)
    Y = np.zeros((n, n))
    for i in range(n):
        e = np.zeros(n)
        e[i] = 1.0
        Y[i] = (e - L[i, :i] @ Y[:i]) / L[i, i]
    return Y.T @ Y


def edge_terms(g, e):
    """(v [2], J_c [2,6], J_o [2,6], Omega [2,2]) of edge e: v = uv - pi(T_c T_o p), the Jacobians of v under the left update exp(delta) T, delta = [omega, upsilon]"""
    Tc, To = _to4(g["cam_T"][g["edge_cam"][e]]), _to4(g["obj_T"][g["edge_obj"][e]])
    k, p, uv = g["edge_camk"][e], g["edge_p"][e], g["edge_uv"][e]
    qw = To[:3, :3] @ p + To[:3, 3]
    qc = Tc[:3, :3] @ qw + Tc[:3, 3]
    x, y, z = qc
    v = np.asarray(uv, float) - np.array([k[0] * x / z + k[2], k[1] * y / z + k[3]])
    D = -np.array([[k[0] / z, 0.0, -k[0] * x / (z * z)], [0.0, k[1] / z, -k[1] * y / (z * z)]])
    Jc = D @ np.hstack([-_skew(qc), np.eye(3)])
    Jo = D @ Tc[:3, :3] @ np.hstack([-_skew(qw), np.eye(3)])
    i = g["edge_info"][e]
    return v, Jc, Jo, np.array([[i[0], i[1]], [i[1], i[2]]], float)


class NumpyCov:
    def __init__(self, g, route):
        self.g, self.route = g, route
        C, O, E = len(g["cam_T"]), len(g["obj_T"]), len(g["edge_cam"])
        self.C, self.O, self.E = C, O, E
        self.fixed = np.r_[np.asarray(g["cam_fixed"]).astype(bool), np.asarray(g["obj_fixed"]).astype(bool)]
        ec, eo = np.asarray(g["edge_cam"], int), np.asarray(g["edge_obj"], int)
        self.counted = np.array([g["edge_inlier"][e] == 1 and not (self.fixed[ec[e]] and self.fixed[C + eo[e]]) for e in range(E)], bool)
        self.terms = [edge_terms(g, e) for e in range(E)]
        hit = set(ec[self.counted].tolist()) | set((C + eo[self.counted]).tolist())
        self.col, n = {}, 0
        for v in range(C + O):
            self.col[v] = None if self.fixed[v] else ("nan" if v not in hit else n)
            if isinstance(self.col[v], int):
                n += 6
        self.n = n
        H = np.zeros((n, n))
        for e in np.flatnonzero(self.counted):
            _, Jc, Jo, Om = self.terms[e]
            J = np.zeros((2, n))
            if isinstance(self.col[ec[e]], int):
                J[:, self.col[ec[e]]:self.col[ec[e]] + 6] = Jc
            if isinstance(self.col[C + eo[e]], int):
                J[:, self.col[C + eo[e]]:self.col[C + eo[e]] + 6] = Jo
            H += J.T @ Om @ J
        self.H = H
        cams = [c for c in range(C) if isinstance(self.col[c], int)]
        objs = [o for o in range(O) if isinstance(self.col[C + o], int)]
        if n == 0:
            self.Sigma = np.zeros((0, 0))
        elif route == "dense":
            self.Sigma = chol_inv(H)
        elif not cams or not objs:
            self.Sigma = np.zeros((n, n))
            for v in cams + [C + o for o in objs]:
                i = self.col[v]
                self.Sigma[i:i + 6, i:i + 6] = chol_inv(H[i:i + 6, i:i + 6])
        else:
            o0 = self.col[C + objs[0]]
            S, Y, Ainv = H[o0:, o0:].copy(), {}, {}
            for c in cams:
                i = self.col[c]
                Ainv[c] = chol_inv(H[i:i + 6, i:i + 6])
                Y[c] = Ainv[c] @ H[i:i + 6, o0:]
                S -= H[i:i + 6, o0:].T @ Y[c]
            SOO = chol_inv(S)
            Sig = np.zeros((n, n))
            Sig[o0:, o0:] = SOO
            for c in cams:
                i = self.col[c]
                Z = Y[c] @ SOO
                Sig[i:i + 6, o0:], Sig[o0:, i:i + 6] = -Z, -Z.T
                for c2 in cams:
                    j = self.col[c2]
                    Sig[i:i + 6, j:j + 6] = Z @ Y[c2].T + (Ainv[c] if c == c2 else 0.0)
            self.Sigma = Sig

    def block(self, u, w):
        i, j = self.col[u], self.col[w]
        if i == "nan" or j == "nan":
            return np.full((6, 6), np.nan)
        if i is None or j is None:
            return np.zeros((6, 6))
        return self.Sigma[i:i + 6, j:j + 6]

    def marginals(self):
        C, O = self.C, self.O
        return np.array([self.block(c, c) for c in range(C)]).reshape(C, 6, 6), np.array([self.block(C + o, C + o) for o in range(O)]).reshape(O, 6, 6)

    def pose(self, v):
        return _to4(self.g["cam_T"][v] if v < self.C else self.g["obj_T"][v - self.C])

    def pairs(self, pairs):
        """(cross, rel) [P,6,6] by the header's adjoint formulas"""
        C = self.C
        cross, rel = np.zeros((len(pairs), 6, 6)), np.zeros((len(pairs), 6, 6))
        for q, (a, b) in enumerate(np.asarray(pairs, int).tolist()):
            Saa, Sbb, Sab = self.block(a, a), self.block(b, b), self.block(a, b)
            cross[q] = Sab
            if np.isnan(Saa).any() or np.isnan(Sbb).any():
                cross[q] = rel[q] = np.nan
            elif a == b:
                rel[q] = 0.0
            elif a < C and b < C:
                A = adjoint(self.pose(b) @ np.linalg.inv(self.pose(a)))
                rel[q] = Sbb + A @ Saa @ A.T - A @ Sab - Sab.T @ A.T
            elif a < C or b < C:
                (c, o, Sco) = (a, b, Sab) if a < C else (b, a, Sab.T)
                A = adjoint(self.pose(c))
                rel[q] = self.block(c, c) + A @ self.block(o, o) @ A.T + Sco @ A.T + A @ Sco.T
            else:
                Bm = adjoint(np.linalg.inv(self.pose(b)))
                rel[q] = Bm @ (Saa + Sbb - Sab - Sab.T) @ Bm.T
            rel[q] = 0.5 * (rel[q] + rel[q].T)
        return cross, rel

    def statistics(self):
        """dict of the outputs of suo_residual_statistics by the header's formulas"""
        C, O, E, g = self.C, self.O, self.E, self.g
        chi2, pcov, lev, t = np.zeros(E), np.zeros((E, 3)), np.zeros(E), np.zeros(E)
        for e in range(E):
            v, Jc, Jo, Om = self.terms[e]
            c, o = int(g["edge_cam"][e]), C + int(g["edge_obj"][e])
            chi2[e] = v @ Om @ v
            if self.col[c] == "nan" or self.col[o] == "nan":
                pcov[e], lev[e], t[e] = np.nan, np.nan, np.nan
                continue
            J = np.hstack([np.zeros((2, 6)) if self.fixed[c] else Jc, np.zeros((2, 6)) if self.fixed[o] else Jo])
            Sj = np.block([[self.block(c, c), self.block(c, o)], [self.block(o, c), self.block(o, o)]])
            P = J @ Sj @ J.T
            P = 0.5 * (P + P.T)
            pcov[e] = P[0, 0], P[0, 1], P[1, 1]
            lev[e] = P[0, 0] * Om[0, 0] + 2 * P[0, 1] * Om[0, 1] + P[1, 1] * Om[1, 1]
            s = -1.0 if self.counted[e] else 1.0
            Rm = np.eye(2) + s * P @ Om
            det = Rm[0, 0] * Rm[1, 1] - Rm[0, 1] * Rm[1, 0]
            if det <= MIN_DET or Rm[0, 0] <= 0 or Rm[1, 1] <= 0:
                t[e] = np.nan
            else:
                Ri = np.array([[Rm[1, 1], -Rm[0, 1]], [-Rm[1, 0], Rm[0, 0]]]) / det
                t[e] = (Om @ v) @ (Ri @ v)
        cnt = self.counted

        def vertex(mask):
            k = np.flatnonzero(mask & cnt)
            return [len(k), chi2[k].sum(), (2.0 - lev[k]).sum()]
        ec, eo = np.asarray(g["edge_cam"], int), np.asarray(g["edge_obj"], int)
        m = int(cnt.sum())
        dof = 2 * m - self.n
        s0 = chi2[cnt].sum() / dof if dof > 0 and not np.isnan(lev[cnt]).any() else np.nan
        return {"edge_chi2": chi2, "edge_pcov": pcov, "edge_lev": lev, "edge_t": t, "cam_stat": np.array([vertex(ec == c) for c in range(C)], float).reshape(C, 3),
                "obj_stat": np.array([vertex(eo == o) for o in range(O)], float).reshape(O, 3), "summary": np.array([m, self.n, chi2[cnt].sum(), lev[cnt].sum(), dof, s0])}


def tracking(g, map_cov):
    """dict: cam_cov, fixed_map_cov [C,6,6], cross, rel [C,O,6,6] by the header's formulas (one route: every camera is a 6x6 block of its own)"""
    C, O, E = len(g["cam_T"]), len(g["obj_T"]), len(g["edge_cam"])
    M = np.asarray(map_cov, float).reshape(6 * O, 6 * O)
    in_map = np.array([not np.isnan(M[6 * o, 6 * o]) for o in range(O)], bool)
    S = np.triu(M) + np.triu(M, 1).T
    S[np.repeat(~in_map, 6), :] = 0.0
    S[:, np.repeat(~in_map, 6)] = 0.0
    out = {"cam_cov": np.zeros((C, 6, 6)), "fixed_map_cov": np.zeros((C, 6, 6)), "cross": np.zeros((C, O, 6, 6)), "rel": np.zeros((C, O, 6, 6))}
    for c in range(C):
        A = adjoint(_to4(g["cam_T"][c]))
        Hinv, G = np.zeros((6, 6)), np.zeros((6, 6 * O))
        if not g["cam_fixed"][c]:
            counted = [e for e in range(E) if g["edge_inlier"][e] == 1 and g["edge_cam"][e] == c and in_map[g["edge_obj"][e]]]
            if not counted:
                for k in out:
                    out[k][c] = np.nan
                continue
            H, Bm = np.zeros((6, 6)), np.zeros((6, 6 * O))
            for e in counted:
                _, Jc, Jo, Om = edge_terms(g, e)
                o = int(g["edge_obj"][e])
                H += Jc.T @ Om @ Jc
                Bm[:, 6 * o:6 * o + 6] += Jc.T @ Om @ Jo
            Hinv = chol_inv(H)
            G = Hinv @ Bm
        Z = G @ S
        P = Hinv + Z @ G.T
        P = 0.5 * (P + P.T)
        out["fixed_map_cov"][c], out["cam_cov"][c] = Hinv, P
        for o in range(O):
            if not in_map[o]:
                out["cross"][c, o] = out["rel"][c, o] = np.nan
                continue
            X = -Z[:, 6 * o:6 * o + 6]
            rel = P + A @ S[6 * o:6 * o + 6, 6 * o:6 * o + 6] @ A.T + X @ A.T + A @ X.T
            out["cross"][c, o], out["rel"][c, o] = X, 0.5 * (rel + rel.T)
    return out
