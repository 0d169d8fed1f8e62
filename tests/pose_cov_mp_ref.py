"""The covariance entries of include/suo_hip.h -- suo_pose_covariances (_pairs, _graph), suo_residual_statistics, suo_tracking_covariances -- written from their
definitions in mpmath at 40 digits: the yardstick of tests/test_pose_cov_mp_ref.py (float64 numpy and the finite-difference references against it) and of the five
GPU modules of the family (the kernels against it).  A graph is the dict of tests/pose_cov_ref.py.

  H, Sigma     the per-edge J_c, J_o and J^T Omega J blocks are tests/ba_phases_ref.PhaseRef's (weight 1, no lambda), summed over the counted edges (edge_inlier == 1,
               the two vertices not both fixed); a free vertex without a counted edge has no row (its blocks are NaN), a fixed vertex is zeros.  Sigma = H^-1 by the
               structure: every object block inverted, the reduced CAMERA system Hcc - sum_o Hco Hoo^-1 Hco^T inverted, the blocks asked for back-substituted.  This is
               neither the kernels' route (they reduce onto the objects) nor a dense factorisation; dense() and objects_route() give those two for the CPU tests.
  pairs        cross = Sigma_ab; rel = J Sigma_joint J^T with J [6,12] the Jacobian of log(T_rel' T_rel^-1) by CENTRAL DIFFERENCES in mp (step 1e-15 at 60 digits),
               T_rel = T_c T_o, T_b^-1 T_a (objects), T_b T_a^-1 (cameras): no adjoint formula.  (a, a): the marginal block and 36 zeros.
  statistics   chi2_e, P_e = J_e Sigma_e J_e^T, lev_e = tr(P_e Omega_e), t_e = (Omega v)^T R^-1 v with R = I + s P Omega and the header's two NaN rules, the per-vertex
               triples, the summary.
  tracking     Hcc^-1, P_c = Hcc^-1 + G Sigma_OO G^T, cross = -(G Sigma_OO)[:, o], rel = J [[P_c, cross], [cross^T, Sigma_oo]] J^T with the same differenced J.

Error scales.  Next to every value stands a float64 magnitude M such that a careful fp64 evaluation errs by a few eps M (the convention of tests/ba_phases_ref.py);
the tolerance of a comparison is K[buffer] eps M, and an entry with M == 0 is a structural zero that must be met exactly.
  MH           the sum of |J|^T |Omega| |J| with every computed factor replaced by its magnitude sum (PhaseRef's MAcc / MAoo / MAco)
  M_Sigma      |Sigma| MH |Sigma|  +  |Sigma| sqrt(diag H (x) diag H) |Sigma|: the first-order effect of H's rounding, and of a Cholesky factorisation's backward error
  Schur route  the kernels' coupled forms go through Hcc^-1 per camera; M carries no cond(Hcc) term: see the note under K_REF
  rel          |J| M_joint |J|^T + |J| |Sigma_joint| |J|^T
  P_e          J Sigma is small where |J| |Sigma| is not (a rotation about the camera and the translation that undoes it), and Sigma's error is -Sigma dH Sigma: so
               |J Sigma| (MH + sqrt(dd^T)) |J Sigma|^T with the FULL rows of Sigma, + MJ |Sigma_e J^T| and its transpose (J's own error, MJ = PhaseRef's magnitude
               of J_e) + |J| |Sigma_e| |J|^T (the rounding of the products as they stand)
  lev          sum (M_P + |P|) |Omega|
  t            u = Omega v, w = R^-1 v: M_u |w| + |u| M_w + |u| |w|, M_u = |Omega| M_v, M_w = |R^-1| (M_v + M_R |w|), M_R = (M_P + |P|) |Omega| + |R| -- R^-1 in mp, so the
               scale grows as 1 / det R where an edge has little redundancy, and is finite wherever t is; an edge with both vertices fixed has P = 0 and
               t = chi2 to the bit: its tolerance is chi2's
  sums         the members' errors come from one Sigma and need not cancel: the tolerance of a sum is the sum of the members' tolerances plus the sum's own rounding,
               K eps (sum of the members' magnitudes); as ONE scale under the sums' K that is M = (K[member] / K[sum]) sum M_member + sum |member|.
               s0^2: that of sum chi2 over dof, plus |s0^2|
  tracking     M_A = |A| MH' |A| for A = Hcc^-1, MH' = MHcc + sqrt(dd^T).  dG = -A dH G keeps its structure, A dB and the product's rounding do not: with
               M_G2 = |A| (M_B + |B|), M_Z = |A| MH' |G S| + M_G2 |S| + |G| |S| and M_P = M_A + 2 |A| MH' |G S G^T| + 2 M_G2 |S| |G|^T + |G| |S| |G|^T (each "2 X" is
               X + X^T); rel as for the pairs with M_joint = [[M_P, M_Z], [M_Z^T, 0]] (the map's covariance is an input)
Magnitudes are float64 numpy (|Sigma| from np.linalg.inv of the rounded H): three digits of them are plenty."""
from __future__ import annotations

from types import SimpleNamespace as NS

import mpmath as mp
import numpy as np

from tests import ba_phases_ref as B
from tests import se3_ref
from tests.ba_phases_ref import _eye, _f, _mp, _zeros, chol_solve, cholesky

DPS = B.DPS
FD_DPS = 60
FD_STEP = "1e-15"
EPS = B.EPS
MIN_DET = 1e-9          # the no-redundancy rule of the header: part of the definition

# K_REF: the largest |float64 numpy restatement - mp| / (eps M) per buffer over every case and over the two routes (dense Cholesky inverse; the coupled kernels'
# Schur route onto the objects), measured by tests/test_pose_cov_mp_ref.py, which prints the table and holds it: a measurement above K_REF fails there.
# K = max(8, 4 K_REF), the rule and reasons of tests/test_ba_phases_ref.py.  No figure here comes from a GPU run.
K_REF = {"sigma": 26.0, "cross": 1.5, "rel": 6.0, "chi2": 0.4, "pcov": 28.0, "lev": 11.0, "t": 14.0, "vstat": 0.6, "summary": 0.25,       # measured: 24.6, 1.32, 5.37,
         "fixed_map": 0.4, "track_cam": 0.15, "track_cross": 0.2, "track_rel": 1.6}                     # 0.347, 26.7, 9.96, 12.8, 0.508, 0.214; 0.324, 0.112, 0.177, 1.45
# The dense route alone sits at 0.42 (sigma), 0.4 (rel), 1.6 (pcov), 1.2 (lev, t): what is above that is the Schur route's, largest on the graphs where a camera hangs
# on ONE object (3x2 with object 1 flagged out: sigma 24.6, pcov 26.7).  Folding cond(Hcc) into M the way tests/ba_phases_ref.py folds it into its Schur outputs
# (cond_2(Hcc) MHco^T E MHco per camera, as a perturbation of H's object blocks) was tried and widens M by 1e3 .. 1e6 on these graphs, so the route's excess stays in K_REF.
K = {buf: max(8.0, 4.0 * k) for buf, k in K_REF.items()}


def tol(buf, M):
    return K[buf] * EPS * np.asarray(M, np.float64)


def ratio(got, ref, M, mutant=False):
    """max |got - ref| / (eps M) over the entries where the reference is a number; the NaN pattern must be the reference's, and an entry whose scale is 0 must be met
    exactly (mutant=True: a miss of either kind is reported as inf instead of asserted)."""
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    M = np.broadcast_to(np.asarray(M, np.float64), np.shape(ref) if np.ndim(M) == 0 else np.shape(M)).ravel()
    same = np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref) & ~np.isnan(got)
    d = np.abs(got[ok] - ref[ok])
    exact = bool((d[M[ok] == 0] == 0).all())
    if mutant and not (same and exact):
        return float("inf")
    assert same, "the NaN pattern differs"
    assert exact, "an entry with no error scale differs"
    pos = M[ok] > 0
    return float((d[pos] / (EPS * M[ok][pos])).max()) if pos.any() else 0.0


# ---- SE(3) in mp, for the differenced Jacobian of a relative pose ----------------------------------------------------------------------------------------------------
def _exp(u):
    th = mp.sqrt(u[0] ** 2 + u[1] ** 2 + u[2] ** 2)
    a, b, c = se3_ref.coefficients(th)
    Om = B._skew(u[:3])
    Om2 = Om @ Om
    T = _eye(4)
    T[:3, :3] = _eye(3) + a * Om + b * Om2
    T[:3, 3] = (_eye(3) + b * Om + c * Om2) @ u[3:]
    return T


def _log(T):
    """log of a pose within 1e-6 rad of the identity (all the differences ask for): [omega, upsilon]"""
    Rm, t = T[:3, :3], T[:3, 3]
    w = np.array([Rm[2, 1] - Rm[1, 2], Rm[0, 2] - Rm[2, 0], Rm[1, 0] - Rm[0, 1]], dtype=object) / 2      # sin(theta) axis
    s = mp.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2)
    th = mp.atan2(s, (Rm[0, 0] + Rm[1, 1] + Rm[2, 2] - 1) / 2)
    assert th < mp.mpf("1e-6")
    t2 = th * th
    om = w * (1 + t2 / 6 + 3 * t2 ** 2 / 40 + 15 * t2 ** 3 / 336)                                        # theta / sin(theta)
    Om = B._skew(om)
    k = mp.mpf(1) / 12 + t2 / 720 + t2 ** 2 / 30240 + t2 ** 3 / 1209600                                 # V^-1 = I - Om / 2 + k Om^2
    ups = t - (Om @ t) / 2 + k * (Om @ (Om @ t))
    return np.array([om[0], om[1], om[2], ups[0], ups[1], ups[2]], dtype=object)


def _inv4(T):
    """The inverse of a 4x4 pose by the adjugate of its 3x3 block, not by its transpose: a float64 rotation matrix is orthonormal to an eps only, and with the true
    inverse exp(d) T T^-1 is exp(d) exactly, so that the structural zeros of the differenced Jacobian stay zeros"""
    R = T[:3, :3]
    adj = np.array([[R[(j + 1) % 3, (i + 1) % 3] * R[(j + 2) % 3, (i + 2) % 3] - R[(j + 1) % 3, (i + 2) % 3] * R[(j + 2) % 3, (i + 1) % 3] for j in range(3)]
                    for i in range(3)], dtype=object)
    Ri = adj / (R[0] @ adj[:, 0])
    Ti = _eye(4)
    Ti[:3, :3] = Ri
    Ti[:3, 3] = -(Ri @ T[:3, 3])
    return Ti


def _to4(T34):
    T = _eye(4)
    T[:3] = _mp(np.asarray(T34, np.float64).reshape(3, 4))
    return T


def _mul(A, Bm):
    """the product of two rigid 4x4 poses (the last row is not multiplied through)"""
    T = _eye(4)
    T[:3, :3] = A[:3, :3] @ Bm[:3, :3]
    T[:3, 3] = A[:3, :3] @ Bm[:3, 3] + A[:3, 3]
    return T


def _rel_pose(Ta, Tb, a_cam, b_cam):
    if a_cam and b_cam:
        return _mul(Tb, _inv4(Ta))
    if a_cam:
        return _mul(Ta, Tb)
    if b_cam:
        return _mul(Tb, Ta)
    return _mul(_inv4(Tb), Ta)


_JCACHE, _STEPS = {}, []


def _steps():
    """exp(+-h e_i), i = 0 .. 5, at the differences' precision: [(plus, minus)]"""
    if not _STEPS:
        for i in range(6):
            d = _zeros(6)
            d[i] = mp.mpf(FD_STEP)
            _STEPS.append((_exp(d), _exp(-d)))
    return _STEPS


def rel_jacobian(Ta34, Tb34, a_cam, b_cam):
    """[6,12] mp: d delta_rel / d (delta_a, delta_b), delta_rel = log(T_rel' T_rel^-1) under the left updates exp(delta) T, by central differences in mp."""
    key = (np.asarray(Ta34, np.float64).tobytes(), np.asarray(Tb34, np.float64).tobytes(), bool(a_cam), bool(b_cam))
    if key not in _JCACHE:
        with mp.workdps(FD_DPS):
            h = mp.mpf(FD_STEP)
            Ta, Tb = _to4(Ta34), _to4(Tb34)
            inv0 = _inv4(_rel_pose(Ta, Tb, a_cam, b_cam))
            J = _zeros(6, 12)
            for i, (p, m) in enumerate(_steps()):
                d = lambda A, Bm: _log(_mul(_rel_pose(A, Bm, a_cam, b_cam), inv0))
                J[:, i] = (d(_mul(p, Ta), Tb) - d(_mul(m, Ta), Tb)) / (2 * h)
                J[:, 6 + i] = (d(Ta, _mul(p, Tb)) - d(Ta, _mul(m, Tb))) / (2 * h)
        _JCACHE[key] = J
    return _JCACHE[key]


def _times_f64(G, S):
    """G [r,k] (mp) times S [k,m] (float64) in integer arithmetic -- S exactly, G to 2^-200 of its largest entry --, hundreds of times faster than mp products"""
    gmax = max(abs(x) for x in G.ravel())
    if gmax == 0 or not S.any():
        return _zeros(G.shape[0], S.shape[1])
    sg = 200 - int(mp.floor(mp.log(gmax, 2)))
    Gi = np.array([int(mp.nint(mp.ldexp(x, sg))) for x in G.ravel()], dtype=object).reshape(G.shape)
    mant, ex = np.frexp(S)
    emin = int(ex[mant != 0].min()) - 53
    Si = np.array([int(m) << int(e) for m, e in zip(np.ldexp(mant, 53).astype(np.int64).ravel().tolist(), np.where(mant != 0, ex - 53 - emin, 0).ravel().tolist())],
                  dtype=object).reshape(S.shape)
    return np.array([mp.ldexp(mp.mpf(z), emin - sg) for z in (Gi @ Si).ravel()], dtype=object).reshape(G.shape[0], S.shape[1])


def _inv_spd(A):
    L = cholesky(A)
    assert L is not None, "a designed case met a non-positive pivot"
    return chol_solve(L, _eye(len(A)))


def _problem(g, info=None):
    return NS(cam_T=g["cam_T"], obj_T=g["obj_T"], cam_fixed=g["cam_fixed"], obj_fixed=g["obj_fixed"], edge_cam=g["edge_cam"], edge_obj=g["edge_obj"],
              edge_camk=g["edge_camk"], edge_p=g["edge_p"], edge_uv=g["edge_uv"], edge_info=g["edge_info"] if info is None else info, huber_delta=0.0,
              chi2_thr=float("inf"))


# ---- H, Sigma and everything cut out of it ----------------------------------------------------------------------------------------------------------------------------
class CovRef:
    """The covariance family over one graph.  Vertices are coded as the library codes them: camera c is c, object o is n_cam + o.

    mutate (the wrong kernels of tests/test_pose_cov_mp_ref.py): ("hco_scale", c, o) one Hco block times 1 + 1e-9; ("flip_xy", e) info_xy of edge e with the other
    sign; ("count", e) edge e counted whatever its flag and its vertices; ("drop_cam", c, o) camera c left out of object o's Schur sum on the kernels' route."""

    def __init__(self, g, mutate=None):
        self.g, self.mutate, self._pairs = g, mutate, {}
        self.C, self.O, self.E = len(g["cam_T"]), len(g["obj_T"]), len(g["edge_cam"])
        C, O, E = self.C, self.O, self.E
        self.ec, self.eo = np.asarray(g["edge_cam"], np.int64), np.asarray(g["edge_obj"], np.int64)
        self.fixed = np.r_[np.asarray(g["cam_fixed"]).astype(bool), np.asarray(g["obj_fixed"]).astype(bool)]
        self.counted = np.array([bool(g["edge_inlier"][e] == 1) and not (self.fixed[self.ec[e]] and self.fixed[C + self.eo[e]]) for e in range(E)], bool)
        info = np.array(g["edge_info"], np.float64).reshape(E, 3)
        if mutate and mutate[0] == "count":
            self.counted[mutate[1]] = True
        if mutate and mutate[0] == "flip_xy":
            info[mutate[1], 1] *= -1
        self.pr = B.PhaseRef(_problem(g, info))
        reached = set()
        for e in np.flatnonzero(self.counted):
            reached.update((int(self.ec[e]), C + int(self.eo[e])))
        self.col, n = {}, 0                      # vertex -> first row in the system, None: fixed, "nan": free without a counted edge
        for v in range(C + O):
            if self.fixed[v]:
                self.col[v] = None
            elif v not in reached:
                self.col[v] = "nan"
            else:
                self.col[v] = n
                n += 6
        self.n = n
        self.cams = [c for c in range(C) if isinstance(self.col[c], int)]
        self.objs = [o for o in range(O) if isinstance(self.col[C + o], int)]
        self.status = [sum(1 for c in range(C) if self.col[c] == "nan"), sum(1 for o in range(O) if self.col[C + o] == "nan")]
        with mp.workdps(DPS):
            self._assemble()
            self._solve()
        self._scales()

    def _assemble(self):
        self.Hcc, self.Hoo, self.Hco = {c: _zeros(6, 6) for c in self.cams}, {o: _zeros(6, 6) for o in self.objs}, {}
        self.MH = np.zeros((self.n, self.n))
        for e in np.flatnonzero(self.counted):
            ed = self.pr.edge[e]
            i, j = self.col[ed.c], self.col[self.C + ed.o]
            if isinstance(i, int):
                self.Hcc[ed.c] += ed.Acc
                self.MH[i:i + 6, i:i + 6] += ed.MAcc
            if isinstance(j, int):
                self.Hoo[ed.o] += ed.Aoo
                self.MH[j:j + 6, j:j + 6] += ed.MAoo
            if isinstance(i, int) and isinstance(j, int):
                if (ed.c, ed.o) not in self.Hco:
                    self.Hco[(ed.c, ed.o)] = _zeros(6, 6)
                self.Hco[(ed.c, ed.o)] += ed.Aco
                self.MH[i:i + 6, j:j + 6] += ed.MAco
                self.MH[j:j + 6, i:i + 6] += ed.MAco.T
        if self.mutate and self.mutate[0] == "hco_scale":
            self.Hco[self.mutate[1:]] = self.Hco[self.mutate[1:]] * (1 + mp.mpf("1e-9"))

    def H_dense(self):
        """H [n,n] in mp, rows as self.col deals them (cameras, then objects)."""
        H = _zeros(self.n, self.n)
        for c in self.cams:
            H[self.col[c]:self.col[c] + 6, self.col[c]:self.col[c] + 6] = self.Hcc[c]
        for o in self.objs:
            j = self.col[self.C + o]
            H[j:j + 6, j:j + 6] = self.Hoo[o]
        for (c, o), blk in self.Hco.items():
            i, j = self.col[c], self.col[self.C + o]
            H[i:i + 6, j:j + 6], H[j:j + 6, i:i + 6] = blk, blk.T
        return H

    def _solve(self):
        """The structured inverse: what block() needs.  With free cameras next to free objects: Hoo^-1 and W_o = Hoo^-1 Hco^T per object, the reduced camera system's
        inverse Sigma_CC; X_o = W_o Sigma_CC on demand."""
        self._dense, self._blk, self._X = None, {}, {}
        self.coupled = bool(self.cams and self.objs)
        if self.mutate and self.mutate[0] == "drop_cam":
            self._dense = self.objects_route(drop=self.mutate[1:])
            return
        if not self.coupled:
            self.Vinv = {c: _inv_spd(self.Hcc[c]) for c in self.cams}
            self.Vinv.update({self.C + o: _inv_spd(self.Hoo[o]) for o in self.objs})
            return
        nc = 6 * len(self.cams)
        self.cpos = {c: 6 * i for i, c in enumerate(self.cams)}
        Sc = _zeros(nc, nc)
        for c in self.cams:
            Sc[self.cpos[c]:self.cpos[c] + 6, self.cpos[c]:self.cpos[c] + 6] = self.Hcc[c]
        self.Hinv, self.W = {}, {}
        for o in self.objs:
            Bt = _zeros(6, nc)
            for c in self.cams:
                if (c, o) in self.Hco:
                    Bt[:, self.cpos[c]:self.cpos[c] + 6] = self.Hco[(c, o)].T
            L = cholesky(self.Hoo[o])
            assert L is not None, "a designed case met a non-positive pivot"
            sol = chol_solve(L, np.hstack([_eye(6), Bt]))
            self.Hinv[o], self.W[o] = sol[:, :6], sol[:, 6:]
            Sc -= Bt.T @ self.W[o]
        self.SCC = _inv_spd(Sc)

    def block(self, u, w):
        """Sigma_uw [6,6] in mp of two vertices that have rows."""
        if self._dense is not None:
            i, j = self.col[u], self.col[w]
            return self._dense[i:i + 6, j:j + 6]
        if (u, w) in self._blk:
            return self._blk[(u, w)]
        C = self.C
        with mp.workdps(DPS):
            if not self.coupled:
                out = self.Vinv[u] if u == w else _zeros(6, 6)
            elif u < C and w < C:
                out = self.SCC[self.cpos[u]:self.cpos[u] + 6, self.cpos[w]:self.cpos[w] + 6]
            elif u < C:
                out = self.block(w, u).T
            else:
                if u - C not in self._X:
                    self._X[u - C] = self.W[u - C] @ self.SCC
                X = self._X[u - C]
                if w < C:
                    out = -X[:, self.cpos[w]:self.cpos[w] + 6]
                else:
                    out = X @ self.W[w - C].T
                    if u == w:
                        out = out + self.Hinv[u - C]
        self._blk[(u, w)] = out
        return out

    def structured(self):
        """Sigma [n,n] in mp from block(): for the comparison with dense() on the small cases."""
        S = _zeros(self.n, self.n)
        rows = [v for v in range(self.C + self.O) if isinstance(self.col[v], int)]
        for u in rows:
            for w in rows:
                S[self.col[u]:self.col[u] + 6, self.col[w]:self.col[w] + 6] = self.block(u, w)
        return S

    def dense(self):
        """Sigma [n,n] by one dense mp Cholesky of H."""
        with mp.workdps(DPS):
            return _inv_spd(self.H_dense()) if self.n else _zeros(0, 0)

    def objects_route(self, drop=None):
        """Sigma [n,n] in mp the way the coupled kernels go: S = blockdiag(Hoo) - sum_c Hco^T Hcc^-1 Hco, Sigma_OO = S^-1, Y_c = Hcc^-1 Hco, Sigma_cc' = [c == c'] Hcc^-1
        + Y_c Sigma_OO Y_c'^T, Sigma_cO = -Y_c Sigma_OO.  drop = (c, o): camera c is left out of the (o, o) block of S (a mutant)."""
        with mp.workdps(DPS):
            ns = 6 * len(self.objs)
            opos = {o: 6 * i for i, o in enumerate(self.objs)}
            S, Y, Ainv = _zeros(ns, ns), {}, {}
            for o in self.objs:
                S[opos[o]:opos[o] + 6, opos[o]:opos[o] + 6] = self.Hoo[o]
            for c in self.cams:
                Ainv[c] = _inv_spd(self.Hcc[c])
                Bc = _zeros(6, ns)
                for o in self.objs:
                    if (c, o) in self.Hco:
                        Bc[:, opos[o]:opos[o] + 6] = self.Hco[(c, o)]
                Y[c] = Ainv[c] @ Bc
                T = Bc.T @ Y[c]
                if drop is not None and drop[0] == c:
                    T[opos[drop[1]]:opos[drop[1]] + 6, opos[drop[1]]:opos[drop[1]] + 6] = _zeros(6, 6)
                S -= T
            SOO = _inv_spd(S)
            Sig = _zeros(self.n, self.n)
            o0 = self.col[self.C + self.objs[0]]
            Sig[o0:, o0:] = SOO
            Z = {c: Y[c] @ SOO for c in self.cams}
            for c in self.cams:
                i = self.col[c]
                Sig[i:i + 6, o0:], Sig[o0:, i:i + 6] = -Z[c], -Z[c].T
                for c2 in self.cams:
                    j = self.col[c2]
                    Sig[i:i + 6, j:j + 6] = Z[c] @ Y[c2].T + (Ainv[c] if c == c2 else 0)
            return Sig

    def _scales(self):
        """M_Sigma [n,n]; cond_cc: cond_2(Hcc) per camera of the coupled form (what the kernels' route carries)."""
        n = self.n
        self.H64 = _f(self.H_dense()) if n else np.zeros((0, 0))
        self.Sig64 = np.linalg.inv(self.H64) if n else np.zeros((0, 0))
        aS = np.abs(self.Sig64)
        d = np.sqrt(np.abs(np.diag(self.H64)))
        self._MHd = self.MH + np.outer(d, d)
        self.cond_cc = {c: B._cond_and_E(_f(self.Hcc[c]))[0] for c in self.cams} if self.coupled else {}
        self.M_Sigma = aS @ self._MHd @ aS

    # ---- the marginal blocks ------------------------------------------------------------------------------------------------------------------------------------------
    def _vertex(self, v):
        """(Sigma_vv float64 [6,6], M [6,6]): zeros for a fixed vertex, NaN for one without a row."""
        i = self.col[v]
        if i is None:
            return np.zeros((6, 6)), np.zeros((6, 6))
        if i == "nan":
            return np.full((6, 6), np.nan), np.zeros((6, 6))
        return _f(self.block(v, v)), self.M_Sigma[i:i + 6, i:i + 6]

    def marginals(self):
        """NS: cam_cov [C,6,6], obj_cov [O,6,6], M_cam, M_obj, status [2]."""
        if not hasattr(self, "_marg"):
            cam, obj = [self._vertex(c) for c in range(self.C)], [self._vertex(self.C + o) for o in range(self.O)]
            stack = lambda rows, k: np.stack([r[k] for r in rows]) if rows else np.zeros((0, 6, 6))
            self._marg = NS(cam_cov=stack(cam, 0), obj_cov=stack(obj, 0), M_cam=stack(cam, 1), M_obj=stack(obj, 1), status=np.array(self.status))
        return self._marg

    # ---- pairs -------------------------------------------------------------------------------------------------------------------------------------------------------
    def joint(self, a, b):
        """(Sigma_joint [12,12] mp, M [12,12]) of two vertices with zeros for a fixed one; (a, a) is fully correlated with itself."""
        Sj, Mj = _zeros(12, 12), np.zeros((12, 12))
        for i, u in enumerate((a, b)):
            for j, w in enumerate((a, b)):
                if isinstance(self.col[u], int) and isinstance(self.col[w], int):
                    Sj[6 * i:6 * i + 6, 6 * j:6 * j + 6] = self.block(u, w)
                    Mj[6 * i:6 * i + 6, 6 * j:6 * j + 6] = self.M_Sigma[self.col[u]:self.col[u] + 6, self.col[w]:self.col[w] + 6]
        return Sj, Mj

    def pose(self, v):
        return self.g["cam_T"][v] if v < self.C else self.g["obj_T"][v - self.C]

    def pairs(self, pairs, mutate=None):
        """NS: cross, rel [P,6,6], M_cross, M_rel, n_nan.  mutate: ("wrong_cross", q, a2, b2) pair q's cross block is Sigma of (b2, a2) transposed; ("no_tR", q) the
        Jacobian of pair q (camera, object) is the adjoint without its [t]x R block; ("plus_ab", q) the (object, object) pair q with + Sigma_ab."""
        pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
        if mutate is None and pairs.tobytes() in self._pairs:
            return self._pairs[pairs.tobytes()]
        P, C = len(pairs), self.C
        out = NS(cross=np.zeros((P, 6, 6)), rel=np.zeros((P, 6, 6)), M_cross=np.zeros((P, 6, 6)), M_rel=np.zeros((P, 6, 6)), n_nan=0)
        with mp.workdps(DPS):
            for q, (a, b) in enumerate(pairs.tolist()):
                if self.col[a] == "nan" or self.col[b] == "nan":
                    out.cross[q] = out.rel[q] = np.nan
                    out.n_nan += 1
                    continue
                Sj, Mj = self.joint(a, b)
                out.cross[q], out.M_cross[q] = _f(Sj[:6, 6:]), Mj[:6, 6:]
                hit = mutate is not None and mutate[1] == q
                if hit and mutate[0] == "wrong_cross":
                    out.cross[q] = _f(self.block(mutate[3], mutate[2]).T)
                if a == b:
                    continue                     # a relative pose that cannot move: 36 zeros, exactly
                J = rel_jacobian(self.pose(a), self.pose(b), a < C, b < C)
                if hit and mutate[0] == "no_tR":
                    Tc = np.asarray(self.pose(min(a, b)), np.float64).reshape(3, 4)
                    A = _zeros(6, 6)
                    A[:3, :3] = A[3:, 3:] = _mp(Tc[:, :3])
                    J = np.hstack([_eye(6), A]) if a < C else np.hstack([A, _eye(6)])
                if hit and mutate[0] == "plus_ab":
                    Sj = Sj.copy()
                    Sj[:6, 6:], Sj[6:, :6] = -Sj[:6, 6:], -Sj[6:, :6]
                aJ = np.abs(_f(J))
                out.rel[q] = _f(J @ Sj @ J.T)
                out.M_rel[q] = aJ @ (Mj + np.abs(_f(Sj))) @ aJ.T
        if mutate is None:
            self._pairs[pairs.tobytes()] = out
        return out

    # ---- residual statistics ---------------------------------------------------------------------------------------------------------------------------------------
    def _pcov_scale(self, a, b, J, MJ, aSj):
        """M of P_e = J Sigma_e J^T [2,2].  J Sigma is small where |J| |Sigma| is not (a rotation about the camera and the translation that undoes it), and Sigma's
        error is -Sigma dH Sigma, so its effect on P is (J Sigma) dH (J Sigma)^T with the FULL rows of Sigma; then J's own error against Sigma J^T, and the rounding
        of the two products as they stand."""
        rows = np.concatenate([np.arange(self.col[v], self.col[v] + 6) if isinstance(self.col[v], int) else np.zeros(0, int) for v in (a, b)])
        keep = np.concatenate([np.full(6, isinstance(self.col[v], int)) for v in (a, b)])
        if not len(rows):
            return np.zeros((2, 2))
        A = np.abs(J[:, keep] @ self.Sig64[rows, :])
        SJt = np.abs(self.Sig64[np.ix_(rows, rows)] @ J[:, keep].T)
        own = MJ[:, keep] @ SJt
        return A @ self._MHd @ A.T + own + own.T + np.abs(J) @ aSj @ np.abs(J).T

    def statistics(self, mutate=None):
        """NS of every output of suo_residual_statistics (edge_chi2, edge_pcov, edge_lev, edge_t, cam_stat, obj_stat, summary, status [4]), M_<output> beside each, and
        det [E] = det R_e.  mutate: ("lev_scaled",) leverage from s0^2 Sigma; ("t_neighbour", e) t of edge e with P of edge e + 1."""
        if mutate is None and hasattr(self, "_stats"):
            return self._stats
        C, O, E = self.C, self.O, self.E
        chi2, pcov, lev, t, det = np.zeros(E), np.zeros((E, 3)), np.zeros(E), np.zeros(E), np.full(E, np.nan)
        Mchi, Mp, Ml, Mt = np.zeros(E), np.zeros((E, 3)), np.zeros(E), np.zeros(E)
        chi_mp, lev_mp, Pm, MPm = [None] * E, [None] * E, [None] * E, [None] * E
        n_nan = n_nored = 0
        with mp.workdps(DPS):
            for e in range(E):
                ed = self.pr.edge[e]
                chi_mp[e], chi2[e], Mchi[e] = ed.chi2, float(ed.chi2), ed.Mchi
                a, b = ed.c, C + ed.o
                if self.col[a] == "nan" or self.col[b] == "nan":
                    pcov[e], lev[e], t[e] = np.nan, np.nan, np.nan
                    n_nan += 1
                    continue
                J = np.hstack([_zeros(2, 6) if self.fixed[a] else ed.Jc, _zeros(2, 6) if self.fixed[b] else ed.Jo])
                MJ = np.hstack([np.zeros((2, 6)) if self.fixed[a] else ed.MJc, np.zeros((2, 6)) if self.fixed[b] else ed.MJo])
                Sj, _ = self.joint(a, b)
                Pm[e] = J @ Sj @ J.T
                MPm[e] = self._pcov_scale(a, b, _f(J), MJ, np.abs(_f(Sj)))
            for e in range(E):
                if Pm[e] is None:
                    continue
                ed = self.pr.edge[e]
                P, MP, Om = Pm[e], MPm[e], ed.Om
                aOm = np.abs(_f(Om))
                pcov[e], Mp[e] = [float(P[0, 0]), float((P[0, 1] + P[1, 0]) / 2), float(P[1, 1])], [MP[0, 0], MP[0, 1], MP[1, 1]]
                lev_mp[e] = P[0, 0] * Om[0, 0] + 2 * P[0, 1] * Om[0, 1] + P[1, 1] * Om[1, 1]
                lev[e], Ml[e] = float(lev_mp[e]), float(((MP + np.abs(_f(P))) * aOm).sum())
                if mutate and mutate[0] == "t_neighbour" and mutate[1] == e:
                    P, MP = Pm[e + 1], MPm[e + 1]
                s = -1 if self.counted[e] else 1
                Rm = _eye(2) + s * (P @ Om)
                dt = Rm[0, 0] * Rm[1, 1] - Rm[0, 1] * Rm[1, 0]
                det[e] = float(dt)
                if dt <= mp.mpf(MIN_DET) or Rm[0, 0] <= 0 or Rm[1, 1] <= 0:
                    t[e] = np.nan
                    n_nored += 1
                    continue
                Ri = np.array([[Rm[1, 1], -Rm[0, 1]], [-Rm[1, 0], Rm[0, 0]]], dtype=object) / dt
                u, w = Om @ ed.err, Ri @ ed.err
                t[e] = float(u @ w)
                au, aw, aRi = np.abs(_f(u)), np.abs(_f(w)), np.abs(_f(Ri))
                MR = (MP + np.abs(_f(P))) @ aOm + np.abs(_f(Rm))
                Mt[e] = float((aOm @ ed.Me) @ aw + au @ (aRi @ (ed.Me + MR @ aw)) + au @ aw)
                if self.fixed[ed.c] and self.fixed[self.C + ed.o]:
                    Mt[e] = Mchi[e] * K["chi2"] / K["t"]          # (P = 0: t is chi2 to the bit, and its tolerance is chi2's)
            cnt = self.counted
            any_nan = bool(np.isnan(lev[cnt]).any())
            if mutate and mutate[0] == "lev_scaled":
                dof = 2 * int(cnt.sum()) - self.n
                s0 = sum(chi_mp[e] for e in np.flatnonzero(cnt)) / dof
                lev_mp = [None if x is None else x * s0 for x in lev_mp]
                lev = np.array([np.nan if x is None else float(x) for x in lev_mp])

            def sums(k, buf):
                """(sum chi2, M, sum lev, M, sum (2 - lev), M) over the edges k; a NaN leverage among them makes its two sums NaN"""
                sc, sl = sum((chi_mp[e] for e in k), mp.mpf(0)), None
                if not np.isnan(lev[k]).any():
                    sl = sum((lev_mp[e] for e in k), mp.mpf(0))
                Mc = float(Mchi[k].sum() * K["chi2"] / K[buf] + np.abs(chi2[k]).sum())
                Mlv = float(Ml[k].sum() * K["lev"] / K[buf] + np.abs(lev[k]).sum())
                nan = float("nan")
                return (float(sc), Mc, nan if sl is None else float(sl), 0.0 if sl is None else Mlv, nan if sl is None else float(2 * len(k) - sl),
                        0.0 if sl is None else Mlv + 2.0 * len(k))

            def vertex(mask):
                k = np.flatnonzero(mask & cnt)
                s = sums(k, "vstat")
                return [len(k), s[0], s[4]], [0.0, s[1], s[5]]
            cam = [vertex(self.ec == c) for c in range(C)]
            obj = [vertex(self.eo == o) for o in range(O)]
            k = np.flatnonzero(cnt)
            s = sums(k, "summary")
            m = len(k)
            dof = 2 * m - self.n
            s0 = float(sum((chi_mp[e] for e in k), mp.mpf(0)) / dof) if dof > 0 and not any_nan else float("nan")
        summary = np.array([m, self.n, s[0], s[2], dof, s0], float)
        M_summary = np.array([0.0, 0.0, s[1], s[3], 0.0, 0.0 if np.isnan(s0) else s[1] / dof + abs(s0)])
        grab = lambda rows, i: np.array([r[i] for r in rows], float).reshape(len(rows), 3)
        out = NS(edge_chi2=chi2, edge_pcov=pcov, edge_lev=lev, edge_t=t, cam_stat=grab(cam, 0), obj_stat=grab(obj, 0), summary=summary,
                 status=np.array(self.status + [n_nan, n_nored]), M_edge_chi2=Mchi, M_edge_pcov=Mp, M_edge_lev=Ml, M_edge_t=Mt, M_cam_stat=grab(cam, 1),
                 M_obj_stat=grab(obj, 1), M_summary=M_summary, det=det, counted=cnt.copy())
        if mutate is None:
            self._stats = out
        return out


# ---- tracking covariances ---------------------------------------------------------------------------------------------------------------------------------------------
def tracking(g, map_cov, mutate=None):
    """NS: cam_cov, fixed_map_cov [C,6,6], cross, rel [C,O,6,6], M_<output> beside each, status [2] = NaN cameras, objects not in the map.  The map's covariance is
    read by its upper triangle; an object whose block has NaN at (0, 0) is not in the map and its edges are not counted.  mutate: ("no_gsg", c, o): P_c of camera c
    without object o's columns of G in G Sigma G^T."""
    C, O, E = len(g["cam_T"]), len(g["obj_T"]), len(g["edge_cam"])
    assert np.asarray(g["obj_fixed"]).all(), "the tracking graph holds every object fixed"
    Mc = np.asarray(map_cov, np.float64).reshape(6 * O, 6 * O)
    in_map = np.array([not np.isnan(Mc[6 * o, 6 * o]) for o in range(O)], bool)
    S64 = np.triu(Mc) + np.triu(Mc, 1).T
    gone = np.repeat(~in_map, 6)
    S64[gone, :] = 0.0
    S64[:, gone] = 0.0
    aS = np.abs(S64)
    pr = B.PhaseRef(_problem(g))
    out = NS(cam_cov=np.zeros((C, 6, 6)), fixed_map_cov=np.zeros((C, 6, 6)), cross=np.zeros((C, O, 6, 6)), rel=np.zeros((C, O, 6, 6)),
             M_cam_cov=np.zeros((C, 6, 6)), M_fixed_map_cov=np.zeros((C, 6, 6)), M_cross=np.zeros((C, O, 6, 6)), M_rel=np.zeros((C, O, 6, 6)))
    n_nan = 0
    with mp.workdps(DPS):
        for c in range(C):
            Pc, Z, MP, MZ = _zeros(6, 6), _zeros(6, 6 * O), np.zeros((6, 6)), np.zeros((6, 6 * O))
            if not g["cam_fixed"][c]:
                counted = [e for e in range(E) if g["edge_inlier"][e] == 1 and g["edge_cam"][e] == c and in_map[g["edge_obj"][e]]]
                if not counted:
                    for k in ("cam_cov", "fixed_map_cov", "cross", "rel"):
                        getattr(out, k)[c] = np.nan
                    n_nan += 1
                    continue
                H, MH, Bo, MB = _zeros(6, 6), np.zeros((6, 6)), {}, np.zeros((6, 6 * O))
                for e in counted:
                    ed = pr.edge[e]
                    H, MH = H + ed.Acc, MH + ed.MAcc
                    Bo[ed.o] = Bo.get(ed.o, 0) + ed.Aco
                    MB[:, 6 * ed.o:6 * ed.o + 6] += ed.MAco
                A = _inv_spd(H)
                aA, d = np.abs(_f(A)), np.sqrt(np.abs(np.diag(_f(H))))
                MA = aA @ (MH + np.outer(d, d)) @ aA
                G = {o: A @ Bo[o] for o in Bo}
                aB, aG = np.zeros((6, 6 * O)), np.zeros((6, 6 * O))
                for o in Bo:
                    aB[:, 6 * o:6 * o + 6], aG[:, 6 * o:6 * o + 6] = np.abs(_f(Bo[o])), np.abs(_f(G[o]))
                MHd = MH + np.outer(d, d)
                MG2 = aA @ (MB + aB)                               # (dG = -A dH G, which keeps its structure below, + A dB + the product's rounding)
                Z = _times_f64(np.hstack([G.get(o, _zeros(6, 6)) for o in range(O)]), S64)
                Pc = A.copy()
                for o in Bo:
                    if not (mutate and mutate[0] == "no_gsg" and mutate[1:] == (c, o)):
                        Pc = Pc + Z[:, 6 * o:6 * o + 6] @ G[o].T
                aGS = aG @ aS
                MZ = aA @ MHd @ np.abs(_f(Z)) + MG2 @ aS + aGS
                T1, T2 = aA @ MHd @ np.abs(_f(Pc - A)), MG2 @ aS @ aG.T
                MP = MA + T1 + T1.T + T2 + T2.T + aGS @ aG.T
                out.fixed_map_cov[c], out.M_fixed_map_cov[c] = _f(A), MA
                out.cam_cov[c], out.M_cam_cov[c] = _f((Pc + Pc.T) / 2), MP
            for o in range(O):
                if not in_map[o]:
                    out.cross[c, o] = out.rel[c, o] = np.nan
                    continue
                X, MX = -Z[:, 6 * o:6 * o + 6], MZ[:, 6 * o:6 * o + 6]
                Soo = _mp(S64[6 * o:6 * o + 6, 6 * o:6 * o + 6])
                Sj = np.vstack([np.hstack([Pc, X]), np.hstack([X.T, Soo])])
                Mj = np.vstack([np.hstack([MP, MX]), np.hstack([MX.T, np.zeros((6, 6))])])
                J = rel_jacobian(g["cam_T"][c], g["obj_T"][o], True, False)
                aJ = np.abs(_f(J))
                rel = J @ Sj @ J.T
                out.cross[c, o], out.M_cross[c, o] = _f(X), MX
                out.rel[c, o], out.M_rel[c, o] = _f((rel + rel.T) / 2), aJ @ (Mj + np.abs(_f(Sj))) @ aJ.T
    out.status = np.array([n_nan, int((~in_map).sum())])
    return out


# ---- one reference per designed graph, shared by the CPU and the GPU modules --------------------------------------------------------------------------------------------
_CASES = {}


def _graph_of(name):
    from tests import pose_cov_cases, pose_cov_graph_cases, pose_cov_pair_cases, resid_stats_cases
    for mod in (resid_stats_cases, pose_cov_pair_cases, pose_cov_graph_cases, pose_cov_cases):
        if name in mod.CASES:
            return mod.CASES[name]()
    raise KeyError(name)


def case(name):
    """The CovRef of the designed graph `name` (tests/pose_cov_cases.py, pose_cov_pair_cases.py, pose_cov_graph_cases.py, resid_stats_cases.py: a name stands for one
    graph in all of them), one per process, read-only."""
    if name not in _CASES:
        _CASES[name] = CovRef(_graph_of(name))
    return _CASES[name]


def graph(name):
    """a deep copy of the graph of case(name), for a test to hand to the library or to modify"""
    return {k: np.array(v, copy=True) for k, v in case(name).g.items()}


def check_blocks(got_cam, got_obj, got_status, cr, what):
    """The marginal blocks of a kernel against CovRef cr, entry by entry at K["sigma"] eps M: NaN / zero blocks exactly where the reference has them, symmetric to the
    tolerance, positive diagonal, status.  Returns the worst error / tolerance."""
    mg = cr.marginals()
    worst = 0.0
    for name, a, b, Mb in (("cam", got_cam, mg.cam_cov, mg.M_cam), ("obj", got_obj, mg.obj_cov, mg.M_obj)):
        assert a.shape == b.shape
        for v in range(len(b)):
            if np.isnan(b[v]).any():
                assert np.isnan(a[v]).all(), (what, name, v)
            elif not b[v].any():
                assert not a[v].any(), (what, name, v, "a fixed vertex is 36 zeros")
            else:
                t, err = tol("sigma", Mb[v]), np.abs(a[v] - b[v])
                worst = max(worst, float((err / t).max()))
                assert (err <= t).all(), (what, name, v, float((err / t).max()))
                assert (np.abs(a[v] - a[v].T) <= t).all() and (np.diag(a[v]) > 0).all(), (what, name, v)
    assert list(got_status) == list(mg.status), (what, got_status, mg.status)
    return worst


def check_pairs(pairs, got_cross, got_rel, got_n_nan, cr, what):
    """The pair blocks of a kernel against CovRef cr at K["cross"] / K["rel"] eps M (a structural zero, M == 0, exactly): NaN blocks exactly where the reference has
    them and counted.  Returns ({kind: worst error / tolerance}, the reference's pairs)."""
    pr = cr.pairs(pairs)
    assert got_cross.shape == pr.cross.shape and got_rel.shape == pr.rel.shape
    worst = {"cross": 0.0, "cam-obj": 0.0, "obj-obj": 0.0, "cam-cam": 0.0}
    for q, (a, b) in enumerate(np.asarray(pairs).tolist()):
        if np.isnan(pr.rel[q]).any():
            assert np.isnan(got_cross[q]).all() and np.isnan(got_rel[q]).all(), (what, q, a, b)
            continue
        kind = "cam-cam" if max(a, b) < cr.C else ("cam-obj" if min(a, b) < cr.C else "obj-obj")
        for buf, key, x, ref, Mx in (("cross", "cross", got_cross[q], pr.cross[q], pr.M_cross[q]), ("rel", kind, got_rel[q], pr.rel[q], pr.M_rel[q])):
            r = ratio(x, ref, Mx) / K[buf]
            worst[key] = max(worst[key], r)
            assert r <= 1.0, (what, q, a, b, buf, r)
        t = tol("rel", pr.M_rel[q])
        assert (np.abs(got_rel[q] - got_rel[q].T) <= t).all(), (what, q, "rel is symmetric")
    assert got_n_nan == pr.n_nan, (what, got_n_nan, pr.n_nan)
    return worst, pr


_TRACK = {}


def track_case(n_obj):
    """tracking() of tests/track_cov_cases.case(n_obj), one per process."""
    if n_obj not in _TRACK:
        from tests import track_cov_cases
        g, Sigma, _ = track_cov_cases.case(n_obj)
        _TRACK[n_obj] = tracking(g, Sigma)
    return _TRACK[n_obj]
