"""The phases of one Levenberg-Marquardt trial of the bundle adjustment, written from their definitions in mpmath at 40 digits -- the yardstick of
tests/test_ba_phases_ref.py (numpy float64 against it) and tests/test_gpu_ba_phases.py (the kernels of csrc/lm_dist.hip against it).  Nothing here calls
tests/ba_numpy_phases.py or restates csrc/lm_device.h.

Definitions
  edge error     e = uv - pi(T_c T_o p), pi(x, y, z) = (fx x / z + cx, fy y / z + cy)                       (types_object_slam.cpp:45-60)
  Jacobians      of e under the LEFT update exp(u) T, u = [omega, upsilon]: d(T q)/du = [-[T q]x | I], so with q_w = T_o p, q_c = T_c q_w and
                 D = -d pi / d q_c (2x3):  J_c = D [-[q_c]x | I],  J_o = D R_c [-[q_w]x | I]                   (types_object_slam.cpp:70-123)
  chi2           e^T Omega e, Omega = [[xx, xy], [xy, yy]]
  Huber          e2 <= delta^2: rho = e2, w = 1; else rho = 2 sqrt(e2) delta - delta^2, w = delta / sqrt(e2)
  active         an edge whose level is 0 and whose two vertices are not both fixed
  normal eq.     H_cc = sum w J_c^T Omega J_c, b_c = -sum w J_c^T Omega e (a free camera's active edges); H_oo, b_o likewise; H_co = sum w J_c^T Omega J_o
  Schur          A_c = H_cc + lambda I; S_g = sum_c H_co^T A_c^-1 H_co', r_g = sum_c H_co^T A_c^-1 b_c over the free cameras, rows / columns by object slot
                 (the free objects in ascending order); a camera whose A_c has a non-positive Cholesky pivot contributes nothing and clears ok
  reduced solve  (blockdiag(H_oo + lambda I) - S) x_o = b_o - r; x_c = A_c^-1 (b_c - sum_o H_co x_o); a non-positive pivot refuses the step
  update         T <- exp(x) T (tests/se3_ref.py: Rodrigues in mp; g2o's shortcut R = V = I + Om + Om^2 below |omega| = 1e-5, as the kernels keep it)
  gain ratio     scale = sum x (lambda x + b), over the cameras and over the objects

Layouts (include/suo_hip.h, "phase-wise bundle adjustment"): lin = [chi2 | (Hoo 21 upper + bo 6) per object | max |diag Hcc|],
sch = [S_g | r_g | ok], red = [chi2 after | scale over cameras | ok | scale over objects].

Error scales.  Next to every value stands a float64 magnitude M such that a careful fp64 evaluation errs by a few eps M:
  * for a sum of products, M is the sum of the products' absolute values, with every factor that is itself computed replaced by ITS magnitude sum (the residual
    e = uv - pi(..) is a difference of numbers of a few hundred pixels: M_e is their absolute sum, not |e|);
  * a Huber weight above delta carries the relative error M_chi2 / (2 chi2) of its chi2;
  * an inverse A^-1 of a positive definite A computed by Cholesky errs by eps cond_2(A) sqrt(A^-1_ii A^-1_jj) entry (i, j) (the bound is invariant under the diagonal
    scaling that makes rotations and translations comparable; sqrt(A^-1_ii A^-1_jj) >= |A^-1_ij|).  Wherever an inverse enters, the magnitude returned is ALREADY
    multiplied by that condition number ("MC"), per camera for A_c and once for the reduced system, and the condition numbers are returned beside it;
  * a step x moves a pose by dR = [d omega]x R, dt = d omega x t + d upsilon: the poses' scales carry the step's.
The tolerance of a comparison is K eps M with K fixed per buffer in tests/test_ba_phases_ref.py.  Magnitudes and condition numbers are float64 numpy: three digits
of them are plenty."""
from __future__ import annotations

from types import SimpleNamespace as NS

import mpmath as mp
import numpy as np

from tests import se3_ref

DPS = 40
EPS = float(np.finfo(np.float64).eps)
IU = np.triu_indices(6)
SHORTCUT_BELOW = mp.mpf("1e-10")          # |omega|^2 below which g2o (and the kernels) use R = V = I + Om + Om^2


def _mp(a):
    a = np.asarray(a, np.float64)
    return np.array([mp.mpf(float(x)) for x in a.ravel()], dtype=object).reshape(a.shape)


def _f(a):
    return np.array([float(x) for x in np.ravel(a)], np.float64).reshape(np.shape(a))


def _skew(v):
    z = mp.mpf(0) if isinstance(v[0], mp.mpf) else 0.0
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], dtype=object if isinstance(v[0], mp.mpf) else np.float64)


def _eye(n):
    I = np.empty((n, n), dtype=object)
    for i in range(n):
        for j in range(n):
            I[i, j] = mp.mpf(1 if i == j else 0)
    return I


def _zeros(*shape):
    Z = np.empty(shape, dtype=object)
    Z.fill(mp.mpf(0))
    return Z


def cholesky(A, floor=None):
    """Lower Cholesky factor of a symmetric mp matrix, or None when a pivot is not positive.  An exactly singular matrix leaves a pivot of rounding noise (1e-40 of
    the diagonal) of either sign: pivots below 1e-25 of the largest diagonal entry count as not positive."""
    n = len(A)
    L = _zeros(n, n)
    floor = mp.mpf("1e-25") * max([abs(A[i, i]) for i in range(n)] + [mp.mpf("1e-300")]) if floor is None else floor
    for j in range(n):
        piv = A[j, j] - (L[j, :j] @ L[j, :j] if j else 0)
        if not piv > floor:
            return None
        L[j, j] = mp.sqrt(piv)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - (L[j + 1:, :j] @ L[j, :j] if j else 0)) / L[j, j]
    return L


def chol_solve(L, B):
    """A^-1 B for A = L L^T; B a vector or a matrix."""
    n = len(L)
    Y = np.array(B, dtype=object, copy=True)
    for i in range(n):
        Y[i] = (Y[i] - (L[i, :i] @ Y[:i] if i else 0)) / L[i, i]
    for i in range(n - 1, -1, -1):
        Y[i] = (Y[i] - (L[i + 1:, i] @ Y[i + 1:] if i + 1 < n else 0)) / L[i, i]
    return Y


def _cond_and_E(A64):
    """(cond_2(A), E) of a float64 symmetric positive definite A: E_ij = sqrt(A^-1_ii A^-1_jj)."""
    ev = np.linalg.eigvalsh(A64)
    d = np.sqrt(np.abs(np.diag(np.linalg.inv(A64))))
    return float(ev.max() / max(ev.min(), 1e-300)), np.outer(d, d)


def in_shortcut(u):
    with mp.workdps(se3_ref.DPS):
        w = [mp.mpf(float(x)) for x in np.asarray(u, np.float64)[:3]]
        return bool(w[0] ** 2 + w[1] ** 2 + w[2] ** 2 < SHORTCUT_BELOW)


def oplus(T, u, g2o_shortcut=True):
    """exp(u) T for a float64 [3,4] pose and a float64 step: (T' float64 [3,4], M [3,4] of the product's own rounding).  g2o_shortcut=False: below the shortcut's
    angle R = V = I + Om + Om^2 is applied as it stands, R' = R R_T, t' = R upsilon + R t -- tests/ba_numpy_phases.py, which does not pass through a quaternion; the
    two differ by |omega|^2 |t|, which reaches a few eps at 1e-8 rad."""
    T = np.asarray(T, np.float64).reshape(3, 4)
    u = np.asarray(u, np.float64)
    short = in_shortcut(u)
    if short and not g2o_shortcut:
        with mp.workdps(se3_ref.DPS):
            Rm, Om = _mp(T), _skew(_mp(u[:3]))
            Rs = _eye(3) + Om + Om @ Om
            Tn = _f(np.hstack([Rs @ Rm[:, :3], (Rs @ _mp(u[3:]) + Rs @ Rm[:, 3])[:, None]]))
    else:
        Tn = se3_ref.oplus_shortcut(T, u) if short else se3_ref.oplus(T, u)
    Om = np.abs(_skew(u[:3]))
    Re = np.eye(3) + Om + Om @ Om
    M = np.zeros((3, 4))
    M[:, :3] = Re @ np.abs(T[:, :3]) + 1.0                 # (+1: the unit quaternion the kernels keep, normalised after every update)
    M[:, 3] = Re @ np.abs(u[3:]) + Re @ np.abs(T[:, 3])
    return Tn, M


def _pose_scale(T, X):
    """What a step known to +-X [6] (omega, upsilon) does to the entries of the updated pose T [3,4]."""
    S = np.zeros((3, 4))
    Xs = np.abs(_skew(X[:3]))
    S[:, :3] = Xs @ np.abs(T[:, :3])
    S[:, 3] = Xs @ np.abs(T[:, 3]) + X[3:]
    return S


class PhaseRef:
    """The phases over one ba.Problem at the poses given (default: the problem's own).  Every method is pure: the state travels in the returned namespaces."""

    def __init__(self, prob, cam_T=None, obj_T=None, flip_xy=False, info=None, chi2_only=False):
        self.P = prob
        self.cam_T = np.array(prob.cam_T if cam_T is None else cam_T, np.float64).reshape(-1, 3, 4)
        self.obj_T = np.array(prob.obj_T if obj_T is None else obj_T, np.float64).reshape(-1, 3, 4)
        self.C, self.O, self.E = len(self.cam_T), len(self.obj_T), len(prob.edge_cam)
        self.cam_fixed = np.asarray(prob.cam_fixed).astype(bool)
        self.obj_fixed = np.asarray(prob.obj_fixed).astype(bool)
        self.free_obj = [o for o in range(self.O) if not self.obj_fixed[o]]
        self.slot = {o: s for s, o in enumerate(self.free_obj)}
        self.ns = 6 * len(self.free_obj)
        self.delta = float(prob.huber_delta)
        self.thr = float(prob.chi2_thr)
        self.info = np.array(prob.edge_info if info is None else info, np.float64)
        self.chi2_only = chi2_only                         # (the state after a step: only its chi2 is asked for)
        if flip_xy:                                        # (a mutant of tests/test_ba_phases_ref.py)
            self.info[:, 1] *= -1
        with mp.workdps(DPS):
            self._edges()

    # ---- per edge ------------------------------------------------------------------------------------------------------------------------------------
    def _edges(self):
        P = self.P
        Tc, To = [_mp(T) for T in self.cam_T], [_mp(T) for T in self.obj_T]
        I3 = _eye(3)
        self.edge = []
        for e in range(self.E):
            c, o = int(P.edge_cam[e]), int(P.edge_obj[e])
            p, k, uv, inf = _mp(P.edge_p[e]), _mp(P.edge_camk[e]), _mp(P.edge_uv[e]), _mp(self.info[e])
            qw = To[o][:, :3] @ p + To[o][:, 3]
            qc = Tc[c][:, :3] @ qw + Tc[c][:, 3]
            x, y, z = qc
            err = np.array([uv[0] - (k[0] * x / z + k[2]), uv[1] - (k[1] * y / z + k[3])], dtype=object)
            Om = np.array([[inf[0], inf[1]], [inf[1], inf[2]]], dtype=object)
            chi2 = err @ Om @ err
            zero = mp.mpf(0)
            if self.chi2_only:
                fe, aOm = np.abs(_f(err)), np.abs(_f(Om))
                aTc, aTo = np.abs(self.cam_T[c]), np.abs(self.obj_T[o])
                Mqc = aTc[:, :3] @ (aTo[:, :3] @ np.abs(P.edge_p[e]) + aTo[:, 3]) + aTc[:, 3]
                fqc, fk = _f(qc), np.asarray(P.edge_camk[e], np.float64)
                aD = np.abs([[fk[0] / fqc[2], 0, fk[0] * fqc[0] / fqc[2] ** 2], [0, fk[1] / fqc[2], fk[1] * fqc[1] / fqc[2] ** 2]])
                Me = np.abs(P.edge_uv[e]) + np.abs([fk[0] * fqc[0] / fqc[2], fk[1] * fqc[1] / fqc[2]]) + np.abs(fk[2:]) + aD @ Mqc
                self.edge.append(NS(c=c, o=o, err=err, chi2=chi2, Mchi=float(fe @ aOm @ Me + Me @ aOm @ fe + fe @ aOm @ fe)))
                continue
            D = -np.array([[k[0] / z, zero, -k[0] * x / (z * z)], [zero, k[1] / z, -k[1] * y / (z * z)]], dtype=object)
            Jc = D @ np.hstack([-_skew(qc), I3])
            Jo = D @ Tc[c][:, :3] @ np.hstack([-_skew(qw), I3])
            # magnitudes (float64)
            aTc, aTo = np.abs(self.cam_T[c]), np.abs(self.obj_T[o])
            Mqw = aTo[:, :3] @ np.abs(P.edge_p[e]) + aTo[:, 3]
            Mqc = aTc[:, :3] @ Mqw + aTc[:, 3]
            fqc, fqw, fk = _f(qc), _f(qw), np.asarray(P.edge_camk[e], np.float64)
            aD = np.abs(_f(D))
            Me = np.abs(P.edge_uv[e]) + np.abs([fk[0] * fqc[0] / fqc[2], fk[1] * fqc[1] / fqc[2]]) + np.abs(fk[2:]) + aD @ Mqc
            aOm = np.abs(_f(Om))
            fe = np.abs(_f(err))
            Mchi = float(fe @ aOm @ Me + Me @ aOm @ fe + fe @ aOm @ fe)
            MJc = aD @ np.hstack([np.abs(_skew(Mqc)), np.eye(3)])
            MJo = aD @ aTc[:, :3] @ np.hstack([np.abs(_skew(Mqw)), np.eye(3)])
            OJc, OJo, Oe = Om @ Jc, Om @ Jo, Om @ err
            self.edge.append(NS(c=c, o=o, err=err, chi2=chi2, Mchi=Mchi, Jc=Jc, Jo=Jo, Acc=Jc.T @ OJc, Aoo=Jo.T @ OJo, Aco=Jc.T @ OJo, gc=-(Jc.T @ Oe), go=-(Jo.T @ Oe),
                                MAcc=MJc.T @ aOm @ MJc, MAoo=MJo.T @ aOm @ MJo, MAco=MJc.T @ aOm @ MJo, Mgc=MJc.T @ aOm @ Me, Mgo=MJo.T @ aOm @ Me,
                                Om=Om, Me=Me, MJc=MJc, MJo=MJo))      # (the last four: tests/pose_cov_mp_ref.py)

    def classify(self):
        """(chi2 float64 [E], M [E], inlier flags [E] under chi2 > chi2_thr -> outlier, chi2 in mp)."""
        chi = [ed.chi2 for ed in self.edge]
        return _f(chi), np.array([ed.Mchi for ed in self.edge]), np.array([0 if c > mp.mpf(self.thr) else 1 for c in chi], np.uint8), chi

    def active(self, level):
        return [e for e in range(self.E) if level[e] == 0 and not (self.cam_fixed[self.edge[e].c] and self.obj_fixed[self.edge[e].o])]

    def _rho(self, ed, robust_on, unit_weight=False):
        """(rho, w, M_rho, relative error scale of w) of an edge, mp / mp / float / float."""
        if not robust_on or ed.chi2 <= mp.mpf(self.delta) ** 2:
            return ed.chi2, mp.mpf(1), ed.Mchi, 0.0
        s = mp.sqrt(ed.chi2)
        w = mp.mpf(self.delta) / s
        return 2 * s * self.delta - mp.mpf(self.delta) ** 2, (mp.mpf(1) if unit_weight else w), float(w) * ed.Mchi + 2 * float(s) * self.delta + self.delta ** 2, \
            ed.Mchi / (2 * float(ed.chi2))

    def chi_total(self, robust_on, level):
        with mp.workdps(DPS):
            chi, M = mp.mpf(0), 0.0
            for e in self.active(level):
                r, _, Mr, _ = self._rho(self.edge[e], robust_on)
                chi, M = chi + r, M + Mr
            return float(chi), M

    # ---- linearise ------------------------------------------------------------------------------------------------------------------------------------
    def linearize(self, robust_on, level, mutate=None):
        """mutate (tests/test_ba_phases_ref.py): ("unit_weight",) or ("drop_pair", o): object o's gather misses its last (camera, object) pair."""
        with mp.workdps(DPS):
            C, O = self.C, self.O
            L = NS(robust_on=robust_on, level=np.array(level, np.uint8), Hcc=_zeros(C, 6, 6), bc=_zeros(C, 6), Hoo=_zeros(O, 6, 6), bo=_zeros(O, 6), Hco={},
                   MHcc=np.zeros((C, 6, 6)), Mbc=np.zeros((C, 6)), MHoo=np.zeros((O, 6, 6)), Mbo=np.zeros((O, 6)), MHco={})
            unit = mutate is not None and mutate[0] == "unit_weight"
            skip = None
            if mutate is not None and mutate[0] == "drop_pair":
                skip = (max(self.edge[e].c for e in self.active(level) if self.edge[e].o == mutate[1]), mutate[1])
            chi, Mchi = mp.mpf(0), 0.0
            for e in self.active(level):
                ed = self.edge[e]
                r, w, Mr, wrel = self._rho(ed, robust_on, unit)
                chi, Mchi = chi + r, Mchi + Mr
                fw = float(w) * (1 + wrel)
                if not self.cam_fixed[ed.c]:
                    L.Hcc[ed.c] += w * ed.Acc
                    L.bc[ed.c] += w * ed.gc
                    L.MHcc[ed.c] += fw * ed.MAcc
                    L.Mbc[ed.c] += fw * ed.Mgc
                if not self.obj_fixed[ed.o] and (ed.c, ed.o) != skip:
                    L.Hoo[ed.o] += w * ed.Aoo
                    L.bo[ed.o] += w * ed.go
                    L.MHoo[ed.o] += fw * ed.MAoo
                    L.Mbo[ed.o] += fw * ed.Mgo
                if not self.cam_fixed[ed.c] and not self.obj_fixed[ed.o]:
                    key = (ed.c, ed.o)
                    if key not in L.Hco:
                        L.Hco[key], L.MHco[key] = _zeros(6, 6), np.zeros((6, 6))
                    L.Hco[key] += w * ed.Aco
                    L.MHco[key] += fw * ed.MAco
            lin, M = np.zeros(2 + 27 * O), np.zeros(2 + 27 * O)
            lin[0], M[0] = float(chi), Mchi
            for o in range(O):
                lin[1 + 27 * o:22 + 27 * o], M[1 + 27 * o:22 + 27 * o] = _f(L.Hoo[o][IU]), L.MHoo[o][IU]
                lin[22 + 27 * o:28 + 27 * o], M[22 + 27 * o:28 + 27 * o] = _f(L.bo[o]), L.Mbo[o]
            free = [c for c in range(C) if not self.cam_fixed[c]]
            dg = [(abs(L.Hcc[c][d, d]), L.MHcc[c][d, d]) for c in free for d in range(6)]
            if dg:
                top = max(dg, key=lambda t: t[0])
                lin[-1], M[-1] = float(top[0]), max(m for _, m in dg)
            L.lin, L.M = lin, M
            L.maxdiag = max([lin[-1]] + [abs(lin[1 + 27 * o + d]) for o in self.free_obj for d in (0, 6, 11, 15, 18, 20)])
            return L

    # ---- Schur ----------------------------------------------------------------------------------------------------------------------------------------
    def schur(self, L, lam, mutate=None):
        """mutate: ("drop_cam", o): object o's row of S_g misses one camera; ("no_lambda",); ("slots", map): another object -> slot map."""
        with mp.workdps(DPS):
            ns, lam_mp = self.ns, mp.mpf(float(lam))
            slot = self.slot if not (mutate and mutate[0] == "slots") else mutate[1]
            Sc = NS(lam=float(lam), S=_zeros(ns, ns), r=_zeros(ns), MS=np.zeros((ns, ns)), Mr=np.zeros(ns), Ainv={}, yc={}, Y={}, cond={}, E={}, failed=[], L=L)
            drop = None
            if mutate and mutate[0] == "drop_cam":
                drop = (sorted(c for (c, o) in L.Hco if o == mutate[1])[len([1 for (c, o) in L.Hco if o == mutate[1]]) // 2], mutate[1])
            for c in range(self.C):
                if self.cam_fixed[c]:
                    continue
                A = L.Hcc[c] + (0 if (mutate and mutate[0] == "no_lambda") else lam_mp) * _eye(6)
                Lc = cholesky(A)
                if Lc is None:
                    Sc.failed.append(c)
                    continue
                Ai = chol_solve(Lc, _eye(6))
                Sc.Ainv[c] = Ai
                Sc.cond[c], Sc.E[c] = _cond_and_E(_f(A))
                Sc.yc[c] = Ai @ L.bc[c]
                objs = [o for (cc, o) in L.Hco if cc == c]
                for o in objs:
                    Sc.Y[(c, o)] = Ai @ L.Hco[(c, o)]
                for o1 in objs:
                    s1 = slot[o1]
                    H1, MH1 = L.Hco[(c, o1)], L.MHco[(c, o1)]
                    Sc.r[6 * s1:6 * s1 + 6] += H1.T @ Sc.yc[c]
                    Sc.Mr[6 * s1:6 * s1 + 6] += Sc.cond[c] * (MH1.T @ Sc.E[c] @ L.Mbc[c])
                    for o2 in objs:
                        if (c, o1) == drop or slot[o2] < s1:          # (the lower blocks are mirrored below: H^T A^-1 H' is the transpose of H'^T A^-1 H)
                            continue
                        s2 = slot[o2]
                        Sc.S[6 * s1:6 * s1 + 6, 6 * s2:6 * s2 + 6] += H1.T @ Sc.Y[(c, o2)]
                        Sc.MS[6 * s1:6 * s1 + 6, 6 * s2:6 * s2 + 6] += Sc.cond[c] * (MH1.T @ Sc.E[c] @ L.MHco[(c, o2)])
            for i in range(ns):
                for j in range(6 * (i // 6)):
                    Sc.S[i, j], Sc.MS[i, j] = Sc.S[j, i], Sc.MS[j, i]
            Sc.ok = 0.0 if Sc.failed else 1.0
            Sc.sch = np.concatenate([_f(Sc.S).ravel(), _f(Sc.r), [Sc.ok]])
            Sc.MC = np.concatenate([Sc.MS.ravel(), Sc.Mr, [0.0]])
            return Sc

    def totals(self, L, Sc):
        """What suo_ba_solve_update takes as `in`, rounded to float64: [Hoo 21 + bo 6 per object | S | r]."""
        return np.concatenate([L.lin[1:1 + 27 * self.O], Sc.sch[:-1]])

    # ---- reduced solve, back-substitution, update -------------------------------------------------------------------------------------------------------
    def solve_update(self, L, Sc, lam, robust_on, totals=None, mutate=None):
        """The step from the float64 `totals` (default: this reference's own, rounded) and the camera blocks of Sc.  mutate: ("scale_without_lambda",)."""
        with mp.workdps(DPS):
            O, ns, lam_mp = self.O, self.ns, mp.mpf(float(lam))
            t = self.totals(L, Sc) if totals is None else np.asarray(totals, np.float64)
            HB, St, rt = t[:27 * O], _mp(t[27 * O:27 * O + ns * ns].reshape(ns, ns)), _mp(t[27 * O + ns * ns:27 * O + ns * ns + ns])
            A, rhs, Mrhs, bo = -St, -rt, np.abs(_f(rt)), {}
            for o, s in self.slot.items():
                H = _zeros(6, 6)
                H[IU] = _mp(HB[27 * o:27 * o + 21])
                H = H + H.T
                for d in range(6):
                    H[d, d] = H[d, d] / 2 + lam_mp
                A[6 * s:6 * s + 6, 6 * s:6 * s + 6] += H
                bo[o] = _mp(HB[27 * o + 21:27 * o + 27])
                rhs[6 * s:6 * s + 6] += bo[o]
                Mrhs[6 * s:6 * s + 6] += np.abs(HB[27 * o + 21:27 * o + 27])
            U = NS(ok=0.0, cond_red=float("inf"), cam_T=self.cam_T.copy(), obj_T=self.obj_T.copy(), xc=np.zeros((self.C, 6)), xo=np.zeros((O, 6)))
            chi0, Mchi0 = self.chi_total(robust_on, L.level)
            U.red, U.Mred = np.array([chi0, 0.0, 0.0, 0.0]), np.array([Mchi0, 0.0, 0.0, 0.0])
            U.MCxc, U.MCxo = np.zeros((self.C, 6)), np.zeros((O, 6))
            U.MCcam, U.MCobj = np.ones((self.C, 3, 4)), np.ones((O, 3, 4))
            for i in range(ns):                                # (the lower triangle is the matrix, as for every Cholesky)
                for j in range(i):
                    A[j, i] = A[i, j]
            Lr = cholesky(A) if ns else _zeros(0, 0)
            if Lr is None or Sc.failed:
                return U
            x = chol_solve(Lr, rhs) if ns else rhs
            if ns:
                # the solve's own error, cond E |rhs|, and what the inputs' error scales do to x = A^-1 b: |A^-1| (M_b + M_A |x|) -- the totals are the reference's rounded
                # values or a kernel's own within THEIR scales, and one tolerance holds for both feeds
                U.cond_red, Er = _cond_and_E(_f(A))
                Mb, MA = Sc.Mr.copy(), Sc.MS.copy()
                for o, s_ in self.slot.items():
                    Mb[6 * s_:6 * s_ + 6] += L.Mbo[o]
                    MA[6 * s_:6 * s_ + 6, 6 * s_:6 * s_ + 6] += L.MHoo[o]
                MCx = U.cond_red * (Er @ Mrhs) + Er @ (Mb + MA @ np.abs(_f(x)))
            else:
                U.cond_red, MCx = 1.0, np.zeros(0)
            sc_o, Msc_o = mp.mpf(0), 0.0
            xo = {o: x[6 * s:6 * s + 6] for o, s in self.slot.items()}
            lam_s = mp.mpf(0) if mutate and mutate[0] == "scale_without_lambda" else lam_mp
            for o, s in self.slot.items():
                U.xo[o], U.MCxo[o] = _f(xo[o]), MCx[6 * s:6 * s + 6]
                sc_o += xo[o] @ (lam_s * xo[o] + bo[o])
                ax, ab = np.abs(U.xo[o]), np.abs(_f(bo[o]))
                Msc_o += float((2 * lam * ax + ab) @ U.MCxo[o] + ax @ (lam * ax + L.Mbo[o]))
            sc_c, Msc_c = mp.mpf(0), 0.0
            for c in range(self.C):
                if self.cam_fixed[c]:
                    continue
                xc = Sc.yc[c].copy()
                MC = Sc.cond[c] * (Sc.E[c] @ L.Mbc[c])
                for (cc, o), Y in Sc.Y.items():
                    if cc == c:
                        xc = xc - Y @ xo[o]
                        MC = MC + Sc.cond[c] * (Sc.E[c] @ L.MHco[(c, o)] @ np.abs(U.xo[o])) + np.abs(_f(Y)) @ U.MCxo[o]
                U.xc[c], U.MCxc[c] = _f(xc), MC
                sc_c += xc @ (lam_s * xc + L.bc[c])
                ax = np.abs(U.xc[c])
                Msc_c += float((2 * lam * ax + L.Mbc[c]) @ MC + ax @ (lam * ax + L.Mbc[c]))
            Mstep = 0.0
            for c in range(self.C):
                if not self.cam_fixed[c]:
                    U.cam_T[c], M = oplus(self.cam_T[c], U.xc[c])
                    U.MCcam[c] = M + _pose_scale(U.cam_T[c], U.MCxc[c])
                    Mstep += 2 * float(L.Mbc[c] @ U.MCxc[c])
            for o in self.free_obj:
                U.obj_T[o], M = oplus(self.obj_T[o], U.xo[o])
                U.MCobj[o] = M + _pose_scale(U.obj_T[o], U.MCxo[o])
                Mstep += 2 * float(L.Mbo[o] @ U.MCxo[o])
            U.ok = 1.0
            U.after = PhaseRef(self.P, U.cam_T, U.obj_T, info=self.info, chi2_only=True)
            chi1, Mchi1 = U.after.chi_total(robust_on, L.level)
            U.red = np.array([chi1, float(sc_c), 1.0, float(sc_o)])
            U.Mred = np.array([Mchi1 + Mstep, Msc_c, 0.0, Msc_o])
            return U


# ---- one reference per designed graph, shared by the CPU and the GPU module ---------------------------------------------------------------------------------------
LAMBDAS = ("lo", "one", "hi")                # 1e-5 maxdiag (computeLambdaInit), 1, 1e6 maxdiag; maxdiag = the largest |diag H| over all free vertices
STATES = [(robust_on, classified) for classified in (0, 1) for robust_on in (0, 1)]      # after classify(keep_all=1) / after classify(0)

# K_REF: the largest |NumpyPhases - mp| / (eps M) per buffer over every case, state and lambda, measured by tests/test_ba_phases_ref.py (which prints the table and
# holds it: a measurement above K_REF fails there).  K = max(8, 4 K_REF): the tolerance of the kernels, K eps M.  No figure here comes from a GPU run.
K_REF = {"chi2": 0.43, "lin": 4.0, "sch": 1.5, "red": 0.27, "poses": 1.0}      # measured: 0.426, 3.96, 1.43, 0.268, 0.996
K = {buf: max(8.0, 4.0 * k) for buf, k in K_REF.items()}


def tol(buf, M):
    return K[buf] * EPS * np.asarray(M, np.float64)


class CaseRef:
    """Everything the tests ask of one graph, computed on first use and kept."""

    def __init__(self, prob):
        self.prob = prob
        self.ref = PhaseRef(prob)
        self.chi2, self.Mchi2, self.inlier, self.chi2_mp = self.ref.classify()
        self._lin, self._sch, self._upd = {}, {}, {}

    def level(self, classified):
        return (1 - self.inlier) if classified else np.zeros(self.ref.E, np.uint8)

    def lin(self, robust_on, classified):
        key = (int(robust_on), int(classified))
        if key not in self._lin:
            self._lin[key] = self.ref.linearize(key[0], self.level(key[1]))
        return self._lin[key]

    def lam(self, robust_on, classified, which):
        md = self.lin(robust_on, classified).maxdiag
        return {"lo": 1e-5 * md, "one": 1.0, "hi": 1e6 * md, "zero": 0.0}[which]

    def sch(self, robust_on, classified, which):
        key = (int(robust_on), int(classified), which)
        if key not in self._sch:
            self._sch[key] = self.ref.schur(self.lin(*key[:2]), self.lam(*key))
        return self._sch[key]

    def upd(self, robust_on, classified, which):
        key = (int(robust_on), int(classified), which)
        if key not in self._upd:
            self._upd[key] = self.ref.solve_update(self.lin(*key[:2]), self.sch(*key), self.lam(*key), key[0])
        return self._upd[key]


_CASES = {}


def case(name):
    """The CaseRef of tests/ba_phase_cases.py's graph `name`, one per process."""
    if name not in _CASES:
        from tests import ba_phase_cases as PC
        _CASES[name] = CaseRef(PC.problem(name))
    return _CASES[name]


def threshold_edges(cr):
    """Three edges of a case for the classification's threshold test: the smallest chi2, the median and the largest."""
    order = np.argsort(cr.chi2)
    return [int(order[0]), int(order[len(order) // 2]), int(order[-1])]
