"""PNP::refine restated from its definitions in mpmath at 40 digits -- no transcription of csrc/pnp.hip or oracle/pnp_oracle.c.

residual     PnPReprojectionError (pnp_ransac.cpp:96-156): x / z - y per point, (x, y, z) = R(q) X + t with cvl::Pose::getR = getRotationMatrix(q)
             (rotation_helpers.h:213-241: the homogeneous form aa + bb - cc - dd ..., q NOT normalised).
update       ceres::QuaternionParameterization: q (+) d = [cos |d|, sin |d| / |d| d] (x) q; the translation is additive.
jacobian     with respect to the six local coordinates at d = 0 by mp CENTRAL DIFFERENCES of that residual under that update (step 1e-15 at 40 digits: relative
             error near 1e-30).  Nothing here differentiates by hand; analytic_jacobian exists only so that tests/test_pnp_refine_ref.py can hold the two together.
system       H = J'J, g = J'r, cost = 1/2 sum |r|^2 over a selection, and the scales assertion (a) of tests/test_gpu_pnp_refine.py measures errors in.
rules        count_rule (evaluate_inlier_set, pnp_ransac.cpp:41-87: 1 / z < 0 skips, err < thr^2 counts) and select_rule (PNP::refine, :240-326: z < 0 drops,
             err > thr^2 drops), with IEEE's answers where z is a zero: 1 / -0.0 = -inf skips in the first rule, -0.0 < 0 is false in the second; x * (+-inf) is
             +-inf (err = inf: no inlier by either rule) unless x or y is 0, where err is NaN: NaN < thr^2 is false (not counted), NaN > thr^2 is false (SELECTED).
             second_pass_rule: `deltas < 0.05 * m` skips the second pass -- a comparison of an int with a double product, evaluated in doubles as the reference does.
lm           the trust-region algorithm the header of oracle/pnp_oracle.c specifies (the project's statement of Ceres' behaviour), in mp, returning the margin of
             every decision it took.  sequence chains select -> lm(5, 1e-6) -> reselect -> optional lm(3, 1e-8).
minimiser    damped Gauss-Newton on the same cost to a gradient below 1e-30."""
from __future__ import annotations

import mpmath as mp
import numpy as np

DPS = 40
FD_STEP = "1e-15"
NEAR = 1e-6          # a decision within this relative distance of its threshold makes a row `near`


def mpf(x):
    return mp.mpf(float(x))


def mpv(v):
    return [mpf(x) for x in np.asarray(v, np.float64).ravel()]


def rot(q):
    a, b, c, d = q
    aa, ab, ac, ad, bb, bc, bd, cc, cd, dd = a * a, a * b, a * c, a * d, b * b, b * c, b * d, c * c, c * d, d * d
    return [[aa + bb - cc - dd, 2 * (bc - ad), 2 * (ac + bd)],
            [2 * (ad + bc), aa - bb + cc - dd, 2 * (cd - ab)],
            [2 * (bd - ac), 2 * (ab + cd), aa - bb - cc + dd]]


def quat_mul(a, b):
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
            a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
            a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]]


def plus(q, t, d):
    """(q, t) (+) d, d = three rotation coordinates then the translation step."""
    n = mp.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    if n == 0:
        qn = list(q)
    else:
        s = mp.sin(n) / n
        qn = quat_mul([mp.cos(n), s * d[0], s * d[1], s * d[2]], q)
    return qn, [t[k] + d[3 + k] for k in range(3)]


def camera_points(q, t, X):
    R = rot(q)
    return [[R[r][0] * p[0] + R[r][1] * p[1] + R[r][2] * p[2] + t[r] for r in range(3)] for p in X]


def residuals(q, t, X, Y):
    """[(r0, r1)] per point, or None where a point has z = 0 (the residual is not finite)."""
    out = []
    for p, y in zip(camera_points(q, t, X), Y):
        if p[2] == 0:
            return None
        iz = 1 / p[2]
        out.append((p[0] * iz - y[0], p[1] * iz - y[1]))
    return out


class Problem:
    """The points of one object as mp numbers (converted once) next to the float64 arrays they came from."""

    def __init__(self, xs, ys, thr):
        self.xs = np.ascontiguousarray(xs, np.float64).reshape(-1, 3)
        self.ys = np.ascontiguousarray(ys, np.float64).reshape(-1, 2)
        self.n = len(self.xs)
        self.thr = float(thr)
        with mp.workdps(DPS):
            self.X = [mpv(p) for p in self.xs]
            self.Y = [mpv(p) for p in self.ys]
            self.thr2 = mpf(thr) * mpf(thr)

    def pick(self, sel):
        idx = [i for i in range(self.n) if sel[i]]
        return [self.X[i] for i in idx], [self.Y[i] for i in idx]


def cost(P, q, t, sel):
    """1/2 sum |r|^2 over the selection; mp.inf where it is not finite."""
    with mp.workdps(DPS):
        X, Y = P.pick(sel)
        r = residuals(q, t, X, Y)
        if r is None:
            return mp.inf
        return sum((a * a + b * b for a, b in r), mp.mpf(0)) / 2


def cost_and_scale(P, q, t, sel):
    """(cost, sum |r| (|pi| + |y|)): the cost and the unit its rounding error is measured in; (inf, 0) where it is not finite."""
    with mp.workdps(DPS):
        X, Y = P.pick(sel)
        r = residuals(q, t, X, Y)
        if r is None:
            return mp.inf, mp.mpf(0)
        c, sc = mp.mpf(0), mp.mpf(0)
        for ri, y in zip(r, Y):
            c += (ri[0] * ri[0] + ri[1] * ri[1]) / 2
            sc += mp.sqrt(ri[0] ** 2 + ri[1] ** 2) * (mp.sqrt((ri[0] + y[0]) ** 2 + (ri[1] + y[1]) ** 2) + mp.sqrt(y[0] ** 2 + y[1] ** 2))
        return c, sc


def jacobian(q, t, X, Y):
    """[n][2][6] by central differences of the residual under the local update."""
    h = mp.mpf(FD_STEP)
    cols = []
    for a in range(6):
        d = [mp.mpf(0)] * 6
        d[a] = h
        rp = residuals(*plus(q, t, d), X, Y)
        d[a] = -h
        rm = residuals(*plus(q, t, d), X, Y)
        cols.append([((p[0] - m[0]) / (2 * h), (p[1] - m[1]) / (2 * h)) for p, m in zip(rp, rm)])
    return [[[cols[a][i][k] for a in range(6)] for k in range(2)] for i in range(len(X))]


def analytic_jacobian(q, t, X, Y):
    """The same by hand (chain rule through the projection; a rotation by dq turns R X by the angle 2 |d| about d): for tests of jacobian only."""
    out = []
    for p in camera_points(q, t, X):
        rx, ry, rz = p[0] - t[0], p[1] - t[1], p[2] - t[2]
        iz = 1 / p[2]
        Pm = [[iz, 0, -p[0] * iz * iz], [0, iz, -p[1] * iz * iz]]
        D = [[0, 2 * rz, -2 * ry, 1, 0, 0], [-2 * rz, 0, 2 * rx, 0, 1, 0], [2 * ry, -2 * rx, 0, 0, 0, 1]]
        out.append([[sum(Pm[k][j] * D[j][a] for j in range(3)) for a in range(6)] for k in range(2)])
    return out


def system(P, q, t, sel):
    """dict H [6][6], g [6], cost and the error units of assertion (a): sg2 = sum (|pi| + |y|)^2, sc = sum |r| (|pi| + |y|).  None where not finite."""
    with mp.workdps(DPS):
        X, Y = P.pick(sel)
        r = residuals(q, t, X, Y)
        if r is None:
            return None
        J = jacobian(q, t, X, Y) if X else []
        H = [[sum((Ji[0][a] * Ji[0][c] + Ji[1][a] * Ji[1][c] for Ji in J), mp.mpf(0)) for c in range(6)] for a in range(6)]
        g = [sum((Ji[0][a] * ri[0] + Ji[1][a] * ri[1] for Ji, ri in zip(J, r)), mp.mpf(0)) for a in range(6)]
        c = sum((a * a + b * b for a, b in r), mp.mpf(0)) / 2
        sg2, sc = mp.mpf(0), mp.mpf(0)
        for ri, y in zip(r, Y):
            pi = mp.sqrt((ri[0] + y[0]) ** 2 + (ri[1] + y[1]) ** 2)
            w = pi + mp.sqrt(y[0] ** 2 + y[1] ** 2)
            sg2 += w * w
            sc += mp.sqrt(ri[0] ** 2 + ri[1] ** 2) * w
        return {"H": H, "g": g, "cost": c, "sg2": sg2, "sc": sc, "n_sel": len(X)}


# ---------------------------------------------------------------------------------------------------------------- rules
def _point_errors(P, q, t):
    """Per point: (z, err, kind) with kind 'ok', 'inf' (z = 0, err infinite) or 'nan' (z = 0 and x or y = 0).  The sign of a zero z changes neither rule's
    answer: -0.0 is skipped by the first (1 / z = -inf) where +0.0 gives an err that is not < thr^2; the second sees z < 0 false for both."""
    out = []
    for p, y in zip(camera_points(q, t, P.X), P.Y):
        if p[2] == 0:
            out.append((p[2], None, "nan" if (p[0] == 0 or p[1] == 0) else "inf"))
        else:
            iz = 1 / p[2]
            e0, e1 = p[0] * iz - y[0], p[1] * iz - y[1]
            out.append((p[2], e0 * e0 + e1 * e1, "ok"))
    return out


def _near(err, thr2):
    return err is not None and abs(err - thr2) <= NEAR * thr2


def count_rule(P, q, t):
    """evaluate_inlier_set with best_inliers = 0: (flags, near)."""
    with mp.workdps(DPS):
        flags, near = [], False
        for z, err, kind in _point_errors(P, q, t):
            if kind != "ok":
                flags.append(0)                      # -0.0: 1 / z = -inf < 0 skips; +0.0: err is inf or NaN, neither is < thr^2
            elif z < 0:
                flags.append(0)
            else:
                flags.append(1 if err < P.thr2 else 0)
                near = near or _near(err, P.thr2)
        return flags, near


def select_rule(P, q, t):
    """The selection of PNP::refine: (flags, near)."""
    with mp.workdps(DPS):
        flags, near = [], False
        for z, err, kind in _point_errors(P, q, t):
            if kind == "nan":
                flags.append(1)                      # z = +-0.0 is not < 0, and NaN > thr^2 is false
            elif kind == "inf":
                flags.append(0)
            elif z < 0:
                flags.append(0)
            else:
                flags.append(0 if err > P.thr2 else 1)
                near = near or _near(err, P.thr2)
        return flags, near


def second_pass_rule(deltas, m):
    """True when the second pass runs: the reference returns early on `deltas < 0.05 * m`, int against double."""
    return not (float(deltas) < 0.05 * float(m))


# ---------------------------------------------------------------------------------------------------------------- the algorithm
def _cholesky_solve(A, b):
    """(x, pivots) of A x = b; x is None when a pivot is not positive."""
    L = [[mp.mpf(0)] * 6 for _ in range(6)]
    piv = []
    for i in range(6):
        for j in range(i + 1):
            s = A[i][j] - sum((L[i][k] * L[j][k] for k in range(j)), mp.mpf(0))
            if i == j:
                piv.append(s)
                if not s > 0:
                    return None, piv
                L[i][i] = mp.sqrt(s)
            else:
                L[i][j] = s / L[j][j]
    y = [mp.mpf(0)] * 6
    for i in range(6):
        y[i] = (b[i] - sum((L[i][k] * y[k] for k in range(i)), mp.mpf(0))) / L[i][i]
    x = [mp.mpf(0)] * 6
    for i in range(5, -1, -1):
        x[i] = (y[i] - sum((L[k][i] * x[k] for k in range(i + 1, 6)), mp.mpf(0))) / L[i][i]
    return x, piv


def _rel(v, thr):
    return float(abs(v - thr) / abs(thr)) if thr != 0 else float(abs(v))


def lm(P, q, t, sel, max_iter, tol):
    """The trust-region pass.  Returns dict q, t (mp), stop in {'gradient', 'function', 'parameter', 'cap', 'radius', 'empty', 'nonfinite'}, traj [(q, t)] of the
    accepted poses, accepted / rejected counts, behind (trial poses with a selected point at or behind the camera plane) and margins [(name, relative distance of the deciding value from its threshold)]."""
    with mp.workdps(DPS):
        q, t = list(q), list(t)
        tol = mpf(tol)
        out = {"traj": [], "margins": [], "accepted": 0, "rejected": 0, "behind": 0}

        def end(stop):
            out.update(q=q, t=t, stop=stop)
            return out
        if not any(sel):
            return end("empty")
        c = cost(P, q, t, sel)
        if c == mp.inf:
            return end("nonfinite")
        radius, decrease = mp.mpf(10) ** 4, mp.mpf(2)
        for _ in range(max_iter):
            S = system(P, q, t, sel)
            out.setdefault("system0", S)
            H, g = S["H"], S["g"]
            gmax = max(abs(v) for v in g)
            out["margins"].append(("gmax - tol", _rel(gmax, tol)))
            if gmax <= tol:
                return end("gradient")
            A = [row[:] for row in H]
            for a in range(6):
                A[a][a] += min(max(H[a][a], mp.mpf("1e-12")), mp.mpf("1e64")) / radius
            step, piv = _cholesky_solve(A, [-v for v in g])
            for a, p in enumerate(piv):
                out["margins"].append((f"pivot {a}", float(abs(p) / A[a][a]) if A[a][a] != 0 else 0.0))
            ok = step is not None
            rho, new_c = mp.mpf(-1), c
            if ok:
                model = sum((-step[a] * (g[a] + sum((H[a][k] * step[k] for k in range(6)), mp.mpf(0)) / 2) for a in range(6)), mp.mpf(0))
                qn, tn = plus(q, t, step)
                new_c = cost(P, qn, tn, sel)
                if min(p[2] for p in camera_points(qn, tn, P.pick(sel)[0])) <= 0:
                    out["behind"] += 1
                if new_c != mp.inf:
                    rho = (c - new_c) / model if model > 0 else mp.mpf(-1)
                    if model > 0:
                        out["margins"].append(("rho - 1e-3", _rel(rho, mp.mpf("1e-3"))))
            if ok and new_c != mp.inf and rho > mp.mpf("1e-3"):
                snorm = mp.sqrt(sum((v * v for v in step), mp.mpf(0)))
                xnorm = mp.sqrt(sum((v * v for v in q + t), mp.mpf(0)))
                dc = c - new_c
                q, t = qn, tn
                out["traj"].append((q, t))
                out["accepted"] += 1
                out["margins"].append(("|dc| - tol cost", _rel(abs(dc), tol * c)))
                out["margins"].append(("|step| - 1e-8 (|x| + 1e-8)", _rel(snorm, mp.mpf("1e-8") * (xnorm + mp.mpf("1e-8")))))
                f_done, p_done = abs(dc) <= tol * c, snorm <= mp.mpf("1e-8") * (xnorm + mp.mpf("1e-8"))
                c = new_c
                radius = min(radius / max(mp.mpf(1) / 3, 1 - (2 * rho - 1) ** 3), mp.mpf(10) ** 16)
                decrease = mp.mpf(2)
                if f_done or p_done:
                    return end("function" if f_done else "parameter")
            else:
                out["rejected"] += 1
                radius /= decrease
                decrease *= 2
                if radius < mp.mpf("1e-32"):
                    return end("radius")
        return end("cap")


def sequence(P, q, t):
    """select -> lm(5, 1e-6) -> reselect -> lm(3, 1e-8) unless fewer than 5 % of the flags changed."""
    with mp.workdps(DPS):
        sel0, near0 = select_rule(P, q, t)
        first = lm(P, q, t, sel0, 5, 1e-6)
        sel1, near1 = select_rule(P, first["q"], first["t"])
        m, deltas = sum(sel1), sum(1 for a, b in zip(sel0, sel1) if a != b)
        second = second_pass_rule(deltas, m)
        last = lm(P, first["q"], first["t"], sel1, 3, 1e-8) if second else None
        return {"sel0": sel0, "sel1": sel1, "m0": sum(sel0), "m": m, "deltas": deltas, "second": second, "first": first, "last": last,
                "q": (last or first)["q"], "t": (last or first)["t"], "near_rules": near0 or near1,
                "margins": first["margins"] + (last["margins"] if last else []) + [("deltas - 0.05 m", float(deltas) - 0.05 * float(m))]}


def is_near(margins):
    """A row is `near` when a floating decision of its mp run lies within NEAR of its threshold (the integer rule deltas < 0.05 m has no rounding to be near to)."""
    return any(v <= NEAR for name, v in margins if not name.startswith("deltas"))


def hessian(P, q, t, sel):
    """The full Hessian of the cost in the local coordinates at (q, t), by central differences of the gradient (step 1e-12: relative error near 1e-24)."""
    with mp.workdps(DPS):
        h = mp.mpf("1e-12")
        cols = []
        for a in range(6):
            d = [mp.mpf(0)] * 6
            d[a] = h
            gp = system(P, *plus(q, t, d), sel)["g"]
            d[a] = -h
            gm = system(P, *plus(q, t, d), sel)["g"]
            cols.append([(x - y) / (2 * h) for x, y in zip(gp, gm)])
        return [[(cols[a][c] + cols[c][a]) / 2 for c in range(6)] for a in range(6)]


def minimiser(P, q, t, sel, max_iter=40):
    """minimiser_at_working_precision at 60 digits with a difference step of 1e-22: at 40 digits the central differences' own truncation (1e-30 relative) is the size
    of the gradient asked for."""
    global DPS, FD_STEP
    saved = DPS, FD_STEP
    DPS, FD_STEP = 60, "1e-22"
    try:
        return minimiser_at_working_precision(P, q, t, sel, max_iter)
    finally:
        DPS, FD_STEP = saved


def minimiser_at_working_precision(P, q, t, sel, max_iter=40):
    """From (q, t) to |g|_inf < 1e-30: Gauss-Newton while it gains a digit per step, else Newton with the full Hessian; steps halved while the cost rises.
    dict q, t, g, H (Gauss-Newton's J'J), iterations, converged."""
    with mp.workdps(DPS):
        q, t = list(q), list(t)
        c = cost(P, q, t, sel)
        last, newton = None, False
        for it in range(max_iter):
            S = system(P, q, t, sel)
            gmax = max(abs(v) for v in S["g"])
            if gmax < mp.mpf("1e-30"):
                return {"q": q, "t": t, "g": S["g"], "H": S["H"], "iterations": it, "converged": True}
            newton = newton or (last is not None and gmax > last / 10)
            last = gmax
            step, _ = _cholesky_solve(hessian(P, q, t, sel) if newton else S["H"], [-v for v in S["g"]])
            if step is None:
                break
            k = mp.mpf(1)
            for _ in range(40):
                qn, tn = plus(q, t, [k * v for v in step])
                cn = cost(P, qn, tn, sel)
                if cn <= c or gmax < mp.mpf("1e-18"):          # (near the minimum the cost no longer resolves the gain: take the step)
                    break
                k /= 2
            q, t, c = qn, tn, cn
        S = system(P, q, t, sel)
        return {"q": q, "t": t, "g": S["g"], "H": S["H"], "iterations": max_iter, "converged": False}


def is_positive_definite(H):
    with mp.workdps(DPS):
        return _cholesky_solve(H, [mp.mpf(0)] * 6)[0] is not None


def pose_distance(q_a, t_a, q_b, t_b):
    """(dR, dt): max |R(q_a) - R(q_b)| and max |t_a - t_b|, in mp, returned as floats."""
    with mp.workdps(DPS):
        Ra, Rb = rot([mp.mpf(v) for v in q_a]), rot([mp.mpf(v) for v in q_b])
        dR = max(abs(Ra[r][c] - Rb[r][c]) for r in range(3) for c in range(3))
        dt = max(abs(mp.mpf(a) - mp.mpf(b)) for a, b in zip(t_a, t_b))
        return float(dR), float(dt)
