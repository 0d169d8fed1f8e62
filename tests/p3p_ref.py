"""The complete solution set of a P3P problem in mpmath at 70 digits, from the definition and by a path unrelated to Lambda-Twist: no line of it is shared with
csrc/pnp.hip or oracle/pnp_oracle.c.

unknowns     the depths l1, l2, l3 along the unit bearings b_i = (u_i, v_i, 1) / |.|:   l_i^2 + l_j^2 - 2 c_ij l_i l_j = a_ij,  c_ij = b_i . b_j,  a_ij = |x_i - x_j|^2
elimination  Grunert's substitution l2 = u l1, l3 = v l1 leaves two conics in (u, v),
                 a13 (1 + u^2 - 2 c12 u) = a12 (1 + v^2 - 2 c13 v)        a23 (1 + u^2 - 2 c12 u) = a12 (u^2 + v^2 - 2 c23 u v),
             whose resultant in u is a quartic in v; mp.polyroots solves it.  EVERY root is kept with its imaginary part.
back         u is the common root of the two conics at v (their difference is linear in u), l1^2 = a12 / (1 + u^2 - 2 c12 u); a real (u, v) gives the depth triple
             (l1, u l1, v l1) and its negative.
pose         by the definition: R maps the frame (d12, d13, d12 x d13) of the model points onto the frame of the camera points l_i b_i, t = l1 b1 - R x1.
self-check   every real solution returned satisfies the three equations (relative to the largest a_ij) and R'R = I to 1e-40; solve() raises otherwise.
edge margin  the smallest of: the relative gap between distinct real roots, |Im| / |root| over the non-real ones, and |depth| / (largest |depth| of the triple) over the
             depth triples of either sign.  A problem the elimination cannot pose (a vanishing a_ij, three equal bearings, a non-finite input, roots polyroots
             cannot separate) has margin 0.  Below EDGE a case is `on an edge`: the count of real positive solutions is not a stable property of its input.
fourth point for p4p: the reprojection error of point 3 under each all-positive solution and whether its z is positive."""
from __future__ import annotations

import mpmath as mp
import numpy as np

DPS = 70
EDGE = 1e-9          # edge margin below which a case is on an edge
REAL = mp.mpf("1e-45")      # |Im| / |root| below which a root is real
CHECK = mp.mpf("1e-40")


def _pmul(a, b):
    out = [mp.mpf(0)] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] += x * y
    return out


def _psub(a, b):
    n = max(len(a), len(b))
    a = a + [mp.mpf(0)] * (n - len(a))
    b = b + [mp.mpf(0)] * (n - len(b))
    return [x - y for x, y in zip(a, b)]


def _peval(p, v):
    return sum(c * v ** k for k, c in enumerate(p))


def _vec(v):
    return [x if isinstance(x, mp.mpf) else mp.mpf(float(x)) for x in v]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _sub(a, b):
    return [a[k] - b[k] for k in range(3)]


def _unit(v):
    n = mp.sqrt(_dot(v, v))
    return [x / n for x in v]


def _pose(lam, b, x, Xinv):
    """R, t from three depths by the definition."""
    p = [[lam[i] * b[i][k] for k in range(3)] for i in range(3)]
    e1, e2 = _sub(p[0], p[1]), _sub(p[0], p[2])
    Y = mp.matrix([[e1[r], e2[r], _cross(e1, e2)[r]] for r in range(3)])
    R = Y * Xinv
    t = [p[0][r] - sum(R[r, k] * x[0][k] for k in range(3)) for r in range(3)]
    return R, t


def solve(xs, ys):
    """xs [>=3][3], ys [>=3][2] (doubles, or mp numbers).  Returns a dict:
         posed      False when the elimination cannot be posed or its answers cannot be verified next to a repeated root (then margin = 0 and sols = [])
         framed     False when the model triple is exactly collinear: the depths exist, R and t of every solution are None
         roots      the roots v of the quartic (mp complex)
         sols       real solutions: dict(lam, R (mp.matrix), t, positive) -- both signs of every real root
         margin     the edge margin (float)
         coeffs     (a12, a13, a23, c12, c13, c23) in mp
    A solution that fails its own check away from an edge is recomputed once at three times the digits (an almost singular model frame costs digits); if it
    fails again, AssertionError."""
    try:
        return _solve(xs, ys, DPS)
    except AssertionError:
        return _solve(xs, ys, 3 * DPS)


def _solve(xs, ys, dps):
    with mp.workdps(dps):
        xin, yin = xs, ys                 # (doubles, or mp numbers from a test that plants an exact pose)
        xs, ys = np.array([[float(v) for v in r] for r in xin]), np.array([[float(v) for v in r] for r in yin])
        out = {"posed": False, "framed": False, "roots": [], "sols": [], "margin": 0.0, "coeffs": None}
        if not (np.isfinite(xs[:3]).all() and np.isfinite(ys[:3]).all()):
            return out
        x = [_vec(xin[i]) for i in range(3)]
        b = [_unit(_vec([yin[i][0], yin[i][1], 1.0])) for i in range(3)]
        c12, c13, c23 = _dot(b[0], b[1]), _dot(b[0], b[2]), _dot(b[1], b[2])
        d12, d13, d23 = _sub(x[0], x[1]), _sub(x[0], x[2]), _sub(x[1], x[2])
        a12, a13, a23 = _dot(d12, d12), _dot(d13, d13), _dot(d23, d23)
        out["coeffs"] = (a12, a13, a23, c12, c13, c23)
        n = _cross(d12, d13)
        amax = max(a12, a13, a23)
        if min(a12, a13, a23) == 0 or (np.array_equal(ys[0], ys[1]) and np.array_equal(ys[0], ys[2])):
            return out
        framed = _dot(n, n) != 0             # an exactly collinear triple has depths but no pose: R and t of its solutions are None
        out["framed"] = framed
        Xinv = mp.matrix([[d12[r], d13[r], n[r]] for r in range(3)]) ** -1 if framed else None
        # conics as polynomials in u whose coefficients are polynomials in v (lowest power first)
        p2, p1, p0 = [a13], [-2 * a13 * c12], [a13 - a12, 2 * a12 * c13, -a12]
        q2, q1, q0 = [a23 - a12], [-2 * a23 * c12, 2 * a12 * c23], [a23, mp.mpf(0), -a12]
        A = _psub(_pmul(p2, q0), _pmul(p0, q2))
        B = _psub(_pmul(p2, q1), _pmul(p1, q2))
        Cc = _psub(_pmul(p1, q0), _pmul(p0, q1))
        res = _psub(_pmul(A, A), _pmul(B, Cc))
        big = max(abs(c) for c in res)
        while len(res) > 1 and abs(res[-1]) <= big * mp.mpf("1e-60"):
            res.pop()
        if len(res) < 2:
            return out
        try:
            roots = mp.polyroots(res[::-1], maxsteps=400, extraprec=6 * dps)
        except mp.libmp.libhyper.NoConvergence:
            return out
        out["roots"] = roots
        margin = mp.mpf(1)
        real = []
        for r in roots:
            if abs(mp.im(r)) <= REAL * max(abs(r), mp.mpf("1e-30")):
                real.append(mp.re(r))
            else:
                margin = min(margin, abs(mp.im(r)) / abs(r))
        for i in range(len(real)):
            for j in range(i + 1, len(real)):
                margin = min(margin, abs(real[i] - real[j]) / max(abs(real[i]), abs(real[j])))
        sols = []
        for v in real:
            den = _peval(B, v)
            if abs(den) <= mp.mpf("1e-50") * amax * amax:      # the conics share both roots in u at this v: the problem is not generic
                return out
            u = -_peval(A, v) / den
            w = 1 + u * u - 2 * c12 * u
            if w <= 0:
                return out
            l1 = mp.sqrt(a12 / w)
            lam = [l1, u * l1, v * l1]
            top = max(abs(z) for z in lam)
            margin = min(margin, min(abs(z) for z in lam) / top)
            for sg in (1, -1):
                L = [sg * z for z in lam]
                eq = max(abs(L[0] ** 2 + L[1] ** 2 - 2 * c12 * L[0] * L[1] - a12), abs(L[0] ** 2 + L[2] ** 2 - 2 * c13 * L[0] * L[2] - a13),
                         abs(L[1] ** 2 + L[2] ** 2 - 2 * c23 * L[1] * L[2] - a23)) / amax
                R, t = _pose(L, b, x, Xinv) if framed else (None, None)
                orth = max(abs(z) for z in (R.T * R - mp.eye(3))) if framed else 0
                if eq > CHECK or orth > CHECK:
                    if margin < EDGE:            # next to a repeated root polyroots' digits run out: the case is on an edge, nothing is claimed of it
                        return out
                    raise AssertionError(f"p3p_ref: a solution fails its own check: equations {mp.nstr(eq, 3)}, R'R - I {mp.nstr(orth, 3)}")
                sols.append({"lam": L, "R": R, "t": t, "positive": all(z > 0 for z in L)})
        out.update(posed=True, sols=sols, margin=float(margin))
        return out


def fourth_point(sol, x3, y3):
    """(reprojection error of point 3 as p4p measures it, z > 0) under one solution, in mp; (None, False) for a non-finite image point."""
    with mp.workdps(DPS):
        if sol["R"] is None:
            return None, False
        X = _vec(x3)
        p = [sum(sol["R"][r, k] * X[k] for k in range(3)) + sol["t"][r] for r in range(3)]
        if not np.isfinite([float(v) for v in y3]).all() or p[2] == 0:
            return None, bool(p[2] > 0)
        Y = _vec(y3)
        e = (p[0] / p[2] - Y[0]) ** 2 + (p[1] / p[2] - Y[1]) ** 2
        return e, bool(p[2] > 0)


def as_float(sol):
    """R [3,3], t [3] of a solution as doubles."""
    return np.array([[float(sol["R"][r, c]) for c in range(3)] for r in range(3)]), np.array([float(z) for z in sol["t"]])


def pose_err(R, t, sol, xmax):
    """The error rule of tests/test_gpu_p3p.py: max(|R - R_mp|_max, |t - t_mp|_inf / max(|t_mp|_inf, |x|_max)), the differences taken in mp."""
    with mp.workdps(DPS):
        if sol["R"] is None or not (np.isfinite(R).all() and np.isfinite(t).all()):
            return float("inf")
        R = np.asarray(R, np.float64).reshape(3, 3)
        eR = max(abs(mp.mpf(float(R[r, c])) - sol["R"][r, c]) for r in range(3) for c in range(3))
        et = max(abs(mp.mpf(float(t[r])) - sol["t"][r]) for r in range(3))
        tn = max(max(abs(z) for z in sol["t"]), mp.mpf(float(xmax)))
        return float(max(eR, et / tn))


def quat_branch(R, tie=1e-9):
    """The branches rot_to_quat (p4p.cpp's matrix-to-quaternion conversion) can enter for rotation R (doubles or mp): a set of 0 (trace), 1, 2, 3.  Comparisons of
    diagonal entries closer than `tie` may fall either way in doubles, so both orders are returned."""
    d = [float(R[0, 0]), float(R[1, 1]), float(R[2, 2])]
    if d[0] + d[1] + d[2] + 1.0 > 1e-7:
        return {0}

    def gt(a, b):
        return {True, False} if abs(a - b) < tie else {a > b}
    out = set()
    for c01 in gt(d[0], d[1]):
        for c02 in gt(d[0], d[2]):
            if c01 and c02:
                out.add(1)
            else:
                for c12 in gt(d[1], d[2]):
                    out.add(2 if c12 else 3)
    return out


def cubic_branch(coeffs):
    """Which entry branch of Lambda-Twist's cubic solver the problem takes, from the mp coefficients of its cubic g^3 + b g^2 + c g + d (the cubic is the published
    one, lambdatwist.p3p.h; only its three coefficients are formed here): 'two-extrema-left' (b^2 >= 3c and the cubic is positive at its left extremum),
    'two-extrema-right' (b^2 >= 3c, not positive there), 'monotone' (b^2 < 3c)."""
    with mp.workdps(DPS):
        a12, a13, a23, c12, c13, c23 = coeffs
        blob = c12 * c23 * c13 - 1
        s13, s23, s12 = 1 - c13 * c13, 1 - c23 * c23, 1 - c12 * c12
        p3 = a13 * (a23 * s13 - a13 * s23)
        if p3 == 0:
            return None
        b = (2 * blob * a23 * a13 + a13 * (2 * a12 + a13) * s23 + a23 * (a23 - a12) * s13) / p3
        c = (a23 * (a13 - a23) * s12 - a12 * a12 * s23 - 2 * a12 * (blob * a23 + a13 * s23)) / p3
        d = a12 * (a12 * s23 - a23 * s12) / p3
        if b * b < 3 * c:
            return "monotone"
        t1 = (-b - mp.sqrt(b * b - 3 * c)) / 3
        return "two-extrema-left" if ((t1 + b) * t1 + c) * t1 + d > 0 else "two-extrema-right"
