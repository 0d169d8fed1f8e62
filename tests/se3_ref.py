"""An exponential map that is no transcription of se3quat.h: the SE(3) left update T' = exp(u^) T in mpmath at 50 digits, u = (omega, upsilon).

oplus            Rodrigues in mp arithmetic (R = I + a Om + b Om^2, V = I + b Om + c Om^2 with a = sin th / th, b = (1 - cos th) / th^2, c = (th - sin th) / th^3,
                 below 1e-6 rad their series to th^8: truncation < 1e-60), T' = [R R_T | V upsilon + R t_T], rounded to float64 once, at the end.
oplus_expm       the same through mpmath's own matrix exponential of the 4x4 twist [[Om, upsilon], [0, 0]] -- no Rodrigues, no series of ours.  tests/test_se3_ref.py
                 holds the two together over the whole case table, and both against scipy.
oplus_shortcut   g2o's shortcut for theta < 1e-5 (se3quat.h:236-240), which is NOT the exponential: R = V = I + Om + Om^2, the Eigen quaternion of that R (trace > 0
                 form), normalised; then SE3Quat::operator*: R' = R(q) R_T, t' = V upsilon + R(q) t_T.  Every operation in mp: what the kernels' shortcut branch must
                 give up to float64 rounding.

The input rotation is taken as given: R_T is used as the matrix it is, not projected onto SO(3)."""
from __future__ import annotations

import mpmath as mp
import numpy as np

DPS = 50


def _skew(w):
    return mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def _split(T, u):
    T = np.asarray(T, np.float64).reshape(3, 4)
    u = np.asarray(u, np.float64).reshape(6)
    R = mp.matrix([[mp.mpf(float(T[r, c])) for c in range(3)] for r in range(3)])
    t = mp.matrix([mp.mpf(float(T[r, 3])) for r in range(3)])
    w = [mp.mpf(float(x)) for x in u[:3]]
    ups = mp.matrix([mp.mpf(float(x)) for x in u[3:]])
    return R, t, w, ups


def _join(R, t):
    out = np.zeros((3, 4))
    for r in range(3):
        for c in range(3):
            out[r, c] = float(R[r, c])
        out[r, 3] = float(t[r])
    return out


def coefficients(th):
    """(a, b, c) of Rodrigues' formulas at the angle th (mp)."""
    if th < mp.mpf("1e-6"):
        t2 = th * th
        a = 1 - t2 / 6 + t2 ** 2 / 120 - t2 ** 3 / 5040 + t2 ** 4 / 362880
        b = mp.mpf(1) / 2 - t2 / 24 + t2 ** 2 / 720 - t2 ** 3 / 40320 + t2 ** 4 / 3628800
        c = mp.mpf(1) / 6 - t2 / 120 + t2 ** 2 / 5040 - t2 ** 3 / 362880 + t2 ** 4 / 39916800
        return a, b, c
    s = mp.sin(th)
    return s / th, (1 - mp.cos(th)) / th ** 2, (th - s) / th ** 3


def exp_RV(w):
    """(R, V) of exp for the rotation vector w (three mp numbers)."""
    th = mp.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2)
    a, b, c = coefficients(th)
    Om = _skew(w)
    Om2 = Om * Om
    I = mp.eye(3)
    return I + a * Om + b * Om2, I + b * Om + c * Om2


def oplus_mp(T, u):
    """exp(u^) T as (R' [3x3 mp], t' [3 mp])."""
    with mp.workdps(DPS):
        R, t, w, ups = _split(T, u)
        Re, V = exp_RV(w)
        return Re * R, V * ups + Re * t


def oplus(T, u):
    """exp(u^) T, float64 [3,4]."""
    with mp.workdps(DPS):
        return _join(*oplus_mp(T, u))


def oplus_expm(T, u):
    """The same through mpmath.expm of the 4x4 twist."""
    with mp.workdps(DPS):
        R, t, w, ups = _split(T, u)
        X = mp.zeros(4)
        Om = _skew(w)
        for r in range(3):
            for c in range(3):
                X[r, c] = Om[r, c]
            X[r, 3] = ups[r]
        E = mp.expm(X, method="taylor")
        Re = E[0:3, 0:3]
        return _join(Re * R, E[0:3, 3] + Re * t)


def quat_to_R_mp(q):
    w, x, y, z = q
    return mp.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def oplus_shortcut(T, u):
    """g2o's theta < 1e-5 branch restated in mp (module doc), float64 [3,4]."""
    with mp.workdps(DPS):
        R, t, w, ups = _split(T, u)
        Om = _skew(w)
        Rs = mp.eye(3) + Om + Om * Om
        tr = Rs[0, 0] + Rs[1, 1] + Rs[2, 2]
        assert tr > 0
        s = mp.sqrt(tr + 1)
        q = [s / 2, (Rs[2, 1] - Rs[1, 2]) / (2 * s), (Rs[0, 2] - Rs[2, 0]) / (2 * s), (Rs[1, 0] - Rs[0, 1]) / (2 * s)]
        n = mp.sqrt(sum(x * x for x in q))
        Rq = quat_to_R_mp([x / n for x in q])
        return _join(Rq * R, Rs * ups + Rq * t)


def quat_to_R(q):
    """The textbook rotation matrix of a unit quaternion (w, x, y, z), float64."""
    w, x, y, z = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def errors(T, T_ref):
    """(max |dR|, max |dt| / max(1, |t_ref|_inf)) of a [3,4] pose against its reference."""
    T, T_ref = np.asarray(T).reshape(3, 4), np.asarray(T_ref).reshape(3, 4)
    return float(np.abs(T[:, :3] - T_ref[:, :3]).max()), float(np.abs(T[:, 3] - T_ref[:, 3]).max() / max(1.0, np.abs(T_ref[:, 3]).max()))
