"""The designed case table of the SE(3) update (csrc/lm_device.h: pose_from_T, pose_oplus, R_to_q, pose_to_T): rows (T [3,4], u [6] = (omega, upsilon), why).

tests/test_se3_ref.py measures the C oracle and the numpy restatement over it on the CPU, tests/test_gpu_se3_update.py the kernels' own functions in one launch.
Built once at import from fixed seeds: the same arrays in every process.

Angles |omega|: 0, 1e-200 and 1e-160 (th^2 underflows to 0, to a denormal), both sides of the shortcut threshold 1e-5 -- but nothing inside 1e-5 (1 +- 1e-6): the kernel tests th^2 < 1e-10, the
oracle sqrt(th^2) < 1e-5, and the two forms they choose between differ by th^2 / 2 in R, so the side a value within an ulp of the threshold lands on is no parity
property -- the Taylor range up to both sides of 0.3, the closed forms, both sides of 2 pi / 3 (where the trace of exp changes sign and R_to_q its form), pi, 2 pi
and beyond.  Axes: +-x, +-y, +-z (beyond 2 pi / 3: each of the three pivot forms), the three face diagonals (which tie R_to_q's diagonal comparisons), random."""
from __future__ import annotations

import numpy as np

TWO_PI_3 = 2.0 * np.pi / 3.0
BAND = (1e-5 * (1 - 1e-6), 1e-5 * (1 + 1e-6))

ANGLES = [0.0, 1e-200, 1e-160, 1e-8, 1e-6, 5e-6, 1e-5 * (1 - 1e-3), 1e-5 * (1 - 1e-5), 1e-5 * (1 + 1e-5), 1.001e-5, 2e-5, 1e-4, 1e-3, 0.01, 0.1, 0.25,
          0.3 - 1e-3, 0.3 * (1 - 1e-9), 0.3 * (1 + 1e-9), 0.3 + 1e-3, 0.5, 1.0, 2.0,
          TWO_PI_3 - 1e-3, TWO_PI_3 - 1e-9, TWO_PI_3 + 1e-9, TWO_PI_3 + 1e-3, 3.0, np.pi - 1e-6, np.pi, np.pi + 1e-6, 5.0, 2 * np.pi - 1e-6, 2 * np.pi, 7.0]


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def rot(axis, angle):
    """Rotation matrix by `angle` about `axis`, from its unit quaternion (orthonormal to rounding)."""
    n = _unit(axis)
    w, (x, y, z) = np.cos(angle / 2), np.sin(angle / 2) * n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _pose(R, t):
    return np.hstack([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)])


def _build():
    rng = np.random.default_rng(20240611)
    E = np.eye(3)
    axes = [("+x", E[0]), ("-x", -E[0]), ("+y", E[1]), ("-y", -E[1]), ("+z", E[2]), ("-z", -E[2]),
            ("xy", _unit([1, 1, 0])), ("yz", _unit([0, 1, 1])), ("xz", _unit([1, 0, 1]))]
    axes += [(f"rand{i}", _unit(rng.standard_normal(3))) for i in range(3)]

    # ---- input poses ----
    rots = [("identity", np.eye(3))]
    while len(rots) < 4:                                            # random, trace > 0
        R = rot(rng.standard_normal(3), rng.uniform(0.2, 1.8))
        if np.trace(R) > 0.2:
            rots.append((f"trace>0 #{len(rots)}", R))
    for i, name in enumerate("xyz"):                                # random, trace <= 0, R[i,i] the largest diagonal entry: pivot form i
        while True:
            R = rot(E[i] + 0.25 * rng.standard_normal(3), rng.uniform(2.3, 3.0))
            d = np.diag(R)
            if np.trace(R) < -0.1 and d.argmax() == i and d[i] - np.delete(d, i).max() > 0.1:
                break
        rots.append((f"trace<=0 pivot {name}", R))
    rots += [("half turn x", np.diag([1.0, -1.0, -1.0])), ("half turn y", np.diag([-1.0, 1.0, -1.0])), ("half turn z", np.diag([-1.0, -1.0, 1.0]))]
    t_norms = [0.0, 1.0, 1e3, 1e4]
    upsilons = [np.zeros(3), np.full(3, 1e-3), np.ones(3), np.full(3, 1e3), np.array([100.0, -60.0, 30.0]), np.array([-1e-3, 1.0, -1e3])]

    rows = []

    def add(R, t, w, ups, why):
        rows.append((_pose(R, t), np.r_[np.asarray(w, np.float64), np.asarray(ups, np.float64)], why))

    # 1. every angle on every axis; the pose, |t| and upsilon cycle (co-prime periods)
    k = 0
    for th in ANGLES:
        for an, ax in axes:
            rn, R = rots[k % len(rots)]
            tn = t_norms[(k // 3) % len(t_norms)]
            t = tn * _unit(rng.standard_normal(3))
            ups = upsilons[k % len(upsilons)] * rng.choice([-1.0, 1.0], 3)
            add(R, t, th * ax, ups, f"angle {th!r} axis {an}; T {rn}, |t| {tn:g}")
            k += 1
    # 2. every input pose kind at |t| 500, |upsilon| 100 and one angle of each branch of exp and of R_to_q
    for rn, R in rots:
        for th in (3e-6, 0.05, 0.25, 0.6, 2.5, 3.5):
            add(R, 500 * _unit(rng.standard_normal(3)), th * _unit(rng.standard_normal(3)), 100 * _unit(rng.standard_normal(3)), f"T {rn} at angle {th}")
    # 3. every |t| on every pose kind, no update rotation / a Taylor one
    for rn, R in rots:
        for tn in t_norms:
            for th in (0.0, 0.2):
                add(R, tn * _unit(rng.standard_normal(3)), th * _unit(rng.standard_normal(3)), rng.standard_normal(3), f"T {rn}, |t| {tn:g}, angle {th}")
    # 4. sign canonicalisation: T a rotation by alpha about n, the update by beta about the same n, alpha + beta > pi: the product quaternion has w < 0 before the
    #    flip; beta > pi: exp's own quaternion has w < 0 too
    for an, ax in axes[::2] + axes[-2:]:
        for alpha, beta in ((2.5, 1.0), (2.5, 2.0), (3.0, 0.25), (2.0, 3.5), (1.0, 5.0)):
            add(rot(ax, alpha), 300 * _unit(rng.standard_normal(3)), beta * ax, 10 * rng.standard_normal(3), f"w < 0 before the flip: {alpha} + {beta} about {an}")
    # 5. w = 0 to rounding: composite half turns
    for an, ax in axes[:6:2] + axes[6:]:
        for alpha in (2.0, 0.2, 2.9):
            add(rot(ax, alpha), 300 * _unit(rng.standard_normal(3)), (np.pi - alpha) * ax, 10 * rng.standard_normal(3), f"composite half turn {alpha} + (pi - {alpha}) about {an}")
    for i, j in ((0, 1), (1, 2), (2, 0)):                             # an exact half turn about e_i times a rotation about e_j: w = 0 exactly
        H = -np.eye(3)
        H[i, i] = 1.0
        for beta in (0.1, 1.0, 2.5):
            add(H, 300 * _unit(rng.standard_normal(3)), beta * E[j], 10 * rng.standard_normal(3), f"half turn about axis {i} times {beta} about axis {j}: w = 0")
    # 6. translations: upsilon per component 0, 1e-3, 1, 1e3 with and without rotation
    for c in (0.0, 1e-3, 1.0, 1e3):
        for th in (0.0, 3e-6, 0.2, 1.0, 2.8):
            for tn in (0.0, 1e3):
                add(rots[1][1], tn * _unit(rng.standard_normal(3)), th * _unit(rng.standard_normal(3)), np.full(3, c), f"upsilon {c:g} per component, angle {th}, |t| {tn:g}")
    return rows


ROWS = _build()
T_IN = np.ascontiguousarray(np.stack([r[0] for r in ROWS]))         # [n,3,4]
U = np.ascontiguousarray(np.stack([r[1] for r in ROWS]))            # [n,6]
WHY = [r[2] for r in ROWS]
ANGLE = np.linalg.norm(U[:, :3], axis=1)
TH2 = (U[:, 0] * U[:, 0] + U[:, 1] * U[:, 1]) + U[:, 2] * U[:, 2]   # as the kernel sums it
SHORTCUT = TH2 < 1e-10                                               # below the band: g2o's shortcut on both sides
TAYLOR = ~SHORTCUT & (TH2 < 0.09)
CLOSED = TH2 >= 0.09


def angle_class(th):
    """The class a row is reported under."""
    for hi, name in ((1e-5, "< 1e-5 (shortcut)"), (1e-3, "1e-5 .. 1e-3"), (0.1, "1e-3 .. 0.1"), (0.3, "0.1 .. 0.3"), (TWO_PI_3, "0.3 .. 2pi/3"), (np.pi, "2pi/3 .. pi")):
        if th < hi:
            return name
    return ">= pi"


CLASSES = ["< 1e-5 (shortcut)", "1e-5 .. 1e-3", "1e-3 .. 0.1", "0.1 .. 0.3", "0.3 .. 2pi/3", "2pi/3 .. pi", ">= pi"]


_REFS = None


def references():
    """(exp [n,3,4], target [n,3,4]) in float64 from tests/se3_ref.py at 50 digits, computed once per process and read-only: the true exponential exp(u^) T of every
    row, and what the update must return -- the same, except g2o's shortcut restated in mp on the rows below the band."""
    global _REFS
    if _REFS is None:
        from tests import se3_ref
        ex = np.stack([se3_ref.oplus(T, u) for T, u in zip(T_IN, U)])
        target = ex.copy()
        for i in np.flatnonzero(SHORTCUT):
            target[i] = se3_ref.oplus_shortcut(T_IN[i], U[i])
        ex.setflags(write=False)
        target.setflags(write=False)
        _REFS = (ex, target)
    return _REFS


def errors(T_out, T_ref):
    """Per row: (max |dR| [n], max |dt| / max(1, |t_ref|_inf) [n])."""
    T_out, T_ref = np.asarray(T_out).reshape(-1, 3, 4), np.asarray(T_ref).reshape(-1, 3, 4)
    dR = np.abs(T_out[:, :, :3] - T_ref[:, :, :3]).max((1, 2))
    dt = np.abs(T_out[:, :, 3] - T_ref[:, :, 3]).max(1) / np.maximum(1.0, np.abs(T_ref[:, :, 3]).max(1))
    return dR, dt


def oracle_oplus(T, u):
    """orc_pose_oplus (oracle/lm_oracle.c) over rows: [n,3,4]."""
    from oracle import geometry as G
    out = np.ascontiguousarray(np.asarray(T, np.float64).reshape(-1, 12).copy())
    u = np.ascontiguousarray(np.asarray(u, np.float64).reshape(-1, 6))
    for i in range(len(out)):
        G.lib().orc_pose_oplus(out[i], u[i])
    return out.reshape(-1, 3, 4)


def bound_rows():
    """The rows the bound is taken from: |omega| >= 0.3, where the oracle's closed forms are well conditioned."""
    return ANGLE >= 0.3


def report(title, dR, dt, rows=None):
    """Worst dR / dt per angle class, as printed lines."""
    rows = np.ones(len(ANGLE), bool) if rows is None else rows
    cls = np.array([angle_class(a) for a in ANGLE])
    lines = [title]
    for c in CLASSES:
        m = rows & (cls == c)
        if m.any():
            lines.append(f"  |omega| {c:18s} rows {int(m.sum()):4d}  dR {dR[m].max():.2e}  dt {dt[m].max():.2e}")
    return "\n".join(lines)
