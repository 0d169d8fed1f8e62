"""The designed table for the refinement half of the PnP kernel (tests/test_pnp_refine_ref.py on the CPU, tests/test_gpu_pnp_refine.py on the device), the packing
of its rows into the arguments of suo_debug_pnp_refine / orc_pnp_refine_debug, the mp reference of every row (tests/pnp_refine_ref.py, computed once per process)
and the error measures both tests share.  Inputs regenerate from seeds; every row says why it is there.

A  workload-shaped: n keypoints of an object the size and depth suo_slam_amd/synthetic.py: make_frame draws, noise on ys, outliers, started at orc_p4p of four
   noisy inliers (SEQUENCE).
B  lane stride: n around the multiples of 64 and at the limit, explicit selections that sit on one slot, one lane, all but one point, four points, none (PASS).
C  far starts: rejected steps, a shrinking radius, the iteration caps, trial poses with selected points behind the camera, a start whose cost is not finite (PASS).
D  the second pass: seeds found by search whose reselection gives (m, deltas) far below, just below, on and far above `deltas < 0.05 m` (SEQUENCE).
E  rule edges: poses whose rotation is exact in float64, err == thr^2 bit for bit and its two neighbours, z = 0, -0.0, -tiny, +tiny (SEQUENCE).
F  weak systems: four or five selected points on a line, or on a fronto-parallel plane (PASS)."""
from __future__ import annotations

import functools

import numpy as np

from oracle import geometry as G
from tests import pnp_refine_ref as RR

THR = 1e-3
SEQUENCE, PASS = 0, 1
OUT_D = 88


def _quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def _small_quat(axis, angle):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])


def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def make_object(seed, n, sigma, outliers=0.0, X=None):
    """Points of a make_frame-sized object (half extents 40-100 mm, depth 600-1200 mm), their noisy normalised projections, the true pose and the inlier mask."""
    rng = np.random.default_rng(seed)
    if X is None:
        X = rng.uniform(-1, 1, (n, 3)) * rng.uniform(40, 100, 3)
    q = _quat(rng)
    z = rng.uniform(600, 1200)
    t = np.array([rng.uniform(-0.25, 0.25) * z, rng.uniform(-0.18, 0.18) * z, z])
    pc = X @ G.quat_to_rot(q).T + t
    y = pc[:, :2] / pc[:, 2:] + rng.normal(0, 1, (n, 2)) * sigma
    inl = np.ones(n, bool)
    k = int(round(outliers * n))
    if k:
        bad = 4 + rng.permutation(n - 4)[:k]                    # (the first four points stay inliers: the start is p4p of them)
        y[bad] += rng.uniform(5, 50, (k, 2)) * THR * rng.choice([-1, 1], (k, 2))
        inl[bad] = False
    return np.ascontiguousarray(X), np.ascontiguousarray(y), q, t, inl


def p4p_start(X, y, idx=(0, 1, 2, 3)):
    q, t = np.zeros(4), np.zeros(3)
    G.lib().orc_p4p(X, y, np.asarray(idx, np.int32), q, t)
    return q, t


def _row(cls, why, X, y, q0, t0, mode=SEQUENCE, sel=None, max_iter=0, tol=0.0, idx=None):
    return {"cls": cls, "why": why, "xs": np.ascontiguousarray(X, np.float64), "ys": np.ascontiguousarray(y, np.float64), "q0": np.asarray(q0, np.float64),
            "t0": np.asarray(t0, np.float64), "mode": mode, "sel": None if sel is None else np.asarray(sel, np.int32), "max_iter": max_iter, "tol": tol,
            "idx": idx}


def _class_a():
    rows = []
    for n in (4, 5, 8, 22, 41):
        for si, (sname, sigma) in enumerate((("0", 0.0), ("thr/10", THR / 10), ("thr/3", THR / 3))):
            for oi, out in enumerate((0.0, 0.15, 0.3)):
                if out and n < 8:
                    continue
                X, y, _, _, _ = make_object(1000 + 100 * n + 10 * si + oi, n, sigma, out)
                q0, t0 = p4p_start(X, y)
                rows.append(_row("A", f"n = {n}, noise {sname}, {int(100 * out)} % outliers, start p4p(0..3)", X, y, q0, t0, idx=(0, 1, 2, 3)))
    return rows


def _near_start(seed, q, t, angle=1e-3, shift=5e-3):
    rng = np.random.default_rng(seed)
    return _qmul(_small_quat(rng.normal(size=3), angle), q), t * (1 + shift * rng.uniform(-1, 1, 3))


def _class_b():
    rows = []
    for n in (63, 64, 65, 127, 128, 129, 1023, 1024):
        X, y, q, t, _ = make_object(2000 + n, n, THR / 10)
        q0, t0 = _near_start(n, q, t)
        last = (n - 1) // 64
        i = np.arange(n)
        four = np.zeros(n, bool)
        four[[0, min(64 + 17, n - 2), (n - 1) // 2, n - 1]] = True                 # four different (lane, slot) positions
        sels = (("all points", np.ones(n, bool)), (f"only slot j = {last}", i // 64 == last), ("only lane 63's points", i % 64 == 63),
                ("all but point 1", i != 1), ("four points in four (lane, slot) positions", four), ("no point", np.zeros(n, bool)))
        for name, s in sels:
            big = n >= 1023 and s.sum() > 64
            its = (1 if n == 1024 else 0) if big else 5            # (an mp system of 1024 points costs a second: one LM step at 1024, the system alone at 1023)
            rows.append(_row("B", f"n = {n}, {name} ({int(s.sum())} selected), {its} iterations", X, y, q0, t0, PASS, s, its, 1e-6))
    return rows


def _class_c():
    rows = []
    k = 0
    for n in (8, 22, 41):
        for angle, frac, its in ((0.05, 0.1, 5), (0.2, 0.3, 5), (0.5, 0.5, 50), (0.5, -0.45, 50)):
            X, y, q, t, inl = make_object(3000 + k, n, THR / 10)
            rng = np.random.default_rng(3500 + k)
            q0 = _qmul(_small_quat(rng.normal(size=3), angle), q)
            t0 = t * (1 + frac * np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), 1.0]))
            rows.append(_row("C", f"n = {n}, start {angle} rad and {int(100 * frac)} % of the depth away, cap {its}", X, y, q0, t0, PASS, inl, its, 1e-6))
            k += 1
    # beyond the range above nothing is rejected (0.5 rad off, Gauss-Newton still converges in four steps): starts 2-3 rad off, where steps are rejected, the radius
    # shrinks and both caps are hit
    for n, seed, angle, frac in ((8, 6, 3.0, 0.5), (8, 7, 3.0, -0.45), (8, 8, 3.0, -0.8), (12, 12, 2.0, 0.5), (12, 13, 2.0, -0.45), (12, 15, 3.0, 0.5)):
        X, y, q, t, inl = make_object(3000 + seed, n, THR / 10)
        rng = np.random.default_rng(3501 + seed)
        q0 = _qmul(_small_quat(rng.normal(size=3), angle), q)
        t0 = t * (1 + frac * np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), 1.0]))
        for its in (5, 50):
            rows.append(_row("C", f"n = {n}, start {angle} rad and {int(100 * frac)} % of the depth away, cap {its}", X, y, q0, t0, PASS, inl, its, 1e-6))
    # trial poses behind the camera: the object a few of its own lengths from the camera plane, started half a radian off
    for s in range(4):
        X, y, q, t, inl = make_object(3900 + s, 12, THR / 10)
        t = np.array([10.0, -5.0, 160.0 + 20 * s])
        pc = X @ G.quat_to_rot(q).T + t
        y = pc[:, :2] / pc[:, 2:]
        q0 = _qmul(_small_quat([1, 2, 0.5], 0.5), q)
        rows.append(_row("C", f"object {int(t[2])} mm from the camera plane (points from z = {pc[:, 2].min():.0f}), start 0.5 rad off, cap 50", X, y, q0, t, PASS, inl,
                         50, 1e-6))
    # a start whose cost is not finite: a selected point ON the camera plane (identity rotation, z = X2 + t2 = 0 exactly)
    X = np.array([[10.0, 20, -500], [30, -20, 100], [-40, 10, 50], [20, 30, -30], [-10, -30, 80], [5, 5, 0]])
    t = np.array([0.0, 0, 500])
    y = np.array([[0.1, 0.1]] * 6)
    rows.append(_row("C", "a selected point with z = 0 at the start: the cost is not finite, the start comes back", X, y, [1, 0, 0, 0], t, PASS, np.ones(6), 5, 1e-6))
    return rows


# (n, seed, noise / thr, (m, deltas) of the reselection, why): seeds found by a search over make_object(4000 + seed, ...); tests/test_pnp_refine_ref.py holds the mp
# reference of every row to the (m, deltas) written here
CLASS_D = ((41, 10, 0.3, (41, 0), "far below the rule: skipped"), (41, 28, 0.3, (41, 2), "skipped: 2 < 2.05"), (41, 43, 0.3, (40, 2), "runs: 2 is not < 2.0"),
           (22, 280, 0.45, (20, 1), "runs: 1 is not < 1.0"), (41, 0, 0.3, (40, 15), "far above the rule: runs"))


def class_d_object(n, seed, noise):
    X, y, _, _, _ = make_object(4000 + seed, n, noise * THR)
    return X, y


def _class_d():
    rows = []
    for n, seed, noise, md, why in CLASS_D:
        X, y = class_d_object(n, seed, noise)
        q0, t0 = p4p_start(X, y)
        rows.append(_row("D", f"n = {n}, seed {seed}: reselection (m, deltas) = {md}, {why}", X, y, q0, t0, idx=(0, 1, 2, 3)))
    return rows


def _class_e():
    rows = []
    up, dn = float(np.nextafter(THR, 1.0)), float(np.nextafter(THR, 0.0))
    good = make_object(5000, 8, THR / 10)[0] / 100.0 + np.array([0, 0, 3.0])            # eight points 2-4 units in front of an identity camera
    rng = np.random.default_rng(5001)
    gy = good[:, :2] / good[:, 2:] + rng.normal(0, THR / 10, (8, 2))
    edge_y = np.array([[-THR, 0.0], [-up, 0.0], [-dn, 0.0], [0.0, THR], [0.0, up], [0.0, dn]])
    # identity; a half turn about z, q = (0, 0, 0, 1): R = diag(-1, -1, 1); a quarter turn about z as the non-unit q = (1, 0, 0, 1): R = 2 [[0, -1, 0], [1, 0, 0],
    # [0, 0, 1]] exactly (getRotationMatrix does not normalise), with t = 0 the projection is that of the rotation
    for name, q, back in (("identity", [1.0, 0, 0, 0], np.eye(3)), ("half turn (0,0,0,1)", [0.0, 0, 0, 1], np.diag([-1.0, -1, 1])),
                          ("quarter turn, q = (1,0,0,1) not normalised", [1.0, 0, 0, 1], np.array([[0, 0.5, 0], [-0.5, 0, 0], [0, 0, 0.5]]))):
        cam = np.concatenate([good, np.tile([0.0, 0, 1], (6, 1))])                      # camera-frame points; X = R^-1 cam is exact (signs, halves)
        X = cam @ back.T
        rows.append(_row("E", f"{name}: err == thr^2 bit for bit and its two neighbours, on either axis", X, np.concatenate([gy, edge_y]), q, [0.0, 0, 0]))
    tiny = 1e-300
    zs = np.array([[1.0, 1, 0], [-1.0, -1, -0.0], [1.0, 2, -tiny], [1.0, 2, tiny], [-3.0, 1, -2.0]])
    zy = np.array([[0.5, 0.5], [0.5, 0.5], [0.5, 0.5], [0.5, 0.5], [1.5, -0.5]])
    rows.append(_row("E", "z = 0 with x, y != 0; z = -0.0 (t2 = -0.0); z = -1e-300; z = +1e-300 off the axis; behind with err = 0", np.concatenate([good, zs]),
                     np.concatenate([gy, zy]), [1.0, 0, 0, 0], [0.0, 0, -0.0]))
    # (the point ON the axis at z = +1e-300 is an inlier by both rules with 1 / z^2 = 1e600 in its Jacobian: it sits in the row whose cost is not finite anyway)
    nan = np.array([[0.0, 1, 0], [1.0, 0, 0], [0.0, 0, 0], [0.0, 0, tiny]])
    rows.append(_row("E", "z = 0 with x or y = 0: err is NaN, neither < nor > thr^2: selected, the cost is not finite; z = +1e-300 on the axis: err = 0",
                     np.concatenate([good, nan]), np.concatenate([gy, [[0.5, 0.5]] * 3, [[0.0, 0.0]]]), [1.0, 0, 0, 0], [0.0, 0, 0]))
    return rows


def _class_f():
    rows = []
    # five seeds of each kind: a weak system amplifies rounding by its condition, which differs by orders of magnitude from row to row, and the trajectory bound of
    # this class is a maximum over its rows (with one or two rows per kind the device run sat 1.5 x above 4 x the oracle's worst: dt 8.5e-15 against 5.5e-15)
    kinds = (("collinear", 4), ("coplanar, fronto-parallel", 4), ("coplanar, fronto-parallel", 5), ("collinear", 5))
    for k, (name, n_sel) in enumerate(kinds[j % 4] for j in range(20)):
        rng = np.random.default_rng(6000 + k)
        n = 12
        X = rng.uniform(-1, 1, (n, 3)) * rng.uniform(40, 100, 3)
        X_, y, q, t, _ = make_object(6100 + k, n, THR / 10, X=X)
        Rt = G.quat_to_rot(q).T
        if name == "collinear":
            line = rng.normal(size=3)
            X[:n_sel] = np.outer(np.linspace(-80, 80, n_sel), line / np.linalg.norm(line))
        else:
            cam = np.concatenate([rng.uniform(-80, 80, (n_sel, 2)), np.full((n_sel, 1), 30.0)], 1)       # one plane z = const in the camera frame
            X[:n_sel] = cam @ Rt.T                                                                         # X = R^T cam (up to rounding)
        X_, y, q, t, _ = make_object(6100 + k, n, THR / 10, X=X)
        q0, t0 = _near_start(6200 + k, q, t)
        sel = np.arange(n) < n_sel
        rows.append(_row("F", f"{n_sel} selected points {name}, seed {k // 4}", X, y, q0, t0, PASS, sel, 5, 1e-6))
    return rows


@functools.lru_cache(maxsize=None)
def table():
    return tuple(_class_a() + _class_b() + _class_c() + _class_d() + _class_e() + _class_f())


def classes():
    return np.array([r["cls"] for r in table()])


def pack(rows, idx_start=False):
    """The arguments of suo_debug_pnp_refine / orc_pnp_refine_debug for these rows; idx_start: rows that carry four indices start from p4p of them."""
    n = np.array([len(r["xs"]) for r in rows], np.int32)
    xs = np.ascontiguousarray(np.concatenate([r["xs"] for r in rows]))
    ys = np.ascontiguousarray(np.concatenate([r["ys"] for r in rows]))
    mode = np.array([r["mode"] for r in rows], np.int32)
    qt = np.ascontiguousarray(np.stack([np.concatenate([r["q0"], r["t0"]]) for r in rows]))
    idx = np.full((len(rows), 4), -1, np.int32)
    if idx_start:
        for k, r in enumerate(rows):
            if r["idx"] is not None:
                idx[k] = r["idx"]
    sel = np.ascontiguousarray(np.concatenate([np.zeros(len(r["xs"]), np.int32) if r["sel"] is None else r["sel"].astype(np.int32) for r in rows]))
    mi = np.array([r["max_iter"] for r in rows], np.int32)
    tol = np.array([r["tol"] for r in rows], np.float64)
    return {"n": n, "xs": xs, "ys": ys, "mode": mode, "qt": qt, "idx": idx, "sel": sel, "max_iter": mi, "tol": tol}


def unpack(rows, out_d, out_i, sel0, sel1):
    """Per row: dict of what the entry returned."""
    res, p = [], 0
    for k, r in enumerate(rows):
        n = len(r["xs"])
        D, I = out_d[k], out_i[k]
        res.append({"q0": D[0:4].copy(), "t0": D[4:7].copy(), "H": D[7:43].reshape(6, 6).copy(), "g": D[43:49].copy(), "cost": float(D[49]),
                    "qm": D[50:54].copy(), "tm": D[54:57].copy(), "q": D[57:61].copy(), "t": D[61:64].copy(), "Tm": D[64:76].reshape(3, 4).copy(),
                    "T": D[76:88].reshape(3, 4).copy(), "count": int(I[0]), "m0": int(I[1]), "m": int(I[2]), "deltas": int(I[3]), "second": int(I[4]),
                    "sel0": sel0[p:p + n].copy(), "sel1": sel1[p:p + n].copy()})
        p += n
    return res


def run_oracle(rows, idx_start=False):
    a = pack(rows, idx_start)
    out_d, out_i = np.full((len(rows), OUT_D), np.nan), np.full((len(rows), 8), -7, np.int32)
    s0, s1 = np.full(len(a["sel"]), -7, np.int32), np.full(len(a["sel"]), -7, np.int32)
    rc = G.lib().orc_pnp_refine_debug(len(rows), a["n"], a["xs"], a["ys"], THR, a["mode"], a["qt"], a["idx"], a["sel"], a["max_iter"], a["tol"], out_d, out_i, s0, s1)
    assert rc == 0
    return unpack(rows, out_d, out_i, s0, s1)


# ---------------------------------------------------------------------------------------------------------------- the mp reference of a row
def reference_row(r):
    P = RR.Problem(r["xs"], r["ys"], THR)
    q0, t0 = RR.mpv(r["q0"]), RR.mpv(r["t0"])
    count, near_c = RR.count_rule(P, q0, t0)
    ref = {"P": P, "count": count}
    if r["mode"] == SEQUENCE:
        S = RR.sequence(P, q0, t0)
        ref.update(sel0=S["sel0"], sel1=S["sel1"], m0=S["m0"], m=S["m"], deltas=S["deltas"], second=int(S["second"]), qm=S["first"]["q"], tm=S["first"]["t"],
                   q=S["q"], t=S["t"], margins=S["margins"], stops=(S["first"]["stop"], S["last"]["stop"] if S["last"] else None),
                   rejected=S["first"]["rejected"] + (S["last"]["rejected"] if S["last"] else 0), behind=0, near=near_c or S["near_rules"] or RR.is_near(S["margins"]))
        ref["system"] = S["first"].get("system0") or RR.system(P, q0, t0, S["sel0"])
    else:
        sel = [int(v != 0) for v in r["sel"]]
        L = RR.lm(P, q0, t0, sel, r["max_iter"], r["tol"])
        ref.update(sel0=sel, sel1=[0] * P.n, m0=sum(sel), m=0, deltas=0, second=0, qm=L["q"], tm=L["t"], q=L["q"], t=L["t"], margins=L["margins"],
                   stops=(L["stop"], None), rejected=L["rejected"], behind=L["behind"], near=near_c or RR.is_near(L["margins"]))
        ref["system"] = L.get("system0") or RR.system(P, q0, t0, sel)
    return ref


@functools.lru_cache(maxsize=None)
def references():
    """The mp reference of every row of the table, computed once per process."""
    return tuple(reference_row(r) for r in table())


@functools.lru_cache(maxsize=None)
def minimisers():
    """Per class-A row: the mp minimiser of the cost over the reference's final selection, started at the reference's final pose (None for the other classes)."""
    out = []
    for r, ref in zip(table(), references()):
        sel = ref["sel1"] if ref["second"] else ref["sel0"]
        out.append(RR.minimiser(ref["P"], ref["q"], ref["t"], sel) if r["cls"] == "A" and sum(sel) >= 3 else None)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- measures
def system_errors(got, ref):
    """(eH, eg, ec, bound) of assertion (a), in units of 2^-53: H[a][c] relative to sqrt(H_aa H_cc), g[a] to sqrt(H_aa sum (|pi| + |y|)^2), cost to
    sum |r| (|pi| + |y|); bound = n_sel + 16.  None where the reference system is not finite or the selection is empty."""
    import mpmath as mp
    S = ref["system"]
    if S is None or S["n_sel"] == 0:
        return None
    with mp.workdps(RR.DPS):
        u = mp.mpf(2) ** -53
        eH = max(abs(RR.mpf(got["H"][a, c]) - S["H"][a][c]) / mp.sqrt(S["H"][a][a] * S["H"][c][c]) for a in range(6) for c in range(6))
        eg = max(abs(RR.mpf(got["g"][a]) - S["g"][a]) / mp.sqrt(S["H"][a][a] * S["sg2"]) for a in range(6))
        ec = abs(RR.mpf(got["cost"]) - S["cost"]) / S["sc"] if S["sc"] > 0 else mp.mpf(0)
        return float(eH / u), float(eg / u), float(ec / u), float(S["n_sel"] + 16)


def cost_slack(ref_system):
    """Twice the cost bound of (a), as an absolute cost."""
    import mpmath as mp
    with mp.workdps(RR.DPS):
        return 2 * (ref_system["n_sel"] + 16) * mp.mpf(2) ** -53 * ref_system["sc"]


def pose_errors(q, t, q_ref, t_ref):
    """(dR, dt / max(1, |t_ref|_inf)) of a float64 pose against an mp one."""
    dR, dt = RR.pose_distance(q, t, q_ref, t_ref)
    return dR, dt / max(1.0, max(abs(float(v)) for v in t_ref))


def measure(res):
    """Everything the assertions (a)-(e) need of one run (oracle or kernel) over the table, per row, against references():
    sys [rows, 4] = (eH, eg, ec, bound) in units of 2^-53 (NaN: no finite system); rules [rows] = every flag, count, m, deltas and the second-pass flag equal the mp
    rules; descent [rows, 2] = (cost(mid; S0) - cost(start; S0)) / slack and (cost(final; S1) - cost(mid; S1)) / slack in mp at the returned bits over the returned
    selections, slack = twice the cost bound of (a) (NaN: not applicable); same_start [rows] = the poses returned are the start bit for bit (rows with an empty
    selection or a start cost that is not finite; True elsewhere); mid, fin [rows, 2] = (dR, dt / max(1, |t|)) of the pose after the first pass and of the final
    pose against the mp trajectory."""
    import mpmath as mp
    rows, refs = table(), references()
    n = len(rows)
    out = {"sys": np.full((n, 4), np.nan), "rules": np.zeros(n, bool), "descent": np.full((n, 2), np.nan), "same_start": np.ones(n, bool),
           "mid": np.zeros((n, 2)), "fin": np.zeros((n, 2))}
    u = 2.0 ** -53
    for k, (r, ref, got) in enumerate(zip(rows, refs, res)):
        P = ref["P"]
        e = system_errors(got, ref)
        if e is not None:
            out["sys"][k] = e
        out["rules"][k] = (list(got["sel0"]) == list(ref["sel0"]) and list(got["sel1"]) == list(ref["sel1"]) and got["count"] == sum(ref["count"])
                           and got["m0"] == ref["m0"] and got["m"] == ref["m"] and got["deltas"] == ref["deltas"] and got["second"] == ref["second"])
        q0, t0, qm, tm, qf, tf = (RR.mpv(got[key]) for key in ("q0", "t0", "qm", "tm", "q", "t"))
        c0, sc0 = RR.cost_and_scale(P, q0, t0, got["sel0"])
        if got["m0"] == 0 or c0 == mp.inf:
            out["same_start"][k] = (np.array_equal(got["qm"], got["q0"]) and np.array_equal(got["tm"], got["t0"]) and
                                    (r["mode"] == SEQUENCE and got["second"] == 1 or (np.array_equal(got["q"], got["q0"]) and np.array_equal(got["t"], got["t0"]))))
        else:
            with mp.workdps(RR.DPS):
                slack = 2 * (got["m0"] + 16) * u * sc0
                out["descent"][k, 0] = float((RR.cost(P, qm, tm, got["sel0"]) - c0) / slack) if slack > 0 else 0.0
        if got["second"]:
            c1, sc1 = RR.cost_and_scale(P, qm, tm, got["sel1"])
            if c1 != mp.inf and got["m"] > 0:
                with mp.workdps(RR.DPS):
                    slack = 2 * (got["m"] + 16) * u * sc1
                    out["descent"][k, 1] = float((RR.cost(P, qf, tf, got["sel1"]) - c1) / slack) if slack > 0 else 0.0
        out["mid"][k] = pose_errors(got["qm"], got["tm"], ref["qm"], ref["tm"])
        out["fin"][k] = pose_errors(got["q"], got["t"], ref["q"], ref["t"])
    return out


def class_bounds(oracle_measure, factor=4.0):
    """Per class: factor x the worst (dR, dt) of the oracle from the mp trajectory over the class's rows that are not near (mid and final poses)."""
    cls, near = classes(), np.array([ref["near"] for ref in references()])
    out = {}
    for c in sorted(set(cls)):
        m = (cls == c) & ~near
        both = np.concatenate([oracle_measure["mid"][m], oracle_measure["fin"][m]])
        out[c] = factor * both.max(0)
    return out


def optimum_errors(res):
    """Assertion (e), per class-A row whose mp run stopped on a tolerance: (dR, dt) of the returned final pose from minimisers(), the same of the mp run's own final
    pose, and the largest gradient entry in mp at the returned bits over the final selection relative to the tolerance of the pass that ended the run."""
    import mpmath as mp
    out = {}
    for k, (r, ref, mn, got) in enumerate(zip(table(), references(), minimisers(), res)):
        if mn is None or "cap" in ref["stops"]:
            continue
        sel = ref["sel1"] if ref["second"] else ref["sel0"]
        S = RR.system(ref["P"], RR.mpv(got["q"]), RR.mpv(got["t"]), sel)
        with mp.workdps(RR.DPS):
            g = float(max(abs(v) for v in S["g"]) / (mp.mpf("1e-8") if ref["second"] else mp.mpf("1e-6")))
        out[k] = (pose_errors(got["q"], got["t"], mn["q"], mn["t"]), pose_errors([float(v) for v in ref["q"]], [float(v) for v in ref["t"]], mn["q"], mn["t"]), g)
    return out
