"""Designed four-point problems for the P3P / P4P minimal solver (csrc/pnp.hip: p3p_lambdatwist, p4p): INPUTS only, seeded, a few hundred.  A problem is four model
points xs [4][3] and four normalised image points ys [4][2]; points 0, 1, 2 go to P3P, point 3 picks among its candidates.  Every case carries a family and a name.

A  generic      the 400 problems of tests/golden/pnp_golden.npz (generic(); not part of cases())
B  half-turns   rotations by pi - delta about x, y, z, the six face diagonals, the four body diagonals and three axes with one dominant component (their off-diagonal
                entries of R are all non-zero), delta in DELTAS: trace(R) + 1 ~ delta^2 lies on both sides of the 1e-7 switch of the matrix-to-quaternion conversion
C  counts       fronto-parallel equilateral / isosceles triangles, camera on and off the axis, near and far; members of a seeded stream of generic problems that the
                reference answers with one candidate, with four and with three (their stream indices are recorded below: found once with
                make_p3p_edge_golden.py --search; none of the first 40000 members is answered with none)
D  degenerate   collinear and almost collinear triples, coincident model points, equal bearings, a NaN image coordinate in point 3
E  scale        coordinates times 2^-10, 2^10, 2^20; a unit object at depth 1e2 .. 1e4; bearings up to |y| = 5; depth about the object's size
F  fourth point the true candidate puts point 3 behind the camera; every candidate does; a grossly wrong fourth image point; close fourth-point errors; an exact tie

The recorded answers of the reference's own solver on cases() are tests/golden/p3p_edge_golden.npz (make_p3p_edge_golden.py)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DELTAS = (0.0, 1e-9, 1e-6, 2e-4, 4e-4, 1e-2)
AXES = {"x": (1, 0, 0), "y": (0, 1, 0), "z": (0, 0, 1),
        "xy": (1, 1, 0), "x-y": (1, -1, 0), "xz": (1, 0, 1), "x-z": (1, 0, -1), "yz": (0, 1, 1), "y-z": (0, 1, -1),
        "xyz": (1, 1, 1), "xy-z": (1, 1, -1), "x-yz": (1, -1, 1), "-xyz": (-1, 1, 1),
        "X": (3, 1, 2), "Y": (1, 3, -2), "Z": (-2, 1, 3)}
# indices into stream() of problems the reference's p3p answers with 1, 4 and 3 candidates (of the first 40000 members 79 give 1, 823 give 4, 12 give 3, none 0)
COUNT1_KEYS = (1023, 1758, 1918, 2237, 2255, 2346, 2757, 2778)
COUNT4_KEYS = (51, 56, 57, 83, 291, 313, 348, 354)
COUNT3_KEYS = (3439, 4527, 8822, 9330, 10809, 13512)


def generic():
    g = np.load(os.path.join(HERE, "pnp_golden.npz"))
    return g["xs"], g["ys"]


def half_turn(axis, delta):
    """Rotation by pi - delta about axis: cos = -cos(delta), sin = sin(delta), so delta survives below 1e-8."""
    n = np.asarray(axis, np.float64)
    n = n / np.linalg.norm(n)
    c, s = -np.cos(delta), np.sin(delta)
    K = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    return c * np.eye(3) + (1 - c) * np.outer(n, n) + s * K


def random_rotation(rng):
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 0] *= -1
    return Q


def project(R, t, x):
    X = x @ R.T + t
    return X[:, :2] / X[:, 2:3]


def stream(k):
    """Member k of the seeded stream of generic problems (the generator family of make_pnp_golden.py); returns xs, ys, R, t."""
    rng = np.random.Generator(np.random.PCG64([2718, k]))
    x = rng.uniform(-100, 100, (4, 3))
    R = random_rotation(rng)
    t = np.array([rng.uniform(-80, 80), rng.uniform(-80, 80), rng.uniform(300, 1500)])
    return x, project(R, t, x), R, t


def cases():
    rng = np.random.Generator(np.random.PCG64(31415))
    out = []

    def add(family, name, x, y):
        out.append({"family": family, "name": name, "xs": np.ascontiguousarray(x, np.float64).copy(), "ys": np.ascontiguousarray(y, np.float64).copy()})

    # ---- B
    for an, axis in AXES.items():
        for delta in DELTAS:
            for rep, depth in enumerate((400.0, 1200.0)):
                x = rng.uniform(-100, 100, (4, 3))
                R = half_turn(axis, delta)
                t = np.array([rng.uniform(-80, 80), rng.uniform(-80, 80), depth])
                add("B", f"half-turn about {an}, delta {delta:g}, depth {depth:g}", x, project(R, t, x))
    # ---- C
    tri = {"equilateral": np.array([[100.0, 0, 0], [-50.0, 50 * np.sqrt(3.0), 0], [-50.0, -50 * np.sqrt(3.0), 0]]),
           "isosceles": np.array([[0.0, 120, 0], [-60.0, -40, 0], [60.0, -40, 0]])}
    for tn, T3 in tri.items():
        for cn, off in (("on axis", (0.0, 0.0)), ("off axis", (30.0, -20.0)), ("far off axis", (140.0, 90.0))):
            for depth in (400.0, 60.0):
                x = np.vstack([T3, [10.0, 20.0, 30.0]])
                t = np.array([off[0], off[1], depth])
                add("C", f"{tn} fronto-parallel triangle, camera {cn}, depth {depth:g}", x, project(np.eye(3), t, x))
    for k in COUNT1_KEYS:
        x, y, _, _ = stream(k)
        add("C", f"stream {k}: one candidate", x, y)
    for k in COUNT4_KEYS:
        x, y, _, _ = stream(k)
        add("C", f"stream {k}: four candidates", x, y)
    for k in COUNT3_KEYS:
        x, y, _, _ = stream(k)
        add("C", f"stream {k}: three candidates", x, y)
    # ---- D
    for rep in range(3):
        x, y, R, t = stream(9000 + rep)
        x[2] = (0.5, 0.25, 2.0)[rep] * x[0] + (0.5, 0.75, -1.0)[rep] * x[1]
        add("D", f"collinear triple {rep}, image consistent", x, project(R, t, x))
        add("D", f"collinear triple {rep}, image of a generic triple", x, y)
    for rep in range(2):
        x, y, R, t = stream(9010 + rep)
        x[2] = 0.5 * (x[0] + x[1]) + 2.5e-10 * np.linalg.norm(x[0] - x[1]) * np.array([0.6, -0.8, 0.0])
        add("D", f"triple within 1e-9 of collinear {rep} (2.5e-10 of the side off the line)", x, project(R, t, x))
    for rep, (i, j) in enumerate(((0, 1), (0, 2), (1, 2))):
        x, y, R, t = stream(9020 + rep)
        x[j] = x[i]
        add("D", f"model points {i} and {j} coincide, image consistent", x, project(R, t, x))
        add("D", f"model points {i} and {j} coincide, bearings distinct", x, y)
    for rep, (i, j) in enumerate(((0, 1), (1, 2))):
        x, y, R, t = stream(9030 + rep)
        y[j] = y[i]
        add("D", f"bearings {i} and {j} equal, model points distinct", x, y)
    x, y, R, t = stream(9040)
    y[1] = y[0]
    y[2] = y[0]
    add("D", "three equal bearings", x, y)
    for rep in range(2):
        x, y, R, t = stream(9050 + rep)
        y[3, rep] = np.nan
        add("D", f"NaN image coordinate {rep} in point 3", x, y)
    # ---- E
    for e in (-10, 10, 20):
        for rep in range(3):
            x, y, R, t = stream(9100 + rep)
            xs = x * 2.0 ** e
            add("E", f"coordinates and translation times 2^{e}, stream {9100 + rep}", xs, project(R, t * 2.0 ** e, xs))
    corner = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [-0.5, -0.5, -0.5]])          # a well-spread object: the depth alone sets the conditioning
    for depth in (1e2, 1e3, 1e4):
        for rep in range(3):
            x = corner @ random_rotation(rng).T
            R = random_rotation(rng)
            t = np.array([rng.uniform(-0.05, 0.05) * depth, rng.uniform(-0.05, 0.05) * depth, depth])
            add("E", f"object of size 1 at depth {depth:g} ({rep})", x, project(R, t, x))
    for rep in range(3):
        x = rng.uniform(-100, 100, (4, 3))
        R = random_rotation(rng)
        t = np.array([(-1) ** rep * 1200.0, 900.0 - 600.0 * rep, 300.0])
        add("E", f"wide bearings ({rep})", x, project(R, t, x))
    for rep in range(3):
        x = rng.uniform(-100, 100, (4, 3))
        R = random_rotation(rng)
        t = np.array([rng.uniform(-20, 20), rng.uniform(-20, 20), 260.0 - 30.0 * rep])
        add("E", f"depth about the object's size ({rep})", x, project(R, t, x))
    # ---- F
    for rep in range(4):
        x, y, R, t = stream(9200 + rep)
        x[3] = R.T @ (np.array([40.0 + 10 * rep, -30.0, -0.5 * t[2]]) - t)          # z of point 3 under the true pose: -t_z / 2
        add("F", f"true pose puts point 3 behind the camera ({rep})", x, project(R, t, x))
    for n, k in enumerate(COUNT1_KEYS[:4]):
        x, y, R, t = stream(k)
        x[3] = R.T @ (np.array([25.0, 35.0 - 10 * n, -2.0 * t[2]]) - t)
        add("F", f"stream {k}: the only candidate puts point 3 behind the camera", x, project(R, t, x))
    for rep in range(3):
        x, y, R, t = stream(9210 + rep)
        y[3] += (3.0, -2.0)
        add("F", f"grossly wrong fourth image point ({rep})", x, y)
    for rep in range(3):
        x, y, R, t = stream(9220 + rep)
        x[3] = x[0] + 1e-4 * (x[1] - x[0])
        y = project(R, t, x)
        y[3] += (1e-3, -5e-4)
        add("F", f"close fourth-point errors ({rep})", x, y)
    for rep in range(3):
        x, y, R, t = stream(9230 + rep)
        x[3] = x[0]
        y[3] = (1000.0, -750.0)
        add("F", f"exact tie of the fourth-point errors ({rep})", x, y)
    return out


def arrays(table=None):
    table = cases() if table is None else table
    return np.stack([c["xs"] for c in table]), np.stack([c["ys"] for c in table])
