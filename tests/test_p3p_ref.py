"""The mp P3P solution set (tests/p3p_ref.py) against exact constructions: a pose planted in mp numbers is among the solutions to 1e-40.  CPU only.

Rotations come from integer quaternions (rational entries, exact to the working precision), image points are the exact projections in mp; the planted depths are the
camera-frame norms of the three points.  Covered: generic rotations, half-turns about an axis, a face diagonal, a body diagonal and a generic axis, and the fronto-
parallel triangles whose problems have four all-positive solutions."""
import mpmath as mp
import numpy as np
import pytest

from tests import p3p_ref as PR

TOL = mp.mpf("1e-40")


def _rot(q):
    a, b, c, d = [mp.mpf(v) for v in q]
    n = a * a + b * b + c * c + d * d
    return mp.matrix([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (a * c + b * d)],
                      [2 * (a * d + b * c), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                      [2 * (b * d - a * c), 2 * (a * b + c * d), a * a - b * b - c * c + d * d]]) / n


def _problem(q, t, x):
    R = _rot(q)
    t = [mp.mpf(v) for v in t]
    x = [[mp.mpf(v) for v in p] for p in x]
    cam = [[sum(R[r, k] * p[k] for k in range(3)) + t[r] for r in range(3)] for p in x]
    y = [[c[0] / c[2], c[1] / c[2]] for c in cam]
    lam = [mp.sqrt(c[0] ** 2 + c[1] ** 2 + c[2] ** 2) for c in cam]
    return R, t, x, y, lam


X_GENERIC = [[17, -42, 5], [-63, 11, 29], [38, 57, -71], [4, -9, 12]]
SQ3 = "1.7320508075688772935274463415058723669428052538103806280558069794519330169088"
PLANTED = [
    ("generic", (3, 1, -2, 5), (12, -31, 640), X_GENERIC),
    ("generic, close", (7, -4, 1, 2), (-5, 9, 190), X_GENERIC),
    ("half-turn about x", (0, 1, 0, 0), (20, 10, 500), X_GENERIC),
    ("half-turn about z", (0, 0, 0, 1), (-30, 15, 900), X_GENERIC),
    ("half-turn about a face diagonal", (0, 1, 1, 0), (8, -14, 700), X_GENERIC),
    ("half-turn about a body diagonal", (0, 1, 1, -1), (8, -14, 700), X_GENERIC),
    ("half-turn about a generic axis", (0, 3, 1, 2), (-22, 40, 450), X_GENERIC),
]


@pytest.mark.parametrize("name,q,t,x", PLANTED, ids=[p[0] for p in PLANTED])
def test_planted_pose_is_recovered(name, q, t, x):
    with mp.workdps(PR.DPS):
        R, t, x, y, lam = _problem(q, t, x)
        s = PR.solve(x, y)
        assert s["posed"] and s["framed"] and s["margin"] > PR.EDGE
        best = min(s["sols"], key=lambda z: max(abs(z["lam"][k] - lam[k]) for k in range(3)))
        assert best["positive"]
        dl = max(abs(best["lam"][k] - lam[k]) / lam[k] for k in range(3))
        dR = max(abs(v) for v in (best["R"] - R))
        dt = max(abs(best["t"][k] - t[k]) for k in range(3)) / max(abs(v) for v in t)
        print(f"{name}: depths {mp.nstr(dl, 3)}, R {mp.nstr(dR, 3)}, t {mp.nstr(dt, 3)}; {len(s['sols'])} real solutions, margin {s['margin']:.2e}")
        assert dl < TOL and dR < TOL and dt < TOL
        if "half-turn" in name:
            assert abs(best["R"][0, 0] + best["R"][1, 1] + best["R"][2, 2] + 1) < TOL and PR.quat_branch(best["R"]) != {0}
        # the mirrored triple is a solution of the three equations too, and no pose of a camera in front of the points
        assert sum(1 for z in s["sols"] if not z["positive"] and all(v < 0 for v in z["lam"])) == sum(1 for z in s["sols"] if z["positive"])


@pytest.mark.parametrize("kind", ["equilateral", "isosceles"])
def test_fronto_parallel_triangle_off_axis_has_four_solutions(kind):
    with mp.workdps(PR.DPS):
        s3 = mp.mpf(SQ3)
        tri = {"equilateral": [[100, 0, 0], [-50, 50 * s3, 0], [-50, -50 * s3, 0]], "isosceles": [[0, 120, 0], [-60, -40, 0], [60, -40, 0]]}[kind]
        R, t, x, y, lam = _problem((1, 0, 0, 0), (30, -20, 400), tri + [[10, 20, 30]])
        s = PR.solve(x, y)
        pos = [z for z in s["sols"] if z["positive"]]
        assert s["posed"] and len(pos) == 4 and s["margin"] > PR.EDGE
        best = min(pos, key=lambda z: max(abs(z["lam"][k] - lam[k]) for k in range(3)))
        assert max(abs(v) for v in (best["R"] - R)) < TOL and max(abs(best["t"][k] - t[k]) for k in range(3)) / 400 < TOL
        # the fourth point tells them apart: the planted pose reprojects it exactly, the others do not
        errs = sorted(PR.fourth_point(z, x[3], y[3])[0] for z in pos)
        assert errs[0] < TOL and errs[1] > mp.mpf("1e-8")


def test_on_axis_equilateral_triangle_is_on_an_edge():
    """The symmetric view has repeated roots: nothing is claimed of it, and it says so."""
    x = np.array([[100.0, 0, 0], [-50.0, 50 * np.sqrt(3.0), 0], [-50.0, -50 * np.sqrt(3.0), 0]])
    cam = x + np.array([0, 0, 400.0])
    s = PR.solve(x, cam[:, :2] / cam[:, 2:3])
    assert s["margin"] < PR.EDGE


def test_what_cannot_be_posed_has_margin_zero():
    x = np.array([[1.0, 2, 3], [4.0, -5, 6], [-7.0, 8, 9]])
    y = np.array([[0.1, 0.2], [-0.1, 0.05], [0.02, -0.2]])
    for xs, ys in ((x[[0, 0, 2]], y), (x, y[[1, 1, 1]]), (x, np.array([[np.nan, 0.2], [-0.1, 0.05], [0.02, -0.2]]))):
        s = PR.solve(xs, ys)
        assert not s["posed"] and s["margin"] == 0.0 and s["sols"] == []
    s = PR.solve(np.array([x[0], x[1], 0.5 * (x[0] + x[1])]), y)          # exactly collinear: depths, no pose
    assert not s["framed"] and all(z["R"] is None for z in s["sols"])


def test_quaternion_branch_classes():
    d = lambda a, b, c: np.diag([a, b, c]).astype(float)      # noqa: E731
    assert PR.quat_branch(np.eye(3)) == {0}
    assert PR.quat_branch(d(1, -1, -1)) == {1} and PR.quat_branch(d(-1, 1, -1)) == {2} and PR.quat_branch(d(-1, -1, 1)) == {3}
    assert PR.quat_branch(d(0, 0, -1)) == {1, 2} and PR.quat_branch(d(0, -1, 0)) == {1, 3} and PR.quat_branch(d(-1, 0, 0)) == {2, 3}
    assert PR.quat_branch(d(-1 / 3, -1 / 3, -1 / 3)) == {1, 2, 3}
    assert PR.quat_branch(d(1, -1, -1) + 1e-8 * np.eye(3)) == {1} and PR.quat_branch(d(1, -1, -1) + 4e-8 * np.eye(3)) == {0}
