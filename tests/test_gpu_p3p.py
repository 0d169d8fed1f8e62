"""The P3P / P4P minimal solver every lane of pnp_batch_kernel runs per hypothesis (csrc/pnp.hip: p3p_lambdatwist with cubick, eigwithknown0, root2real,
gauss_newton_refineL, inv3; rot_to_quat; the fourth-point choice of p4p) reached through suo_debug_p3p, over the designed table of tests/golden/p3p_edge_cases.py
(families B .. F) and the 400 generic problems (A): ONE launch, one thread per problem.  Two yardsticks (tests/p3p_cases.py): the recorded answers of the reference's
own solver, and the mp solution set of tests/p3p_ref.py.  tests/test_p3p_edge_cases.py shows without a GPU what the table reaches and what may be left out.

(a) count       valid equals the recorded count on every case that is not on an edge (edge margin < 1e-9); on an edge 0 <= valid <= 4; zero beyond valid
(b) candidates  in the reference's order, every explained candidate against its mp solution: err_dev <= 8 err_ref + 64 2^-53, with
                err = max(|R - R_mp|_max, |t - t_mp|_inf / max(|t_mp|_inf, |x|_max)) and err_ref the recorded candidate's own error against the same solution.  Of an
                unexplained candidate (the reference's not-quite-rotations) only the finiteness pattern is compared.
(c) chosen      qt is finite; identity with status 1 exactly where the reference returns identity; the same candidate as the reference chose wherever the choice is
                decided (one admissible mp solution, or the two best fourth-point errors more than 1e-6 apart) and on the exact-tie cases (the first wins); the
                pose under the error rule of (b) against the recorded pose's error
(d) generic     all 400: p4p pose at 1e-12 against p4p_T (what test_gpu_geometry checks for 100 chosen poses), and the same bound for every candidate against
                p3p_R, p3p_t (t relative to |x|_max)
(e) same code   a sample of B, C and F as four-point problems through lambdatwist.pnp_batch(refine=False), at both launch widths: equal to qt bit for bit wherever
                best_inliers > 0
(f) refusals    n = 0, n < 0, a NULL pointer: SUO_ERR_ARG, outputs untouched

Which case catches which slip in rot_to_quat's non-trace branches (tallies: tests/test_p3p_edge_cases.py): the chosen pose of the half-turns about the axes with one
dominant component -- X (3, 1, 2) branch 1, Y (1, 3, -2) branch 2, Z (-2, 1, 3) branch 3 -- at delta 1e-6, 2e-4 has every R[i] + R[j] above 0.1 and every R[i] - R[j]
above 1e-7 in size, so a flipped sign or a swapped index in any term of those branches moves a quaternion component by 1e-7 or more, against a bound near 1e-14; the
face and body diagonals enter the later branches through the tied comparisons.  `xr[2] < 0` flipped: the four `true pose puts point 3 behind` cases choose the
other candidate and the `only candidate behind` cases stop returning identity.  `e < e0` -> `e <= e0`: the exact-tie cases return the last candidate.
tests/test_p3p_edge_cases.py runs these mutants on the oracle, whose three branches are the kernel's text and whose answers equal the kernel's bit for bit: each fails
this module's comparison on 2 (the `<=`) to 209 cases; all 216 single-digit index changes and 18 sign flips of those branches were tried once that way, the least
visible of them failing 15 cases.

Measured on an MI355X, 286 designed + 400 generic problems in one launch:
    (a)-(c) 565 candidates and 263 chosen poses under the error rule, 262 choices asserted (2 of them exact ties); largest err_dev / err_ref 1.000;
            candidates bit-identical to the recorded ones on 286 of 286 designed cases
    (d)     |dR|, |dt| / |x|max and the pose difference all 0: bit-identical on 400 of 400 generic problems
    (e)     109 of 115 sampled problems compared bit for bit with pnp_batch (the other six return identity without an inlier)
No defect was found in csrc/pnp.hip.  The module takes 5 s, 3.5 of them the mp solution sets."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import p3p_cases as PC  # noqa: E402

SUO_ERR_ARG = 1
MARK = 7.25


def _call(xs, ys, n=None, drop=None):
    """suo_debug_p3p; outputs pre-filled with marks; drop: the name of one pointer passed as NULL."""
    from suo_slam_amd import _lib
    lib = _lib.lib()
    m = len(xs)
    a = {"xs": np.ascontiguousarray(xs, np.float64), "ys": np.ascontiguousarray(ys, np.float64), "valid": np.full(m, -7, np.int32), "R": np.full((m, 4, 9), MARK),
         "t": np.full((m, 4, 3), MARK), "qt": np.full((m, 7), MARK), "status": np.full(m, -7, np.int32)}
    p = {k: (None if k == drop else v.ctypes.data) for k, v in a.items()}
    rc = lib.suo_debug_p3p(m if n is None else n, p["xs"], p["ys"], p["valid"], p["R"], p["t"], p["qt"], p["status"])
    return rc, a


@pytest.fixture(scope="module")
def run():
    """The one launch over families A .. F."""
    from suo_slam_amd import _lib
    _lib.require_gpu()
    D = PC.designed()
    g = np.load(PC.os.path.join(PC.HERE, "golden", "pnp_golden.npz"))
    nd = len(D["table"])
    rc, a = _call(np.concatenate([D["xs"], g["xs"]]), np.concatenate([D["ys"], g["ys"]]))
    _lib.check(rc, "suo_debug_p3p")
    out = lambda s: tuple(a[k][s] for k in ("valid", "R", "t", "qt", "status"))      # noqa: E731
    return {"D": D, "designed": out(slice(0, nd)), "generic": out(slice(nd, None)), "gold_a": g}


def test_counts_candidates_and_chosen_pose_on_the_designed_table(run):
    D = run["D"]
    fails, s = PC.compare(D, *run["designed"], ties=PC.tie_cases(D))
    print(f"(a)-(c) {s['cases']} designed cases: {s['candidates']} candidates and {s['poses']} chosen poses under the error rule, {s['choices']} choices asserted; "
          f"largest err_dev / err_ref {s['max_ratio']:.3f}; candidates bit-identical to the recorded ones on {s['bit_identical_cases']} cases")
    assert not fails, (len(fails), fails[:8])
    assert s["candidates"] >= 500 and s["poses"] >= 240 and s["choices"] >= 240


def test_generic_family_at_the_recorded_bound(run):
    valid, R, t, qt, status = run["generic"]
    g = run["gold_a"]
    n = len(g["xs"])
    assert n == 400 and np.array_equal(valid, g["p3p_valid"])
    worst = [0.0, 0.0, 0.0]
    same = 0
    for i in range(n):
        v, xmax = valid[i], np.abs(g["xs"][i]).max()
        fin = np.isfinite(g["p3p_R"][i, :v]).all(1) & np.isfinite(g["p3p_t"][i, :v]).all(1)
        assert np.array_equal(np.isfinite(R[i, :v]).all(1) & np.isfinite(t[i, :v]).all(1), fin), i
        if fin.any():
            worst[0] = max(worst[0], np.abs(R[i, :v][fin] - g["p3p_R"][i, :v][fin]).max())
            worst[1] = max(worst[1], np.abs(t[i, :v][fin] - g["p3p_t"][i, :v][fin]).max() / xmax)
        assert np.all(R[i, v:] == 0) and np.all(t[i, v:] == 0), i
        same += int(np.array_equal(R[i], g["p3p_R"][i], equal_nan=True) and np.array_equal(t[i], g["p3p_t"][i], equal_nan=True))
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = PC.pose_of(qt[i])
        assert np.isfinite(qt[i]).all() and status[i] == int(np.array_equal(g["p4p_T"][i], np.eye(4))), i
        worst[2] = max(worst[2], np.abs(T - g["p4p_T"][i]).max())
        assert np.abs(T - g["p4p_T"][i]).max() < 1e-12, i
    print(f"(d) 400 generic problems: candidates |dR| {worst[0]:.2e}, |dt| / |x|max {worst[1]:.2e}, pose {worst[2]:.2e}; candidates bit-identical on {same} problems")
    assert worst[0] < 1e-12 and worst[1] < 1e-12


def test_the_production_kernel_sees_the_same(run):
    from suo_slam_amd import lambdatwist as lt
    D = run["D"]
    qt = run["designed"][3]
    pick = [i for i, c in enumerate(D["table"]) if (c["family"] == "B" and i % 3 == 0) or c["family"] in "CF"]
    assert len(pick) > 64
    checked = 0
    for part in (pick[:32], pick[32:]):                 # 32 objects: 16 waves each; the rest in one launch: 4 waves each
        T, status, info = lt.pnp_batch([D["xs"][i] for i in part], [D["ys"][i] for i in part], 1e-3, seed=11, refine=False, return_info=True)
        for k, i in enumerate(part):
            if info["best_inliers"][k] > 0:
                Rq, tq = PC.pose_of(qt[i])
                assert np.array_equal(T[k, :3, :3], Rq) and np.array_equal(T[k, :3, 3], tq), (i, D["table"][i]["name"])
                checked += 1
            else:
                assert status[k] == 1 and np.array_equal(T[k], np.eye(4)), (i, D["table"][i]["name"])
    print(f"(e) {checked} of {len(pick)} four-point problems compared bit for bit")
    assert checked >= 0.8 * len(pick)


def test_entry_refusals():
    from suo_slam_amd import _lib
    _lib.require_gpu()
    D = PC.EC.cases()[:5]
    xs, ys = PC.EC.arrays(D)

    def untouched(a):
        return (a["valid"] == -7).all() and (a["status"] == -7).all() and all((a[k] == MARK).all() for k in ("R", "t", "qt"))
    rc, a = _call(xs, ys)
    assert rc == 0 and not untouched(a)
    for n in (0, -3):
        rc, a = _call(xs, ys, n=n)
        assert rc == SUO_ERR_ARG and untouched(a), n
    for key in ("xs", "ys", "valid", "R", "t", "qt", "status"):
        rc, a = _call(xs, ys, drop=key)
        assert rc == SUO_ERR_ARG and untouched(a), key
