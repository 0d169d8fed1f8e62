"""The refinement half of pnp_batch_kernel (csrc/pnp.hip: select_inliers, refine_normal_eqs, refine_cost, refine_pass, chol6, quat_plus and refine_sequence, the very
functions the production kernel calls) reached through suo_debug_pnp_refine, against the mp reference of tests/pnp_refine_ref.py over the designed table of
tests/pnp_refine_cases.py: ONE launch, one wave per row.

(a) system     H, g, cost at the start against the mp system, in units that follow from how each is formed, bound (n_sel + 16) 2^-53
(b) rules      both selections, the RANSAC count, m, deltas and the second-pass flag equal the mp rules exactly on every row that is not near; class E with no exclusions
(c) descent    in mp at the kernel's output bits the cost over the kernel's own selection does not rise by more than twice the cost bound of (a), on every row; rows
               with an empty selection or a start cost that is not finite return the start bit for bit
(d) trajectory the pose after the first pass and the final pose against lm / sequence in mp on every row that is not near; the bound is 4 x the worst distance of
               orc_pnp_refine_debug from the same mp result over the row's class, computed here (the factor pays for the DPP tree sums and the one-reciprocal-per-
               pivot Cholesky against the oracle's sequential forms); tests/test_pnp_refine_ref.py holds that class bound below 1e-9 on A, B, D
(e) optimum    class A rows whose mp run stopped on a tolerance: the gradient in mp at the kernel's final bits is within the tolerance that ended the run, and the
               final pose is no farther from the mp minimiser than the mp run's own end plus bound (d).  (The algorithm stops on its gradient tolerance, up to dR
               8.8e-5 from the minimum in mp itself: see tests/test_pnp_refine_ref.py.)
(f) same code  class A and D rows started from four indices: SEQUENCE equals suo_pnp_replay with those indices in every row of the draw table bit for bit, at both
               launch widths (1 object: 16 waves; 33: 4 waves); with refine off the replay returns the reported start
(g) refusals   leave marked output buffers untouched

Measured on an MI355X, 140 rows, kernel | oracle (both against mp):
    (a) H 6.8 | 10.2 units of 2^-53 (0.40 of the bound at worst), g 0.94 | 0.94 (0.04), cost 0.72 | 0.72 (0.04)     (b) exact on all 140 rows
    (c) no pass raises its cost: worst change 0 (rows that start within their gradient tolerance), 129 first passes and 15 second passes checked
    (d) worst dR / dt per class:  A 2.4e-15 / 3.9e-16 | 2.3e-15 / 5.1e-16    B 3.1e-13 / 3.2e-15 | 2.8e-13 / 5.0e-15    C 1.9e-10 / 1.3e-10 | 1.0e-10 / 7.1e-11
        D 3.6e-16 / 3.9e-16 | the same    E 8.4e-17 / 1.1e-16 | 8.4e-17 / 1.0e-16    F 3.3e-14 / 8.5e-15 | 4.3e-14 / 6.5e-15   (bound: 4 x the oracle's)
    (e) gradient at the end 0.91 of the tolerance at worst; 1.1e-15 / 2.3e-16 beyond the mp run's own distance from the minimiser     (f), (g) hold
Seeded changes to csrc/pnp.hip, each built, run once and reverted:
    sign of D[2][1] flipped (2 * rx for -2 * rx)    fails (a) H by 2.5e17 units, (b), (d) dR 3.7e-3 on class A, (e) gradient 4.2e4 x the tolerance; (c) and (f) pass:
                                                    the pose still descends, as the statistical tests always saw
    slot loop of the normal equations stops at 15   fails (a) H by 9.0e15 units and (d) dR 4.1e-3, on the 1023- and 1024-point rows of class B; (f) passes
    `>` -> `>=` in select_inliers                   fails (b) on the three err == thr^2 rows of class E and (a) there (the system of another selection); (f) passes
The whole module takes 12 s, 10 of them the mp references."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import geometry as G  # noqa: E402
from tests import pnp_refine_cases as PC  # noqa: E402


def _call(a, n_obj=None, like=None):
    """suo_debug_pnp_refine on packed arguments (like: the complete arguments the sizes are taken from, where `a` has a pointer set to None); returns
    (rc, out_d, out_i, sel0, sel1), the outputs pre-filled with marks."""
    from suo_slam_amd import _lib
    lib = _lib.lib()
    like = a if like is None else like
    n_obj = len(like["n"]) if n_obj is None else n_obj
    out_d, out_i = np.full((len(like["n"]), PC.OUT_D), 7.0), np.full((len(like["n"]), 8), -7, np.int32)
    s0, s1 = np.full(max(len(like["sel"]), 1), -7, np.int32), np.full(max(len(like["sel"]), 1), -7, np.int32)
    p = {k: (v.ctypes.data if v is not None else None) for k, v in a.items()}
    rc = lib.suo_debug_pnp_refine(n_obj, p["n"], p["xs"], p["ys"], PC.THR, p["mode"], p["qt"], p["idx"], p["sel"], p["max_iter"], p["tol"], out_d.ctypes.data,
                                  out_i.ctypes.data, s0.ctypes.data, s1.ctypes.data)
    return rc, out_d, out_i, s0, s1


def _run(rows, idx_start=False):
    from suo_slam_amd import _lib
    rc, out_d, out_i, s0, s1 = _call(PC.pack(rows, idx_start))
    _lib.check(rc, "suo_debug_pnp_refine")
    return PC.unpack(rows, out_d, out_i, s0, s1)


@pytest.fixture(scope="module")
def run():
    """The one launch over the table, the mp references, the oracle's run and the class bounds."""
    from suo_slam_amd import _lib
    _lib.require_gpu()
    rows, refs = PC.table(), PC.references()
    got = _run(rows)
    orc = PC.measure(PC.run_oracle(rows))
    return {"rows": rows, "refs": refs, "got": got, "M": PC.measure(got), "O": orc, "bound": PC.class_bounds(orc), "cls": PC.classes(),
            "near": np.array([r["near"] for r in refs])}


def _why(run, k):
    return f"row {k} [{run['rows'][k]['cls']}] {run['rows'][k]['why']}"


def test_system_matches_the_mp_system(run):
    s = run["M"]["sys"]
    ok = ~np.isnan(s[:, 0])
    assert ok.sum() >= 100
    ratio = s[ok, :3] / s[ok, 3:4]
    print(f"(a) kernel system error in units of 2^-53: H {s[ok, 0].max():.2f}  g {s[ok, 1].max():.2f}  cost {s[ok, 2].max():.2f};  / bound: H {ratio[:, 0].max():.3f}  "
          f"g {ratio[:, 1].max():.3f}  cost {ratio[:, 2].max():.3f}")
    for c in range(3):
        assert ratio[:, c].max() <= 1.0, (("H", "g", "cost")[c], _why(run, int(np.flatnonzero(ok)[ratio[:, c].argmax()])), ratio[:, c].max())


def test_rules_equal_the_mp_rules(run):
    must = ~run["near"] | (run["cls"] == "E")
    bad = np.flatnonzero(must & ~run["M"]["rules"])
    print(f"(b) rules compared exactly on {int(must.sum())} rows")
    assert len(bad) == 0, [_why(run, k) for k in bad]


def test_every_pass_descends(run):
    d, same = run["M"]["descent"], run["M"]["same_start"]
    print(f"(c) cost change / slack: first pass worst {np.nanmax(d[:, 0]):.3g} over {int((~np.isnan(d[:, 0])).sum())} rows, second pass worst {np.nanmax(d[:, 1]):.3g} over "
          f"{int((~np.isnan(d[:, 1])).sum())} rows")
    assert same.all(), [_why(run, k) for k in np.flatnonzero(~same)]
    assert np.nanmax(d[:, 0]) <= 1.0, _why(run, int(np.nanargmax(d[:, 0])))
    assert np.nanmax(d[:, 1]) <= 1.0, _why(run, int(np.nanargmax(d[:, 1])))
    assert (~np.isnan(d[:, 0])).sum() >= 100 and (~np.isnan(d[:, 1])).sum() >= 10


def test_trajectory_matches_the_mp_algorithm(run):
    M, cls, near = run["M"], run["cls"], run["near"]
    for c in "ABCDEF":
        m = (cls == c) & ~near
        k = np.concatenate([M["mid"][m], M["fin"][m]]).max(0)
        o = run["bound"][c] / 4
        print(f"(d) class {c}: {int(m.sum())} rows, kernel dR {k[0]:.2e} dt {k[1]:.2e} | oracle dR {o[0]:.2e} dt {o[1]:.2e} | bound dR {4 * o[0]:.2e} dt {4 * o[1]:.2e}")
    for c in "ABCDEF":
        for k in np.flatnonzero((cls == c) & ~near):
            for key in ("mid", "fin"):
                assert M[key][k][0] <= run["bound"][c][0] and M[key][k][1] <= run["bound"][c][1], (_why(run, k), key, M[key][k], run["bound"][c])


def test_class_a_ends_at_the_optimum(run):
    O = PC.optimum_errors(run["got"])
    B = run["bound"]["A"]
    assert len(O) >= 30
    print(f"(e) gradient at the kernel's end / tolerance, worst {max(v[2] for v in O.values()):.3f}; beyond the mp run's own distance from the minimiser, worst dR "
          f"{max(v[0][0] - v[1][0] for v in O.values()):.2e} dt {max(v[0][1] - v[1][1] for v in O.values()):.2e}")
    for k, (got, own, g) in O.items():
        assert g <= 1.0 + 1e-6, (_why(run, k), g)
        assert got[0] <= own[0] + B[0] and got[1] <= own[1] + B[1], (_why(run, k), got, own)


def _T34(q, t):
    return np.concatenate([G.quat_to_rot(q), np.asarray(t).reshape(3, 1)], 1)          # (the kernel's quat_to_rot, operation for operation)


def test_sequence_is_the_production_code(run):
    """(f): bit for bit against suo_pnp_replay whose every hypothesis is the row's four indices."""
    from suo_slam_amd import lambdatwist as lt
    rows = [r for r in run["rows"] if r["cls"] in "AD"]
    assert len(rows) > 33                        # (33 in one launch: 4 waves per object; the rest one by one: 16 waves)
    got = _run(rows, idx_start=True)
    tabs = [np.tile(np.asarray(r["idx"], np.int32), (1000, 1)) for r in rows]
    for refine in (True, False):
        T33, i33 = lt.pnp_replay_batch([r["xs"] for r in rows[:33]], [r["ys"] for r in rows[:33]], tabs[:33], PC.THR, refine=refine)
        T1 = [lt.pnp_replay(r["xs"], r["ys"], tab, PC.THR, refine=refine) for r, tab in zip(rows[33:], tabs[33:])]
        T = np.concatenate([T33, np.stack([x[0] for x in T1])])
        best = np.concatenate([i33["best_inliers"], [x[1]["best_inliers"] for x in T1]])
        refined = 0
        for k, (r, g) in enumerate(zip(rows, got)):
            assert best[k] == g["count"], (r["why"], best[k], g["count"])
            start = _T34(g["q0"], g["t0"])
            want = g["T"] if (refine and g["count"] > 3) else start                       # (PNP::compute refines only a consensus of more than three)
            refined += int(refine and g["count"] > 3 and not np.array_equal(g["T"], start))
            assert np.array_equal(T[k, :3, :], want), (r["why"], refine, np.abs(T[k, :3, :] - want).max())
            assert np.array_equal(_T34(g["q"], g["t"]), g["T"]) and np.array_equal(_T34(g["qm"], g["tm"]), g["Tm"])
        assert not refine or refined >= 20


def test_refusals_leave_the_outputs_untouched():
    from suo_slam_amd import _lib
    _lib.require_gpu()
    rows = [r for r in PC.table() if r["cls"] == "B"][:4]

    def refused(b, n_obj=None):
        rc, out_d, out_i, s0, s1 = _call(b, n_obj, like=a)
        return rc != 0 and (out_d == 7.0).all() and (out_i == -7).all() and (s0 == -7).all() and (s1 == -7).all()
    a = PC.pack(rows)
    assert _call(a)[0] == 0
    assert refused(a, 0) and refused(a, -2)
    for key in a:
        b = dict(a)
        b[key] = None
        assert refused(b), key
    b = dict(a)
    b["n"] = a["n"].copy()
    b["n"][1] = 1025
    assert refused(b)
    b["n"][1] = -1
    assert refused(b)
    for bad in (51, -1):
        b = dict(a)
        b["max_iter"] = a["max_iter"].copy()
        b["max_iter"][2] = bad
        assert refused(b)
    b = dict(a)
    b["mode"] = a["mode"].copy()
    b["mode"][0] = 2
    assert refused(b)
    for bad in ([0, 1, 2, int(a["n"][3])], [0, -1, 2, 3]):
        b = dict(a)
        b["idx"] = a["idx"].copy()
        b["idx"][3] = bad
        assert refused(b)
    big = PC.make_object(1, 1025, 0.0)
    a = PC.pack([PC._row("B", "1025 points", big[0], big[1], big[2], big[3], PC.PASS, np.ones(1025), 1, 1e-6)])
    assert refused(a)
