"""The mp reference of the bundle-adjustment phases (tests/ba_phases_ref.py) proved on the CPU, and the tolerances of tests/test_gpu_ba_phases.py fixed by it.

1. tests/ba_numpy_phases.NumpyPhases -- float64, dense numpy, written apart from the reference -- against it on every designed graph (tests/ba_phase_cases.py), every
   state (Huber kernel off / on, before / after the chi2 classification) and lambda in {1e-5 maxdiag, 1, 1e6 maxdiag}, buffer by buffer:
   K_ref = max |numpy - mp| / (eps M), M the reference's own error scale (condition numbers folded in for the Schur, solve and update outputs).  The table is printed;
   it must stay at or below ba_phases_ref.K_REF, from which the kernels' tolerance follows as K = max(8, 4 K_REF): 4 because kernels and numpy are plain fp64
   evaluations of the same sums in other orders and trees, 8 so that a buffer on which numpy happens to be nearly exact keeps a few roundings.
2. Seven wrong kernels, as mutants of the reference: each must leave that tolerance by a factor of 100 at least, at one of the lambdas the GPU module runs.
3. classify: the reference's chi2 against NumpyPhases', and the thresholds' separation the GPU module relies on."""
import numpy as np
import pytest

from tests import ba_phase_cases as PC
from tests import ba_phases_ref as R
from tests.ba_numpy_phases import NumpyPhases

EPS = R.EPS


def _ratio(got, ref, M, mutant=False):
    """max |got - ref| / (eps M); an entry whose scale is 0 must be met exactly (a mutant that misses one is told apart by any tolerance)."""
    got, ref, M = (np.asarray(a, np.float64).ravel() for a in (got, ref, M))
    d = np.abs(got - ref)
    if mutant and (d[M == 0] != 0).any():
        return float("inf")
    assert (d[M == 0] == 0).all(), "an entry with no error scale differs"
    return float((d[M > 0] / (EPS * M[M > 0])).max()) if (M > 0).any() else 0.0


def _as_numpy_updates(T0, x, T1):
    """The reference's updated poses with the small-angle shortcut applied as NumpyPhases applies it (ba_phases_ref.oplus): reference and numpy then state ONE definition."""
    T1 = T1.copy()
    for v in range(len(T0)):
        if np.any(x[v]) and R.in_shortcut(x[v]):
            T1[v] = R.oplus(T0[v], x[v], g2o_shortcut=False)[0]
    return T1


def _numpy_against_mp(name):
    """{buffer: K_ref} of one case."""
    cr = R.case(name)
    k = {b: 0.0 for b in R.K_REF}
    for robust_on, classified in R.STATES:
        NP = NumpyPhases(PC.problem(name))
        NP.classify(0 if classified else 1)
        k["chi2"] = max(k["chi2"], _ratio(NP.P.chi2[:cr.ref.E], cr.chi2, cr.Mchi2))
        if classified:
            assert np.array_equal(NP.level, cr.level(1))
        L = cr.lin(robust_on, classified)
        k["lin"] = max(k["lin"], _ratio(NP._linearize(robust_on), L.lin, L.M))
        for which in R.LAMBDAS:
            lam, Sc, U = cr.lam(robust_on, classified, which), cr.sch(robust_on, classified, which), cr.upd(robust_on, classified, which)
            k["sch"] = max(k["sch"], _ratio(NP._schur(lam), Sc.sch, Sc.MC))
            assert Sc.ok == 1.0 and U.ok == 1.0
            o = NP._solve_update(lam, robust_on, cr.ref.totals(L, Sc))
            k["red"] = max(k["red"], _ratio([o[0], o[1], o[3], o[2]], U.red, U.Mred))
            cam, obj = np.stack([T[:3] for T in NP.cam]), np.stack([T[:3] for T in NP.obj])
            ref_cam, ref_obj = _as_numpy_updates(cr.ref.cam_T, U.xc, U.cam_T), _as_numpy_updates(cr.ref.obj_T, U.xo, U.obj_T)
            k["poses"] = max(k["poses"], _ratio(cam, ref_cam, U.MCcam), _ratio(obj, ref_obj, U.MCobj))
            NP.restore()
    return k


@pytest.mark.parametrize("name", PC.NAMES)
def test_numpy_phases_agree_with_the_mp_reference(name):
    k = _numpy_against_mp(name)
    print(f"K_ref {name:7s} " + "  ".join(f"{b} {v:.3g}" for b, v in k.items()))
    for b, v in k.items():
        assert v <= R.K_REF[b], f"{name}: K_ref of {b} is {v:.3g}, above the {R.K_REF[b]} the kernels' tolerance was fixed from"
        assert R.K[b] == max(8.0, 4.0 * R.K_REF[b])


def _mutant_ratio(buf, got, ref, M):
    return _ratio(got, ref, M, mutant=True) / R.K[buf]


def _report(what, ratios):
    print(f"mutant {what}: |mutant - ref| / tolerance = " + ", ".join(f"{k}: {v:.3g}" for k, v in ratios.items()))
    assert max(ratios.values()) >= 100.0, f"{what}: the tolerance does not tell this mutant from the reference"


def test_mutant_one_camera_missing_from_a_slice_sum():
    cr = R.case("slices")
    o = PC.SLICE_LISTS.index(43)
    out = {}
    for which in R.LAMBDAS:
        Sc = cr.sch(1, 1, which)
        mut = cr.ref.schur(cr.lin(1, 1), cr.lam(1, 1, which), mutate=("drop_cam", o))
        out[which] = _mutant_ratio("sch", mut.sch, Sc.sch, Sc.MC)
    _report("S_g of object '43' without one camera", out)
    assert min(out.values()) >= 100.0


def test_mutant_one_pair_missing_from_a_gather():
    cr = R.case("slices")
    L = cr.lin(1, 1)
    mut = cr.ref.linearize(1, cr.level(1), mutate=("drop_pair", PC.SLICE_LISTS.index(9)))
    _report("gather of object '9' without one pair", {"lin": _mutant_ratio("lin", mut.lin, L.lin, L.M)})


def test_mutant_unit_weight_above_delta():
    cr = R.case("small")
    L = cr.lin(1, 0)
    assert any(ed.chi2 > cr.ref.delta ** 2 for ed in cr.ref.edge)
    mut = cr.ref.linearize(1, cr.level(0), mutate=("unit_weight",))
    _report("w = 1 above delta", {"lin": _mutant_ratio("lin", mut.lin[1:], L.lin[1:], L.M[1:])})


def test_mutant_sign_of_info_xy():
    cr = R.case("small")
    mut = R.PhaseRef(cr.prob, flip_xy=True)
    L, Lm = cr.lin(0, 0), mut.linearize(0, cr.level(0))
    _report("info.xy with the other sign", {"lin": _mutant_ratio("lin", Lm.lin, L.lin, L.M), "chi2": _mutant_ratio("chi2", mut.classify()[0], cr.chi2, cr.Mchi2)})


def test_mutant_lambda_left_off_the_camera_blocks():
    cr = R.case("small")
    out = {}
    for which in R.LAMBDAS:
        Sc = cr.sch(1, 1, which)
        mut = cr.ref.schur(cr.lin(1, 1), cr.lam(1, 1, which), mutate=("no_lambda",))
        out[which] = _mutant_ratio("sch", mut.sch, Sc.sch, Sc.MC)
    _report("Hcc without lambda", out)


def test_mutant_fixed_object_given_a_slot():
    cr = R.case("slots")
    nfo = len(cr.ref.free_obj)
    wrong = {o: o % nfo for o in cr.ref.free_obj}           # the slot counter also counts fixed objects (and wraps: the buffer has ns rows)
    assert sorted(wrong.values()) == list(range(nfo)) and wrong != cr.ref.slot
    out = {}
    for which in R.LAMBDAS:
        Sc = cr.sch(1, 1, which)
        mut = cr.ref.schur(cr.lin(1, 1), cr.lam(1, 1, which), mutate=("slots", wrong))
        out[which] = _mutant_ratio("sch", mut.sch, Sc.sch, Sc.MC)
    _report("a fixed object given a slot", out)


def test_mutant_scale_term_without_lambda_x():
    cr = R.case("small")
    out = {}
    for which in R.LAMBDAS:
        U = cr.upd(1, 1, which)
        mut = cr.ref.solve_update(cr.lin(1, 1), cr.sch(1, 1, which), cr.lam(1, 1, which), 1, mutate=("scale_without_lambda",))
        out[which] = _mutant_ratio("red", mut.red, U.red, U.Mred)
    _report("scale = sum x b", out)


@pytest.mark.parametrize("name", PC.NAMES)
def test_classify_chi2_and_flags(name):
    cr = R.case(name)
    NP = NumpyPhases(PC.problem(name))
    NP.classify(0)
    assert _ratio(NP.P.chi2[:cr.ref.E], cr.chi2, cr.Mchi2) <= R.K["chi2"]
    assert np.array_equal(NP.P.inlier, cr.inlier) and NP.good[0] == cr.inlier.sum()
    gap = np.abs(cr.chi2 - cr.prob.chi2_thr) / cr.prob.chi2_thr
    assert gap.min() > 1e-6, "an edge of the case sits on the inlier threshold"
    if name == "slots":
        assert not cr.inlier[cr.prob.edge_cam == PC.SLOTS_CAST_OUT_CAMERA].any()


def test_threshold_edges_stand_apart():
    """The three edges the GPU module moves the threshold onto: no other edge's chi2 within 1e-6 relative."""
    cr = R.case("small")
    for e in R.threshold_edges(cr):
        others = np.delete(cr.chi2, e)
        assert (np.abs(others - cr.chi2[e]) > 1e-6 * cr.chi2[e]).all()
