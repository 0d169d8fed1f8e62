"""The mp reference of the covariance entries (tests/pose_cov_mp_ref.py) proved on the CPU, and the tolerances of the five GPU modules of the family fixed by it.

1. The structured mp inverse (object blocks, reduced camera system, back-substitution) against one dense mp Cholesky of the same H on every case with n <= 48, to
   1e-30 relative; the kernels' route (Schur complement onto the objects) in mp agrees as well.
2. The finite-difference references that the GPU modules used until now (pose_cov_ref, pose_cov_pairs_ref, pose_cov_graph_ref, resid_stats_ref, track_cov_ref)
   against the mp reference: each inside the tolerance its GPU module stated for it (OLD TOLERANCES below restate them), and the table of their error over the new
   scale eps M -- how far the old tests were from measuring the kernels.
3. K_REF: tests/pose_cov_numpy.py -- float64, analytic Jacobians, the header's adjoint formulas -- on its two routes against the mp reference, buffer by buffer:
   K_REF = max |numpy - mp| / (eps M) over both routes and all cases.  The table is printed; it must stay at or below pose_cov_mp_ref.K_REF, from which the
   kernels' tolerance follows as K = max(8, 4 K_REF) (the rule and reasons of tests/test_ba_phases_ref.py).
4. On every case and every output entry the new tolerance K eps M is at most the old one.
5. Eleven wrong kernels, as mutants of the reference: each leaves the new tolerance by a factor of 100 at least; the table says which of them the old tolerance admitted.
6. The studentised residual: no edge has an infinite tolerance, and per case at most one counted edge in ten has tol(t) > 1e-6 max(1, |t|)."""
import functools

import numpy as np
import pytest

from tests import pose_cov_cases as K
from tests import pose_cov_graph_cases as GK
from tests import pose_cov_graph_ref as GR
from tests import pose_cov_mp_ref as M
from tests import pose_cov_numpy as N
from tests import pose_cov_pair_cases as PK
from tests import pose_cov_pairs_ref as PR
from tests import pose_cov_ref as R
from tests import resid_stats_cases as RK
from tests import resid_stats_ref as RS
from tests import track_cov_cases as TC
from tests.ba_phases_ref import _f

EPS = M.EPS
MARGINAL_CASES = [n for n in K.CASES if n != "2x17"] + list(GK.NAMES) + [n for n in PK.CASES if n not in K.CASES]
STAT_KEYS = ("edge_chi2", "edge_pcov", "edge_lev", "edge_t", "cam_stat", "obj_stat", "summary")
STAT_BUF = {"edge_chi2": "chi2", "edge_pcov": "pcov", "edge_lev": "lev", "edge_t": "t", "cam_stat": "vstat", "obj_stat": "vstat", "summary": "summary"}
TRACK_BUF = {"fixed_map_cov": "fixed_map", "cam_cov": "track_cam", "cross": "track_cross", "rel": "track_rel"}


def _pairs_for(name, g):
    """the pair list of a case: that of its GPU module, plus every camera pair on the graphs of the pairs module"""
    if name in GK.CASES:
        return GK.pairs_of(g)
    if name in PK.CASES:
        return np.vstack([PK.case(name)[1], np.array(GK.camera_pairs(g), np.int32)])
    return PK.pairs_of(g, [(0, 1)] if len(g["obj_T"]) > 1 else [])


@functools.lru_cache(maxsize=None)
def _fd(name):
    """(FD reference of pose_cov_ref, pairs, (cross, rel, n_nan) of pose_cov_graph_ref) of a marginal case"""
    g = M.case(name).g
    ref = R.covariances(g)
    pairs = _pairs_for(name, g)
    return ref, pairs, GR.relative(g, ref, pairs)


@functools.lru_cache(maxsize=None)
def _mp_pairs(name):
    return M.case(name).pairs(_fd(name)[1])


# ---- OLD TOLERANCES: what the GPU modules applied to the finite-difference references until now, restated --------------------------------------------------------------
def old_rel_tol(g, a, b, bound):
    nc = len(g["cam_T"])
    if a < nc and b < nc:
        return bound * (1 + 6 * np.abs(PR.adjoint(PR.vertex_pose(g, b) @ np.linalg.inv(PR.vertex_pose(g, a)))).max()) ** 2
    if a < nc or b < nc:
        return bound * (1 + 6 * np.abs(PR.adjoint(PR.vertex_pose(g, min(a, b)))).max()) ** 2
    return 4 * 36 * np.abs(PR.adjoint(np.linalg.inv(PR.vertex_pose(g, b)))).max() ** 2 * bound


def old_stat_tols(g, ref, st):
    """{output: tolerance array} of tests/test_gpu_resid_stats.py as it stood: per edge (t infinite where its propagation gave up), then the sums"""
    E = len(g["edge_cam"])
    b = R.bound(ref) if ref["H"].shape[0] else 0.0
    S = float(np.abs(ref["Sigma"]).max()) if ref["H"].shape[0] else 0.0
    tol = {k: np.zeros(E) for k in ("pcov", "lev", "chi2", "t")}
    for e in range(E):
        J, v = st["J"][e], st["v"][e]
        a = float(np.abs(J).sum(1).max())
        i = np.abs(g["edge_info"][e])
        Om = np.array([[g["edge_info"][e][0], g["edge_info"][e][1]], [g["edge_info"][e][1], g["edge_info"][e][2]]])
        om = float(i[0] + 2 * i[1] + i[2])
        dJ = 16 * EPS * (1 + float(np.abs(g["edge_uv"][e]).max())) / R.STEP + 10 * a * R.STEP ** 2
        dv = 400 * EPS * (1 + a)
        av = np.abs(v)
        tol["chi2"][e] = 2 * dv * float((np.abs(Om) @ av).sum()) + dv * dv * om + 8 * EPS * float(av @ np.abs(Om) @ av)
        if np.isnan(st["edge_lev"][e]):
            continue
        tp = b * a * a + 24 * dJ * S * a + 30 * EPS * S * a * a
        p = st["edge_pcov"][e]
        P = np.array([[p[0], p[1]], [p[1], p[2]]])
        tol["pcov"][e] = tp
        tol["lev"][e] = tp * om + 8 * EPS * float((np.abs(P) * np.abs(Om)).sum())
        if np.isnan(st["edge_t"][e]):
            continue
        s = -1.0 if st["counted"][e] else 1.0
        Minv = np.linalg.inv(np.linalg.inv(Om) + s * P)
        x1 = float(np.abs(Minv @ v).sum())
        k = tp * float(np.abs(Minv).sum())
        if k >= 0.5:
            tol["t"][e] = np.inf
            continue
        Rm = np.eye(2) + s * P @ Om
        cancel = (abs(Rm[0, 0] * Rm[1, 1]) + abs(Rm[0, 1] * Rm[1, 0])) / st["det"][e]
        tol["t"][e] = (x1 * x1 * tp + 2 * x1 * dv + dv * dv * float(np.abs(Minv).sum())) / (1 - k) + 64 * EPS * cancel * float(np.abs(Om @ v) @ np.abs(np.linalg.inv(Rm)) @ av)
    sum_tol = lambda members, tols: float(np.sum(tols) + len(members) * EPS * np.abs(members).sum())
    out = {"edge_chi2": tol["chi2"], "edge_pcov": np.repeat(tol["pcov"][:, None], 3, 1), "edge_lev": tol["lev"], "edge_t": tol["t"]}
    cnt = st["counted"]
    for key, idx, n_v in (("cam_stat", g["edge_cam"], len(g["cam_T"])), ("obj_stat", g["edge_obj"], len(g["obj_T"]))):
        t = np.zeros((n_v, 3))
        for v in range(n_v):
            k = np.flatnonzero((idx == v) & cnt)
            t[v, 1], t[v, 2] = sum_tol(st["edge_chi2"][k], tol["chi2"][k]), sum_tol(2 - st["edge_lev"][k], tol["lev"][k])
        out[key] = t
    k = np.flatnonzero(cnt)
    dof = st["summary"][4]
    t_chi2 = sum_tol(st["edge_chi2"][k], tol["chi2"][k])
    t_lev = sum_tol(st["edge_lev"][k], tol["lev"][k]) if not np.isnan(st["summary"][3]) else 0.0
    out["summary"] = np.array([0, 0, t_chi2, t_lev, 0, (t_chi2 / dof + 4 * EPS * abs(st["summary"][5])) if dof > 0 else 0.0])
    return out


def old_track_tols(g, Sigma, ref, c):
    cf = 1e3 * EPS * ref["cond"][c]
    cam = cf * (ref["hinv_max"][c] + 2 * ref["gsg_max"][c])
    tol = {"fixed_map_cov": cf * ref["hinv_max"][c], "cam_cov": cam, "cross": cf * ref["gs_max"][c], "rel": cam * (1 + 6 * ref["a_max"][c]) ** 2}
    if g["cam_fixed"][c]:
        O = len(g["obj_T"])
        diag = max((np.abs(Sigma[6 * o:6 * o + 6, 6 * o:6 * o + 6]).max() for o in range(O) if not np.isnan(Sigma[6 * o, 6 * o])), default=0.0)
        tol["rel"] = 1e3 * EPS * (6 * ref["a_max"][c]) ** 2 * diag
    return tol


def _over(got, ref, tol):
    """max |got - ref| / tol over the entries where ref is a number and tol is positive and finite (an old tolerance of 0 stood for an exact zero)"""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    tol = np.broadcast_to(np.asarray(tol, float), ref.shape)
    ok = ~np.isnan(ref) & ~np.isnan(got) & (tol > 0) & np.isfinite(tol)
    return float((np.abs(got - ref)[ok] / tol[ok]).max()) if ok.any() else 0.0


# ---- what a set of outputs is, for the three comparisons (FD reference, numpy restatement, mutant) ------------------------------------------------------------------
def _family_new(name, cam, obj, cross, rel):
    """{buffer: max |x - mp| / (eps M)} of marginal blocks and pair blocks against the mp reference of a marginal case (or of (CovRef, its pairs))"""
    cr, pr = (M.case(name), _mp_pairs(name)) if isinstance(name, str) else name
    mg = cr.marginals()
    return {"sigma": max(M.ratio(cam, mg.cam_cov, mg.M_cam, True), M.ratio(obj, mg.obj_cov, mg.M_obj, True)),
            "cross": M.ratio(cross, pr.cross, pr.M_cross, True), "rel": M.ratio(rel, pr.rel, pr.M_rel, True)}


def _family_old(name, cam, obj, cross, rel):
    """max |x - FD reference| / old tolerance over the same outputs: at most 1 means the old GPU tests would have passed x"""
    ref, pairs, (rcross, rrel, _) = _fd(name) if isinstance(name, str) else name[1:]
    g, b = (M.case(name).g if isinstance(name, str) else name[0]), R.bound(ref)
    worst = max(_over(cam, ref["cam_cov"], b), _over(obj, ref["obj_cov"], b), _over(cross, rcross, b))
    for q, (a, c) in enumerate(pairs.tolist()):
        worst = max(worst, _over(rel[q], rrel[q], old_rel_tol(g, a, c, b)))
    return worst


def _stats_new(st_ref, out):
    return {STAT_BUF[k] + ("" if k not in ("cam_stat", "obj_stat") else ":" + k[:3]): M.ratio(out[k], getattr(st_ref, k), getattr(st_ref, "M_" + k), True) for k in STAT_KEYS}


def _as_dict(ns):
    return {k: getattr(ns, k) for k in STAT_KEYS}


# ---- 1 -------------------------------------------------------------------------------------------------------------------------------------------------------------------
def _rows_at_most(name):
    g = M._graph_of(name)
    return 6 * int((np.asarray(g["cam_fixed"]) == 0).sum() + (np.asarray(g["obj_fixed"]) == 0).sum())


@pytest.mark.parametrize("name", [n for n in dict.fromkeys(MARGINAL_CASES + RK.NAMES) if n != "no_edges" and _rows_at_most(n) <= 48])
def test_the_structured_inverse_is_the_dense_one(name):
    cr = M.case(name)
    S, D = cr.structured(), cr.dense()
    scale = np.sqrt(np.abs(np.outer(np.diag(_f(D)), np.diag(_f(D)))))
    assert float(np.abs(_f(S - D) / scale).max()) <= 1e-30
    if cr.coupled:
        assert float(np.abs(_f(cr.objects_route() - D) / scale).max()) <= 1e-30


# ---- 2 and 4 -----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MARGINAL_CASES)
def test_fd_references_of_blocks_and_pairs_sit_inside_their_bound_and_the_new_tolerance_is_tighter(name):
    ref, pairs, (rcross, rrel, n_nan) = _fd(name)
    cr, pr = M.case(name), _mp_pairs(name)
    mg = cr.marginals()
    g, b = cr.g, R.bound(ref)
    assert list(mg.status) == list(ref["status"]) and pr.n_nan == n_nan
    new = _family_new(name, ref["cam_cov"], ref["obj_cov"], rcross, rrel)
    own = max(_over(ref["cam_cov"], mg.cam_cov, b), _over(ref["obj_cov"], mg.obj_cov, b), _over(rcross, pr.cross, b))
    own_rel = max([_over(rrel[q], pr.rel[q], old_rel_tol(g, a, c, b)) for q, (a, c) in enumerate(pairs.tolist())], default=0.0)
    print(f"FD reference {name:15s} n {cr.n:3d}  own error / old bound: blocks {own:.4f}  rel {own_rel:.4f}   error / (eps M): "
          + "  ".join(f"{k} {v:.1f}" for k, v in new.items()))
    assert own <= 1.0 and own_rel <= 1.0, "the finite-difference reference is outside the bound its GPU module stated"
    # 4: entry by entry
    assert (M.tol("sigma", mg.M_cam) <= b).all() and (M.tol("sigma", mg.M_obj) <= b).all() and (M.tol("cross", pr.M_cross) <= b).all()
    for q, (a, c) in enumerate(pairs.tolist()):
        assert (M.tol("rel", pr.M_rel[q]) <= old_rel_tol(g, a, c, b)).all(), (name, q, a, c)


@pytest.mark.parametrize("name", RK.NAMES)
def test_fd_reference_of_the_statistics_sits_inside_its_tolerances_and_the_new_ones_are_tighter(name):
    g, ref, old = RK.case(name)
    st = M.case(name).statistics()
    assert list(st.status) == list(old["status"]) and np.array_equal(st.counted, old["counted"])
    otol = old_stat_tols(g, ref, old)
    own = {k: _over(old[k], getattr(st, k), otol[k]) for k in STAT_KEYS}
    new = _stats_new(st, old)
    print(f"FD reference {name:18s} own error / old tolerance: " + "  ".join(f"{k} {v:.1e}" for k, v in own.items()) + "   error / (eps M): "
          + "  ".join(f"{k} {v:.1f}" for k, v in new.items()))
    assert max(own.values()) <= 1.0
    for k in STAT_KEYS:
        ok = ~np.isnan(getattr(st, k))
        assert (M.tol(STAT_BUF[k], getattr(st, "M_" + k))[ok] <= np.broadcast_to(otol[k], ok.shape)[ok]).all(), (name, k)


@pytest.mark.parametrize("n_obj", sorted(TC.SIZES))
def test_fd_reference_of_the_tracking_covariances_sits_inside_its_tolerances_and_the_new_ones_are_tighter(n_obj):
    g, Sigma, ref = TC.case(n_obj)
    tr = M.track_case(n_obj)
    assert list(tr.status) == list(ref["status"])
    own, new = dict.fromkeys(TRACK_BUF, 0.0), {}
    for c in range(len(g["cam_T"])):
        otol = old_track_tols(g, Sigma, ref, c)
        for k in TRACK_BUF:
            own[k] = max(own[k], _over(ref[k][c], getattr(tr, k)[c], otol[k]))
            ok = ~np.isnan(getattr(tr, k)[c])
            Mk = getattr(tr, "M_" + k)[c]
            # (the old tolerance of a fixed camera's zero blocks was 0: exactness, which M == 0 still asks for)
            assert (M.tol(TRACK_BUF[k], Mk)[ok] <= otol[k]).all(), (n_obj, c, k, float(M.tol(TRACK_BUF[k], Mk)[ok].max()), otol[k])
    for k in TRACK_BUF:
        new[k] = M.ratio(ref[k], getattr(tr, k), getattr(tr, "M_" + k), True)
    print(f"FD reference track {n_obj:2d} objects  own error / old tolerance: " + "  ".join(f"{k} {v:.4f}" for k, v in own.items()) + "   error / (eps M): "
          + "  ".join(f"{k} {v:.1f}" for k, v in new.items()))
    assert max(own.values()) <= 1.0


# ---- 3 -------------------------------------------------------------------------------------------------------------------------------------------------------------------
def _hold(measured):
    for buf, v in measured.items():
        buf = buf.split(":")[0]
        assert v <= M.K_REF[buf], f"K_ref of {buf} is {v:.3g}, above the {M.K_REF[buf]} the kernels' tolerance was fixed from"
        assert M.K[buf] == max(8.0, 4.0 * M.K_REF[buf])


@pytest.mark.parametrize("name", MARGINAL_CASES)
def test_numpy_blocks_and_pairs_agree_with_the_mp_reference_on_both_routes(name):
    g, pairs = M.case(name).g, _fd(name)[1]
    worst = {}
    for route in ("dense", "schur"):
        nc = N.NumpyCov(g, route)
        k = _family_new(name, *nc.marginals(), *nc.pairs(pairs))
        print(f"K_ref {name:15s} {route:5s} " + "  ".join(f"{b} {v:.3g}" for b, v in k.items()))
        worst = {b: max(v, worst.get(b, 0.0)) for b, v in k.items()}
    _hold(worst)


@pytest.mark.parametrize("name", RK.NAMES)
def test_numpy_statistics_agree_with_the_mp_reference_on_both_routes(name):
    cr = M.case(name)
    worst = {}
    for route in ("dense", "schur"):
        nc = N.NumpyCov(cr.g, route)
        k = _stats_new(cr.statistics(), nc.statistics())
        cam, obj = nc.marginals()
        k["sigma"] = max(M.ratio(cam, cr.marginals().cam_cov, cr.marginals().M_cam, True), M.ratio(obj, cr.marginals().obj_cov, cr.marginals().M_obj, True))
        print(f"K_ref {name:18s} {route:5s} " + "  ".join(f"{b} {v:.3g}" for b, v in k.items()))
        worst = {b: max(v, worst.get(b, 0.0)) for b, v in k.items()}
    _hold(worst)


@pytest.mark.parametrize("n_obj", sorted(TC.SIZES))
def test_numpy_tracking_covariances_agree_with_the_mp_reference(n_obj):
    g, Sigma, _ = TC.case(n_obj)
    tr, nt = M.track_case(n_obj), N.tracking(g, Sigma)
    k = {TRACK_BUF[key]: M.ratio(nt[key], getattr(tr, key), getattr(tr, "M_" + key), True) for key in TRACK_BUF}
    print(f"K_ref track {n_obj:2d} objects " + "  ".join(f"{b} {v:.3g}" for b, v in k.items()))
    _hold(k)


# ---- 5 -------------------------------------------------------------------------------------------------------------------------------------------------------------------
def _report(what, new, old):
    """new: {buffer: |mutant - mp| / (eps M)}; old: max |mutant - FD reference| / old tolerance"""
    over = {b: v / M.K[b.split(":")[0]] for b, v in new.items()}
    print(f"mutant {what}: |mutant - ref| / new tolerance = " + ", ".join(f"{k}: {v:.3g}" for k, v in over.items())
          + f";  / old tolerance = {old:.3g} ({'ADMITTED' if old <= 1.0 else 'caught'} by the old tests)")
    assert max(over.values()) >= 100.0, f"{what}: the tolerance does not tell this mutant from the reference"
    return old <= 1.0


def _blocks_mutant(name, mutate=None, pair_mutate=None):
    cr = M.case(name) if mutate is None else M.CovRef(M.case(name).g, mutate)
    mg, pr = cr.marginals(), cr.pairs(_fd(name)[1], mutate=pair_mutate)
    out = (mg.cam_cov, mg.obj_cov, pr.cross, pr.rel)
    return _family_new(name, *out), _family_old(name, *out)


def _designed_mutant(g, pairs, mutate=None, pair_mutate=None):
    """the same for a graph designed for one mutant: its own mp and finite-difference references"""
    cr, mut = M.CovRef(g), (M.CovRef(g, mutate) if mutate else None)
    ref = R.covariances(g)
    mg, pr = (mut or cr).marginals(), (mut or cr).pairs(pairs, mutate=pair_mutate)
    out = (mg.cam_cov, mg.obj_cov, pr.cross, pr.rel)
    return _family_new((cr, cr.pairs(pairs)), *out), _family_old((g, ref, np.asarray(pairs), GR.relative(g, ref, pairs)), *out)


def _stats_old(name, out):
    g, ref, old = RK.case(name)
    otol = old_stat_tols(g, ref, old)
    exact = all(np.array_equal(out[k][..., i], old[k][..., i]) for k, i in (("cam_stat", 0), ("obj_stat", 0))) and list(out["summary"][[0, 1, 4]]) == list(old["summary"][[0, 1, 4]])
    return max(_over(out[k], old[k], otol[k]) for k in STAT_KEYS) if exact else float("inf")


def _q(name, a, b):
    return _fd(name)[1].tolist().index([a, b])


BARELY, NEAR = 1.6e-5, 1e-5


def _stats_mutant(name, what, cov_mutate=None, stat_mutate=None):
    cr = M.case(name) if cov_mutate is None else M.CovRef(M.case(name).g, cov_mutate)
    mut = _as_dict(cr.statistics(mutate=stat_mutate) if stat_mutate else cr.statistics())
    return what, _stats_new(M.case(name).statistics(), mut), _stats_old(name, mut)


def _m_hco():
    return [("Hco(1, 0) of 3x2 times 1 + 1e-9", *_blocks_mutant("3x2", ("hco_scale", 1, 0)))]


def _m_flip_xy():
    assert M.case("3x2").counted[0]
    return [("info_xy of edge 0 of 3x2 with the other sign", *_blocks_mutant("3x2", ("flip_xy", 0)))]


def _m_drop_cam():
    g = K.case("3x2")[0]                 # where that camera barely sees the object: its edges with object 1 carry BARELY of their information
    g["edge_info"][(g["edge_cam"] == 2) & (g["edge_obj"] == 1)] *= BARELY
    return [("S(1, 1) of 3x2 without camera 2", *_blocks_mutant("3x2", ("drop_cam", 2, 1))),
            ("S(1, 1) of 3x2 without camera 2, which barely sees object 1", *_designed_mutant(g, PK.pairs_of(g), ("drop_cam", 2, 1)))]


def _m_outlier():
    e = int(np.flatnonzero(M.case("flagged_3x2").g["edge_inlier"] == 0)[0])
    return [_stats_mutant("flagged_3x2", f"edge {e} of flagged_3x2 (edge_inlier == 0) counted", cov_mutate=("count", e))]


def _m_both_fixed():
    g = M.case("fixed_pair_3x2").g
    e = int(np.flatnonzero((g["edge_cam"] == 0) & (g["edge_obj"] == 1))[0])
    return [_stats_mutant("fixed_pair_3x2", f"edge {e} of fixed_pair_3x2 (both vertices fixed) counted", cov_mutate=("count", e))]


def _m_wrong_cross():
    return [("Sigma_co of (1, object 0) of 5x16 returned as Sigma_oc^T of (1, object 1)",
             *_blocks_mutant("5x16", pair_mutate=("wrong_cross", _q("5x16", 1, 5 + 0), 1, 5 + 1)))]


def _m_no_tR():
    g = K.case("3x2")[0]                 # a pose near the origin: camera 1 moved to NEAR of its distance from it
    g["cam_T"][1][:, 3] *= NEAR
    pairs = PK.pairs_of(g)
    return [("rel of (camera 1, object 0) of 3x2 with Ad = blockdiag(R, R)", *_blocks_mutant("3x2", pair_mutate=("no_tR", _q("3x2", 1, 3 + 0)))),
            ("the same with camera 1 near the origin", *_designed_mutant(g, pairs, pair_mutate=("no_tR", pairs.tolist().index([1, 3]))))]


def _m_plus_ab():
    return [("rel of objects (0, 1) of 5x16 with + Sigma_ab", *_blocks_mutant("5x16", pair_mutate=("plus_ab", _q("5x16", 5 + 0, 5 + 1))))]


def _m_lev_scaled():
    return [_stats_mutant("3x2", "leverages of 3x2 from s0^2 Sigma", stat_mutate=("lev_scaled",))]


def _m_t_neighbour():
    return [_stats_mutant("3x2", "t of edge 0 of 3x2 with P of edge 1", stat_mutate=("t_neighbour", 0))]


def _m_no_gsg():
    g, Sigma, ref = TC.case(2)
    tr, mut = M.track_case(2), M.tracking(g, Sigma, mutate=("no_gsg", 0, 0))
    new = {TRACK_BUF[k]: M.ratio(getattr(mut, k), getattr(tr, k), getattr(tr, "M_" + k), True) for k in TRACK_BUF}
    old = max(_over(getattr(mut, k)[c], ref[k][c], old_track_tols(g, Sigma, ref, c)[k]) for k in TRACK_BUF for c in range(3))
    return [("P_0 of the 2-object tracking graph without object 0's G Sigma G^T", new, old)]


MUTANTS = {"hco_scaled": _m_hco, "info_xy_flipped": _m_flip_xy, "camera_dropped_from_schur_sum": _m_drop_cam, "outlier_edge_counted": _m_outlier,
           "both_fixed_edge_counted": _m_both_fixed, "cross_block_of_the_wrong_pair": _m_wrong_cross, "adjoint_without_tR": _m_no_tR,
           "object_pair_with_plus_sigma_ab": _m_plus_ab, "leverage_from_scaled_sigma": _m_lev_scaled, "t_with_the_neighbours_pcov": _m_t_neighbour,
           "tracking_without_one_objects_gain": _m_no_gsg}


@functools.lru_cache(maxsize=None)
def _mutant(name):
    """every site of the mutant reported and held 100 times outside the new tolerance; True when the old tolerance admitted its last (its subtlest) site"""
    return [_report(*site) for site in MUTANTS[name]()][-1]


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_leaves_the_new_tolerance_by_a_factor_of_100(name):
    _mutant(name)


def test_the_old_tolerances_admitted_at_least_three_of_the_mutants():
    admitted = [name for name in MUTANTS if _mutant(name)]
    print("admitted by the old tolerances: " + ", ".join(admitted))
    assert len(MUTANTS) == 11 and len(admitted) >= 3


# ---- 6 -------------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RK.NAMES)
def test_the_tolerance_of_t_is_finite_and_seldom_wide(name):
    st = M.case(name).statistics()
    fin = ~np.isnan(st.edge_t)
    tt = M.tol("t", st.M_edge_t)
    assert np.isfinite(tt[fin]).all()
    wide = fin & st.counted & (tt > 1e-6 * np.maximum(1.0, np.abs(np.nan_to_num(st.edge_t))))
    print(f"t cap {name:18s} counted {int(st.counted.sum()):3d}  tol(t) > 1e-6 max(1, |t|): {int(wide.sum())}")
    assert 10 * int(wide.sum()) <= int(st.counted.sum()), (name, int(wide.sum()), int(st.counted.sum()))
