"""Covariance of a tracked camera with the map's uncertainty carried in (csrc/track_cov.hip through suo_tracking_covariances) against the mp reference of
tests/pose_cov_mp_ref.py (tracking()), on the graphs of tests/track_cov_cases.py.

Tolerances, entry by entry, K[buffer] eps M with K fixed on the CPU by tests/test_pose_cov_mp_ref.py (which also shows each at or below the old tolerance), A = Hcc^-1:
  fixed_map_cov   M_A = |A| MHcc |A| + |A| sqrt(diag H (x) diag H) |A|
  cross           dG = -A dH G keeps its structure: |A| MH' |G Sigma| + |A| (M_B + |B|) |Sigma| + |G| |Sigma|
  cam_cov         M_A + 2 |A| MH' |G Sigma G^T| + 2 |A| (M_B + |B|) |Sigma| |G|^T + |G| |Sigma| |G|^T
  rel             |J| M_joint |J|^T + |J| |Sigma_joint| |J|^T, J the mp-differenced Jacobian of T_c T_o (not the adjoint formula)
  fixed camera    nothing is inverted: cam_cov, fixed_map_cov and cross are zeros exactly; rel has the product's own rounding only
Every case prints its worst error / tolerance ratio."""
import ctypes as C

import numpy as np
import pytest

from suo_slam_amd import _lib, ba
from tests import pose_cov_cases as K
from tests import pose_cov_mp_ref as MP
from tests import track_cov_cases as TC

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
KEYS = ("cam_cov", "fixed_map_cov", "cross", "rel")


def _same_bits(x, y):
    return all(np.array_equal(x[k], y[k], equal_nan=True) for k in KEYS + ("status",))


BUF = {"cam_cov": "track_cam", "fixed_map_cov": "fixed_map", "cross": "track_cross", "rel": "track_rel"}


def _check(g, Sigma, got, ref, what, objects=None):
    """every block of every camera against the reference (pose_cov_mp_ref.tracking) to its tolerance (objects: only those objects' cross / rel blocks); NaN exactly
    where the reference has it; cam_cov and rel exactly symmetric; returns the worst error / tolerance ratio per output"""
    O = len(g["obj_T"])
    objects = range(O) if objects is None else objects
    worst = dict.fromkeys(KEYS, 0.0)
    for c in range(len(g["cam_T"])):
        if g["cam_fixed"][c]:
            assert not got["cam_cov"][c].any() and not got["fixed_map_cov"][c].any() and not np.nan_to_num(got["cross"][c]).any(), (what, c, "fixed camera: zeros")
        for k in ("cam_cov", "fixed_map_cov"):
            if np.isnan(getattr(ref, k)[c]).any():
                assert np.isnan(got[k][c]).all(), (what, c, k)
                continue
            r = MP.ratio(got[k][c], getattr(ref, k)[c], getattr(ref, "M_" + k)[c]) / MP.K[BUF[k]]
            worst[k] = max(worst[k], r)
            assert r <= 1.0, (what, c, k, r)
        assert np.array_equal(got["cam_cov"][c], got["cam_cov"][c].T, equal_nan=True), (what, c, "cam_cov is exactly symmetric")
        for o in objects:
            for k in ("cross", "rel"):
                if np.isnan(getattr(ref, k)[c, o]).any():
                    assert np.isnan(got[k][c, o]).all(), (what, c, o, k)
                    continue
                r = MP.ratio(got[k][c, o], getattr(ref, k)[c, o], getattr(ref, "M_" + k)[c, o]) / MP.K[BUF[k]]
                worst[k] = max(worst[k], r)
                assert r <= 1.0, (what, c, o, k, r)
            assert np.array_equal(got["rel"][c, o], got["rel"][c, o].T, equal_nan=True), (what, c, o, "rel is exactly symmetric")
    print(f"track_cov {what}: error / tolerance: " + "  ".join(f"{k} {worst[k]:.4f}" for k in KEYS))
    return worst


@pytest.mark.parametrize("n_obj", sorted(TC.SIZES))
def test_blocks_meet_the_tolerances_and_the_fixed_map_block_keeps_its_bits(n_obj):
    g, Sigma, _ = TC.case(n_obj)
    ref = MP.track_case(n_obj)
    before = {k: v.copy() for k, v in g.items()}
    got = ba.tracking_covariances(*K.args(g), map_cov=Sigma)
    _check(g, Sigma, got, ref, f"{n_obj} objects")
    assert list(got["status"]) == list(ref.status) == [1, 0]
    assert np.isnan(got["cam_cov"][2]).all() and np.isnan(got["cross"][2]).all() and np.isnan(got["rel"][2]).all(), "a free camera without a counted edge"
    if n_obj >= 2:
        assert not (g["edge_obj"][g["edge_cam"] == 0] == n_obj - 1).any() and np.abs(got["cross"][0, n_obj - 1]).max() > 0, "cross is dense over the objects"
    marg = ba.pose_covariances(*K.args(g))
    assert np.array_equal(got["fixed_map_cov"], marg[0], equal_nan=True), "fixed_map_cov is suo_pose_covariances' camera block, bit for bit"
    assert _same_bits(got, ba.tracking_covariances(*K.args(g), map_cov=Sigma)), "two calls give the same bits"
    assert all(np.array_equal(g[k], before[k]) for k in g), "the problem is not modified"


def test_a_certain_map_gives_the_fixed_map_covariance_and_no_cross_block():
    for n_obj in (2, 17):
        g, Sigma, _ = TC.case(n_obj)
        got = ba.tracking_covariances(*K.args(g), map_cov=np.zeros_like(Sigma))
        assert np.array_equal(got["cam_cov"], got["fixed_map_cov"], equal_nan=True)
        assert not got["cross"][:2].any() and np.isnan(got["cross"][2]).all()
        assert np.array_equal(got["rel"][0], np.broadcast_to(got["cam_cov"][0], got["rel"][0].shape)), "rel of a certain object is the camera's block"


def test_only_the_upper_triangle_of_the_map_covariance_is_read():
    for n_obj in (2, 17):
        g, Sigma, _ = TC.case(n_obj)
        low = Sigma.copy()
        low[np.tril_indices(len(low), -1)] = np.random.default_rng(1).normal(0, 1e3, len(np.tril_indices(len(low), -1)[0]))
        low[-1, 0] = np.nan
        assert _same_bits(ba.tracking_covariances(*K.args(g), map_cov=low), ba.tracking_covariances(*K.args(g), map_cov=Sigma))


def test_an_object_marked_nan_is_left_out_of_the_map():
    g, Sigma, _ = TC.case(16)
    seen = sorted(set(g["edge_obj"][(g["edge_cam"] == 0) & (g["edge_inlier"] == 1)]))
    o = int(seen[1])
    marked = Sigma.copy()
    marked[6 * o:6 * o + 6, :] = np.nan
    marked[:, 6 * o:6 * o + 6] = np.nan
    got = ba.tracking_covariances(*K.args(g), map_cov=marked)
    assert list(got["status"]) == [1, 1]
    assert np.isnan(got["cross"][:, o]).all() and np.isnan(got["rel"][:, o]).all()
    # the restatement WITHOUT that object's edges, the object certain (zero rows and columns) instead of marked
    without = dict(g, edge_inlier=np.where(g["edge_obj"] == o, 0, g["edge_inlier"]).astype(np.uint8))
    zeroed = np.nan_to_num(marked, nan=0.0)
    others = [j for j in range(16) if j != o]
    _check(without, zeroed, got, MP.tracking(without, zeroed), f"16 objects, object {o} not in the map", objects=others)
    # only its (0, 0) entry decides
    corner = Sigma.copy()
    corner[6 * o, 6 * o] = np.nan
    assert _same_bits(got, ba.tracking_covariances(*K.args(g), map_cov=corner))


def test_a_batch_gives_every_problem_the_bits_it_gets_alone():
    cases = [TC.case(n)[:2] for n in (1, 17, 64)]
    problems = [ba.Problem(*K.args(g)) for g, _ in cases]
    batch = ba.tracking_covariances_batch(problems, [S for _, S in cases])
    for (g, S), b in zip(cases, batch):
        assert _same_bits(b, ba.tracking_covariances(*K.args(g), map_cov=S))
    again = ba.tracking_covariances_batch(problems[::-1], [S for _, S in cases][::-1])[::-1]
    assert all(_same_bits(a, b) for a, b in zip(batch, again))


def test_every_output_pointer_may_be_null():
    g, Sigma, _ = TC.case(2)
    p = ba.Problem(*K.args(g))
    s = _lib.BaProblem()
    p._fill(s)
    status = np.full(2, -1, np.int32)
    lib = _lib.lib()
    _lib.check(lib.suo_tracking_covariances(C.byref(s), Sigma.ctypes.data, None, None, None, None, status.ctypes.data), "suo_tracking_covariances")
    assert list(status) == [1, 0]
    _lib.check(lib.suo_tracking_covariances(C.byref(s), Sigma.ctypes.data, None, None, None, None, None), "suo_tracking_covariances")


def test_a_free_object_or_more_objects_than_the_cap_are_refused():
    g, Sigma, _ = TC.case(2)
    g["obj_fixed"][1] = 0
    with pytest.raises(_lib.SuoError, match=r"code 1\).*object 1 of problem 0 is free"):
        ba.tracking_covariances(*K.args(g), map_cov=Sigma)
    g, Sigma, _ = TC.case(64)
    g["obj_T"] = np.concatenate([g["obj_T"], g["obj_T"][:1]])
    g["obj_fixed"] = np.ones(65, np.uint8)
    with pytest.raises(_lib.SuoError, match=r"code 1\).*65 objects.*at most 64"):
        ba.tracking_covariances(*K.args(g), map_cov=np.zeros((390, 390)))


def test_monte_carlo_on_the_device_has_the_consider_covariance():
    """The 4096 problems of the CPU pin (tests/test_track_cov_ref.py) through ba.optimize_batch in one call; the same two gates."""
    g = TC.mc_setup()["g"]
    obj_T, d_obj, uv = TC.mc_draws()
    problems = [ba.Problem(*K.args(dict(g, obj_T=obj_T[n], edge_uv=uv[n])), **TC.OPT_KW) for n in range(TC.MC_N)]
    ba.optimize_batch(problems)
    m = TC.mc_gates(TC.mc_errors(np.stack([p.cam_T.reshape(3, 4) for p in problems])), d_obj)
    print("device LM, whitened by P_c:", m["eig_consider"], "gate", TC.MC_GATE, " by Hcc^-1:", m["eig_fixed_map"], " cross", m["cross_err"], m["cross_err_flipped"])
    assert TC.MC_GATE[0] <= m["eig_consider"].min() and m["eig_consider"].max() <= TC.MC_GATE[1]
    assert m["eig_fixed_map"].min() >= 2.0
    # and the entry agrees with the restatement the gates are stated in
    s = TC.mc_setup()
    _check(g, s["Sigma"], ba.tracking_covariances(*K.args(g), map_cov=s["Sigma"]), MP.tracking(g, s["Sigma"]), "Monte-Carlo set-up")


def _run_slam(state_dict, n_views, n_obj, max_crops):
    from suo_slam_amd import synthetic as S
    from suo_slam_amd.object_slam import ObjectSLAM
    seq = S.make_slam_sequence(np.random.default_rng(3), n_views, n_obj)
    slam = ObjectSLAM(None, seq["mesh_db"], state_dict=state_dict, max_crops=max_crops, debug_gt_kp=True, manual_kp_std=0.01, run_network_in_debug=True)
    for vw in seq["views"]:
        slam.process_view(vw["view_id"], vw["image"], vw["K"], vw["obj_ids"].copy(), vw["bboxes"].copy(), vw["model_kps"], vw["model_kps_masks"], vw["kp_masks"],
                          uv_gt=vw["uv_gt"])
    return slam


def test_object_slam_reports_the_tracking_covariance_of_a_view_from_a_cached_map_covariance(state_dict):
    slam = _run_slam(state_dict, 3, 6, 16)
    views = list(slam.cam_poses)
    assert len(views) == 3
    poses = {v: np.array(T).copy() for v, T in slam.cam_poses.items()}
    obj_ids, Sigma = slam.map_covariance()
    assert obj_ids == list(slam.obj_poses) and Sigma.shape == (6 * len(obj_ids),) * 2 and np.isfinite(Sigma).all() and np.array_equal(Sigma, Sigma.T)
    out = slam.tracking_covariance(views[-1], map_cov=(obj_ids, Sigma))
    prob, (_, obj_index, _, curr_only, view_curr) = slam.build_problem(curr_only=True)
    assert curr_only and view_curr == views[-1] and len(obj_index) >= 2
    at = np.concatenate([np.arange(6 * obj_ids.index(o), 6 * obj_ids.index(o) + 6) for o in obj_index])
    direct = ba.tracking_covariances_batch([prob], [Sigma[np.ix_(at, at)]])[0]
    assert np.array_equal(out["cam"], direct["cam_cov"][0]) and np.array_equal(out["cam_fixed_map"], direct["fixed_map_cov"][0])
    assert list(out["cross"]) == list(obj_index) == list(out["rel"]) and out["status"] == [0, 0]
    for o, j in obj_index.items():
        assert np.array_equal(out["cross"][o], direct["cross"][0, j]) and np.array_equal(out["rel"][o], direct["rel"][0, j])
    for S6 in [out["cam"], out["cam_fixed_map"]] + list(out["rel"].values()):
        assert S6.shape == (6, 6) and np.isfinite(S6).all() and np.array_equal(S6, S6.T) and (np.diag(S6) > 0).all()
    assert all(np.isfinite(X).all() and X.any() for X in out["cross"].values())
    gain = out["cam"] - out["cam_fixed_map"]
    assert np.linalg.eigvalsh(gain).min() >= -1e-9 * np.linalg.eigvalsh(out["cam"]).max(), "cam - cam_fixed_map is positive semi-definite"
    assert np.trace(gain) > 0
    # the default view is the last one; an earlier view and the map without it (map_cov=None) also answer
    assert np.array_equal(slam.tracking_covariance(map_cov=(obj_ids, Sigma))["cam"], out["cam"])
    mid = slam.tracking_covariance(views[1])
    assert np.isfinite(mid["cam"]).all() and np.linalg.eigvalsh(mid["cam"] - mid["cam_fixed_map"]).min() >= -1e-9 * np.linalg.eigvalsh(mid["cam"]).max()
    # an object the cached map does not hold is left out
    gone = list(obj_index)[0]
    keep = np.concatenate([np.arange(6 * i, 6 * i + 6) for i, o in enumerate(obj_ids) if o != gone])
    part = slam.tracking_covariance(views[-1], map_cov=([o for o in obj_ids if o != gone], Sigma[np.ix_(keep, keep)]))
    assert part["status"] == [0, 1] and np.isnan(part["cross"][gone]).all() and np.isnan(part["rel"][gone]).all() and np.isfinite(part["cam"]).all()
    assert all(np.array_equal(poses[v], slam.cam_poses[v]) for v in poses), "nothing in the map changes"
