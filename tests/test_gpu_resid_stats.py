"""suo_residual_statistics (csrc/resid_stats.hip behind the pose-covariance kernels) against the mp reference of tests/pose_cov_mp_ref.py (CovRef.statistics), on the
graphs of tests/resid_stats_cases.py.

Tolerances, entry by entry, K[buffer] eps M with M the reference's own error scale (its module docstring) and K fixed on the CPU by tests/test_pose_cov_mp_ref.py,
which also shows every one of them at or below the tolerance this module applied before, and that the tolerance of t is finite on every edge whose t is (no edge is
exempt) and wider than 1e-6 max(1, |t|) on at most one counted edge in ten:
  chi2  M_chi2 of tests/ba_phases_ref.py          P_e   (J Sigma) dH (J Sigma)^T through the full rows of Sigma, J's own error, the products' rounding
  lev   sum (M_P + |P|) |Omega|                   t     through the mp inverse of R = I + s P Omega; P = 0 (both vertices fixed): chi2's
  sums  the members' M plus their magnitudes; s0^2: that of sum chi2 over dof, plus |s0^2|
Counts, m, n, dof, status and the NaN pattern are exact.  Observed error-to-tolerance ratios: profiles/resid_stats.txt, and the row of csrc/resid_stats.hip in DESIGN.md's kernel table."""
import numpy as np
import pytest

from suo_slam_amd import ba
from tests import pose_cov_cases as K
from tests import pose_cov_mp_ref as MP
from tests import resid_stats_cases as RK

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
NO_PAIRS = np.zeros((0, 2), np.int32)
ALL_OUT = ba.RESID_KEYS + ("summary", "status")


def _run(g):
    return ba.residual_statistics(*K.args(g))


def _same_bits(x, y, keys=ALL_OUT):
    return all(np.array_equal(x[k], y[k], equal_nan=True) for k in keys)


BUF = {"edge_chi2": "chi2", "edge_pcov": "pcov", "edge_lev": "lev", "edge_t": "t", "cam_stat": "vstat", "obj_stat": "vstat", "summary": "summary"}


def _check(name, g, cr, got):
    """every output against the reference (a CovRef): the NaN pattern, counts and status exactly, the rest to K eps M; returns the worst error / tolerance"""
    st = cr.statistics()
    RK.far_from_the_threshold(name, g, {"det": st.det, "counted": st.counted})
    worst = {}
    for key, buf in BUF.items():
        a, b = got[key], getattr(st, key)
        assert a.shape == b.shape, (name, key)
        assert np.array_equal(np.isnan(a), np.isnan(b)), (name, key, "the NaN pattern is exact")
        worst[key] = MP.ratio(a, b, getattr(st, "M_" + key)) / MP.K[buf]
        assert worst[key] <= 1.0, (name, key, worst[key])
    for key in ("cam_stat", "obj_stat"):
        assert np.array_equal(got[key][:, 0], getattr(st, key)[:, 0]), (name, key, "counts are exact")
    m, n, dof = st.summary[0], st.summary[1], st.summary[4]
    assert list(got["summary"][[0, 1, 4]]) == [m, n, dof], (name, got["summary"], "m, n and dof are exact")
    assert list(got["status"]) == list(st.status), (name, got["status"], st.status)
    # sum lev = n on the device alone, and 0 <= lev <= 2 on a counted edge
    k = np.flatnonzero(st.counted)
    if len(k) and not np.isnan(st.summary[3]):
        alone = MP.tol("summary", st.M_summary[3])
        worst["sum lev - n"] = abs(got["summary"][3] - n) / alone
        assert abs(got["summary"][3] - n) <= alone, (name, got["summary"][3], n, alone)
        t_lev = MP.tol("lev", st.M_edge_lev[k])
        assert (got["edge_lev"][k] >= -t_lev).all() and (got["edge_lev"][k] <= 2 + t_lev).all(), (name, "0 <= lev <= 2 on a counted edge")
    print(f"resid_stats {name}: E {len(g['edge_cam'])}  m {int(m)}  n {int(n)}  s0^2 {got['summary'][5]:.4f}  error / tolerance: "
          + "  ".join(f"{key} {val:.2e}" for key, val in worst.items()))
    return worst


@pytest.mark.parametrize("name", RK.NAMES)
def test_every_output_meets_the_derived_tolerance_and_two_calls_give_the_same_bits(name):
    g = MP.graph(name)
    got = _run(g)
    _check(name, g, MP.case(name), got)
    # the covariances are the graph entry's on the same problem, bit for bit
    cam, obj, _, _, status = ba.pose_covariances_graph(*K.args(g), pairs=NO_PAIRS)
    assert np.array_equal(got["cam_cov"], cam, equal_nan=True) and np.array_equal(got["obj_cov"], obj, equal_nan=True) and list(got["status"][:2]) == list(status[:2])
    assert _same_bits(got, _run(g)), "two calls give the same bits"


def test_the_designed_graphs_take_the_paths_they_were_designed_for():
    g = MP.graph("three_edges")
    got = _run(g)
    cut = RK.designed("three_edges", g)
    assert np.isnan(got["edge_t"][cut]).all() and np.isfinite(got["edge_lev"][cut]).all() and np.isfinite(got["edge_pcov"][cut]).all() and got["status"][3] == 3
    g = MP.graph("fixed_pair_3x2")
    got = _run(g)
    both = (g["edge_cam"] == 0) & (g["edge_obj"] == 1)
    assert both.sum() >= 4 and not got["edge_pcov"][both].any() and not got["edge_lev"][both].any()
    assert np.array_equal(got["edge_t"][both], got["edge_chi2"][both]), "P = 0: t is chi2 to the bit"
    g = MP.graph("no_edges")
    got = _run(g)
    assert np.array_equal(got["summary"][:5], np.zeros(5)) and np.isnan(got["summary"][5]) and list(got["status"]) == [0, 2, 0, 0]
    assert not got["cam_stat"].any() and not got["obj_stat"].any() and got["edge_chi2"].shape == (0,) and np.isnan(got["obj_cov"]).all() and not got["cam_cov"].any()


def test_every_problem_of_a_batch_of_all_cases_equals_its_solo_bits():
    graphs = [MP.graph(n) for n in RK.NAMES]
    solo = [_run(g) for g in graphs]
    batch = ba.residual_statistics_batch([ba.Problem(*K.args(g)) for g in graphs])
    for n, a, b in zip(RK.NAMES, batch, solo):
        assert _same_bits(a, b), n
    # the other order, so that no member's grid position is the one it has alone
    back = ba.residual_statistics_batch([ba.Problem(*K.args(g)) for g in graphs[::-1]])
    for n, a, b in zip(RK.NAMES, back[::-1], solo):
        assert _same_bits(a, b), n


@pytest.mark.parametrize("name", ["1x17", "cam_only", "flagged_3x2", "three_edges", "object_out_3x17m", "6x20m"])
def test_four_times_the_information_scales_every_output_by_a_power_of_two_exactly(name):
    g = MP.graph(name)
    one = _run(g)
    g["edge_info"] = 4.0 * g["edge_info"]
    four = _run(g)
    assert np.array_equal(four["edge_lev"], one["edge_lev"], equal_nan=True) and np.array_equal(four["status"], one["status"])
    assert np.array_equal(4.0 * four["edge_pcov"], one["edge_pcov"], equal_nan=True)
    assert np.array_equal(4.0 * four["cam_cov"], one["cam_cov"], equal_nan=True) and np.array_equal(4.0 * four["obj_cov"], one["obj_cov"], equal_nan=True)
    for key in ("edge_chi2", "edge_t"):
        assert np.array_equal(four[key], 4.0 * one[key], equal_nan=True), key
    for key in ("cam_stat", "obj_stat"):
        assert np.array_equal(four[key][:, 0], one[key][:, 0]) and np.array_equal(four[key][:, 1], 4.0 * one[key][:, 1]), key
        assert np.array_equal(four[key][:, 2], one[key][:, 2]), (key, "redundancies do not scale")
    scale = np.array([1, 1, 4, 1, 1, 4.0])
    assert np.array_equal(four["summary"], scale * one["summary"], equal_nan=True)


def test_statistics_after_optimize_leave_the_problem_unchanged():
    g = MP.graph("3x2")
    p = ba.Problem(*K.args(g), its=(10, 10), init_with_outliers=True)
    ba.optimize_batch([p])
    fields = ("cam_T", "obj_T", "cam_fixed", "obj_fixed", "edge_cam", "edge_obj", "edge_camk", "edge_p", "edge_uv", "edge_info", "inlier", "chi2", "stats")
    before = {k: getattr(p, k).copy() for k in fields}
    got = ba.residual_statistics_batch([p])[0]
    for k in fields:
        assert np.array_equal(getattr(p, k), before[k]), k
    state = dict(g, cam_T=p.cam_T.reshape(-1, 3, 4), obj_T=p.obj_T.reshape(-1, 3, 4), edge_inlier=p.inlier)
    _check("3x2 after optimize", state, MP.CovRef(state), got)
    assert got["summary"][4] > 0 and np.isfinite(got["summary"][5]) and got["summary"][5] > 0, got["summary"]


def _run_slam(state_dict, n_views, n_obj, max_crops):
    from suo_slam_amd import synthetic as S
    from suo_slam_amd.object_slam import ObjectSLAM
    seq = S.make_slam_sequence(np.random.default_rng(3), n_views, n_obj)
    slam = ObjectSLAM(None, seq["mesh_db"], state_dict=state_dict, max_crops=max_crops, debug_gt_kp=True, manual_kp_std=0.01, run_network_in_debug=True)
    for vw in seq["views"]:
        slam.process_view(vw["view_id"], vw["image"], vw["K"], vw["obj_ids"].copy(), vw["bboxes"].copy(), vw["model_kps"], vw["model_kps_masks"], vw["kp_masks"],
                          uv_gt=vw["uv_gt"])
    return slam


def test_object_slam_reports_residual_statistics_and_scales_its_covariances(state_dict):
    slam = _run_slam(state_dict, 3, 6, 16)
    views = list(slam.cam_poses)
    poses_before = {v: np.array(T, copy=True) for v, T in slam.cam_poses.items()}, {o: np.array(T, copy=True) for o, T in slam.obj_poses.items()}
    inl_before = {(v, o): np.array(d["inliers"], copy=True) for v, det in slam.detections.items() for o, d in det.items()}
    rs = slam.residual_statistics()
    assert set(rs) == {"summary", "cams", "objs", "edges"}
    assert list(rs["cams"]) == views and list(rs["objs"]) == list(slam.obj_poses)
    prob, (cam_index, obj_index, e_ref, _, _) = slam.build_problem(False)
    assert list(rs["edges"]) == [(v, o) for v, o, _, _ in e_ref.segs]
    direct = ba.residual_statistics_batch([prob])[0]
    for (v, o, first, n) in e_ref.segs:
        e = rs["edges"][(v, o)]
        assert set(e) == {"chi2", "leverage", "t"} and all(len(e[k]) == n == len(slam.detections[v][o]["inliers"]) for k in e)
        assert np.array_equal(e["chi2"], direct["edge_chi2"][first:first + n]) and np.array_equal(e["t"], direct["edge_t"][first:first + n], equal_nan=True)
    s = rs["summary"]
    assert s["m"] == int(np.asarray(prob.inlier).sum()) and s["n"] == 6 * (len(views) - 1 + len(obj_index)) and s["dof"] == 2 * s["m"] - s["n"] > 0
    assert s["s0_sq"] == s["chi2"] / s["dof"] and abs(s["leverage"] - s["n"]) < 1e-6 * s["n"] and s["status"] == [0, 0, 0, 0]
    assert sum(c[0] for c in rs["cams"].values()) == s["m"] == sum(o[0] for o in rs["objs"].values())
    sub = slam.residual_statistics(view_ids=views[1:])
    assert list(sub["cams"]) == views[1:] and all(k[0] in views[1:] for k in sub["edges"]) and sub["summary"] == s
    # nothing in the map changed
    for v in views:
        assert np.array_equal(slam.cam_poses[v], poses_before[0][v])
    for o in slam.obj_poses:
        assert np.array_equal(slam.obj_poses[o], poses_before[1][o])
    for (v, o), inl in inl_before.items():
        assert np.array_equal(slam.detections[v][o]["inliers"], inl)
    # the unscaled covariances: the bits of the graph entry on the same problem, as before; scaled = variance_factor x unscaled
    plain = slam.pose_covariances(relative=True, trajectory=True)
    assert "variance_factor" not in plain
    keys = [(v, o) for v in views for o in obj_index]
    pairs = [(cam_index[v], len(cam_index) + obj_index[o]) for v, o in keys] + [(cam_index[a], cam_index[b]) for a, b in zip(views[:-1], views[1:])]
    cam_cov, obj_cov, _, rel_cov, _ = ba.pose_covariances_graph_batch([prob], [np.array(pairs, np.int32)])[0]
    for v, i in cam_index.items():
        assert np.array_equal(plain["cams"][v], cam_cov[i])
    for o, j in obj_index.items():
        assert np.array_equal(plain["objs"][o], obj_cov[j])
    assert list(plain["rel"]) == keys and list(plain["rel_cams"]) == list(zip(views[:-1], views[1:]))
    for S6, mine in zip(rel_cov, list(plain["rel"].values()) + list(plain["rel_cams"].values())):
        assert np.array_equal(mine, S6)
    scaled = slam.pose_covariances(relative=True, trajectory=True, scaled=True)
    f = scaled["variance_factor"]
    assert f == s["s0_sq"] and set(scaled) == set(plain) | {"variance_factor"}
    for group in plain:
        assert list(scaled[group]) == list(plain[group])
        for k in plain[group]:
            assert np.array_equal(scaled[group][k], f * plain[group][k], equal_nan=True), (group, k)
