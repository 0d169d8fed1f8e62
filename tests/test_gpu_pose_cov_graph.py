"""suo_pose_covariances_graph (csrc/pose_cov_graph.hip: the coupled form with the reduced system in device memory, and (camera, camera) pairs) against the mp
reference of tests/pose_cov_mp_ref.py, on the graphs of tests/pose_cov_graph_cases.py and the graphs the old entries serve.

Tolerances, entry by entry, K eps M with K fixed on the CPU by tests/test_pose_cov_mp_ref.py (which also shows each below the old tolerance everywhere):
  marginal and cross blocks      M = the block of M_Sigma = |Sigma| MH |Sigma| + |Sigma| sqrt(diag H (x) diag H) |Sigma|
  rel of every kind of pair      M = |J| M_joint |J|^T + |J| |Sigma_joint| |J|^T, J the mp-differenced Jacobian of the relative pose; M == 0 is an exact zero
Observed error-to-tolerance ratios: profiles/pose_cov_graph.txt."""
import numpy as np
import pytest

from suo_slam_amd import _lib, ba
from tests import pose_cov_cases as K
from tests import pose_cov_graph_cases as GK
from tests import pose_cov_mp_ref as MP
from tests import pose_cov_pair_cases as PK

pytestmark = pytest.mark.gpu

CAP = 64


def _check_blocks(got, cr, what):
    """every marginal block against the reference (a CovRef) to the tolerance; NaN / zero blocks exactly where the reference has them; symmetric to the tolerance,
    positive diagonal"""
    worst = MP.check_blocks(got[0], got[1], got[-1][:2], cr, what)
    print(f"pose_cov_graph {what}: n {cr.n}  max M {cr.M_Sigma.max():.3e}  marginal error / tolerance {worst:.4f}")


def _check_pairs(g, pairs, got, cr, what):
    """every pair against the reference to its tolerance; NaN blocks exactly where the reference has them and status[2] counting them; rel symmetric with a positive
    diagonal; 36 zeros for two fixed vertices and for the rel of (c, c), whose cross is the marginal block; no cross block with a fixed vertex"""
    cam, obj, cross, rel, status = got
    worst, pr = MP.check_pairs(pairs, cross, rel, status[2], cr, what)
    nc = len(g["cam_T"])
    fixed = np.r_[g["cam_fixed"], g["obj_fixed"]].astype(bool)
    for q, (a, b) in enumerate(pairs):
        if np.isnan(pr.rel[q]).any():
            continue
        if a == b and a < nc:
            assert not rel[q].any() and np.array_equal(cross[q], cam[a]), (what, q, "(c, c): the marginal block and a relative pose that cannot move")
        elif fixed[a] and fixed[b]:
            assert not rel[q].any() and not cross[q].any(), (what, q, "two fixed vertices: 36 zeros")
        else:
            assert (np.diag(rel[q]) > 0).all(), (what, q, a, b)
        if (fixed[a] or fixed[b]) and a != b:
            assert not cross[q].any(), (what, q, "a fixed vertex has no cross block")
    assert list(status[:2]) == list(cr.marginals().status), (what, status)
    print(f"pose_cov_graph {what}: error / tolerance: cross {worst['cross']:.4f}  rel cam-obj {worst['cam-obj']:.4f}  rel obj-obj {worst['obj-obj']:.4f}"
          f"  rel cam-cam {worst['cam-cam']:.4f}")
    return pr


def _transposes_to_the_bit(pairs, cross, what):
    where = {(int(a), int(b)): q for q, (a, b) in enumerate(pairs)}
    n = 0
    for (a, b), q in where.items():
        if a != b and (b, a) in where:
            assert np.array_equal(cross[q], cross[where[(b, a)]].T, equal_nan=True), (what, a, b)
            n += 1
    return n


def _same_bits(x, y):
    return all(np.array_equal(a, b, equal_nan=True) for a, b in zip(x, y))


NO_PAIRS = np.zeros((0, 2), np.int32)


@pytest.mark.parametrize("name", GK.NAMES)
def test_large_maps_meet_the_bound_and_two_calls_give_the_same_bits(name):
    g, ref = MP.graph(name), MP.case(name)
    got = ba.pose_covariances_graph(*K.args(g), pairs=NO_PAIRS)
    _check_blocks(got, ref, name)
    assert list(got[4]) == list(ref.marginals().status) + [0]
    assert _same_bits(got, ba.pose_covariances_graph(*K.args(g), pairs=NO_PAIRS)), "two calls give the same bits"


@pytest.mark.parametrize("name", GK.NAMES)
def test_pairs_of_large_maps_meet_the_tolerances(name):
    g, ref = MP.graph(name), MP.case(name)
    pairs = GK.pairs_of(g)
    C = len(g["cam_T"])
    assert (C + 15, C + 16) in {tuple(p) for p in pairs.tolist()} and (0, 0) in {tuple(p) for p in pairs.tolist()}
    got = ba.pose_covariances_graph(*K.args(g), pairs=pairs)
    _check_blocks(got, ref, name + " with pairs")
    ref_pairs = _check_pairs(g, pairs, got, ref, name)
    assert _transposes_to_the_bit(pairs, got[2], name) >= C * (C - 1) // 2 + 3
    un = GK.unseen_pair(g)
    if un is not None:                                     # dense over the objects: also where the camera does not see the object
        q = un[0] * len(g["obj_T"]) + un[1]
        assert tuple(pairs[q]) == (un[0], C + un[1]) and np.abs(got[2][q]).max() > 0 and np.abs(ref_pairs.cross[q]).max() > 0
    assert _same_bits(got, ba.pose_covariances_graph(*K.args(g), pairs=pairs)), "two calls give the same bits"


@pytest.mark.parametrize("name", ["3x2", "5x16", "moved_cam_only"])
def test_camera_pairs_on_graphs_the_old_entry_serves(name):
    g, ref = MP.graph(name), MP.case(name)
    pairs = np.array(GK.camera_pairs(g), np.int32)
    got = ba.pose_covariances_graph(*K.args(g), pairs=pairs)
    _check_blocks(got, ref, name + " with camera pairs")
    _check_pairs(g, pairs, got, ref, name + " camera pairs")
    _transposes_to_the_bit(pairs, got[2], name)
    old = ba.pose_covariances(*K.args(g))
    mg = ref.marginals()
    assert (np.abs(got[0] - old[0]) <= 2 * MP.tol("sigma", mg.M_cam)).all() and (np.abs(got[1] - old[1]) <= 2 * MP.tol("sigma", mg.M_obj)).all()
    assert list(got[4][:2]) == list(old[2])
    if name == "moved_cam_only":                           # no free object: the kernels of the old entry, one camera with itself
        assert _same_bits(got[:2], old[:2]) and np.array_equal(got[2][0], got[0][0]) and not got[3][0].any()
    else:                                                  # two free cameras share objects: their cross block is not zero
        assert np.abs(got[2][pairs.tolist().index([1, 2])]).max() > 0


def test_without_a_free_object_two_cameras_have_no_cross_block_and_rel_comes_from_the_marginal_blocks():
    rng = np.random.default_rng(51)
    g = K._graph(rng, K._arc(rng, 3), [1, 0, 0], 2, lambda c, o: True, (4, 4), obj_fixed=[1, 1])      # camera tracking: two free cameras, every object fixed
    pairs = np.array(GK.camera_pairs(g), np.int32)
    ref = MP.CovRef(g)
    got = ba.pose_covariances_graph(*K.args(g), pairs=pairs)
    _check_blocks(got, ref, "3 cameras, no free object")
    _check_pairs(g, pairs, got, ref, "3 cameras, no free object")
    _transposes_to_the_bit(pairs, got[2], "3 cameras, no free object")
    assert _same_bits(got[:2], ba.pose_covariances(*K.args(g))[:2])
    for q, (a, b) in enumerate(pairs):
        assert a == b or not got[2][q].any(), (a, b)
    assert np.array_equal(got[3][pairs.tolist().index([0, 1])], got[0][1]), "(gauge, c): Sigma_cc"


@pytest.mark.parametrize("name", ["3x2", "5x16", "moved_1x17", "moved_cam_only", "1x33"])
def test_without_a_camera_pair_every_output_is_the_pair_entrys_bit_for_bit(name):
    g = MP.graph(name)
    pairs = PK.pairs_of(g, PK.OBJ_PAIRS.get(name, [(0, 1)])) if name in PK.CASES else PK.pairs_of(g, [(0, 1), (3, 32)])
    old = ba.pose_covariances_pairs(*K.args(g), pairs=pairs)
    new = ba.pose_covariances_graph(*K.args(g), pairs=pairs)
    assert len(old) == len(new) == 5
    for x, y in zip(old, new):
        assert np.array_equal(x, y, equal_nan=True), name


def test_every_problem_of_a_batch_that_mixes_the_four_forms_equals_its_solo_bits():
    graphs = {n: MP.graph(n) for n in ("1x9", "cam_only", "5x16", "3x17m", "2x32")}
    lists = {"1x9": PK.pairs_of(graphs["1x9"]), "cam_only": np.array([(0, 1), (0, 0), (1, 2)], np.int32), "5x16": PK.pairs_of(graphs["5x16"], [(0, 15)]),
             "3x17m": GK.pairs_of(graphs["3x17m"]), "2x32": GK.pairs_of(graphs["2x32"])}
    names = list(graphs)
    batch = ba.pose_covariances_graph_batch([ba.Problem(*K.args(graphs[n])) for n in names], [lists[n] for n in names])
    for n, got in zip(names, batch):
        assert _same_bits(got, ba.pose_covariances_graph(*K.args(graphs[n]), pairs=lists[n])), n
    # form 2 kept its kernels inside the mixed batch
    assert _same_bits(batch[2], ba.pose_covariances_pairs(*K.args(graphs["5x16"]), pairs=lists["5x16"]))
    # the other order, so that no member's grid position is the one it has alone
    back = ba.pose_covariances_graph_batch([ba.Problem(*K.args(graphs[n])) for n in names[::-1]], [lists[n] for n in names[::-1]])
    for x, y in zip(batch, back[::-1]):
        assert _same_bits(x, y)


def test_an_object_without_a_counted_edge_nans_its_pairs_and_the_others_meet_the_bound():
    g = MP.graph("3x17m")
    g["edge_inlier"][g["edge_obj"] == 16] = 0
    pairs = GK.pairs_of(g)
    ref = MP.CovRef(g)
    hit = np.array([3 + 16 in (a, b) for a, b in pairs])
    assert list(ref.marginals().status) == [0, 1] and ref.pairs(pairs).n_nan == hit.sum() >= 3 + 4
    got = ba.pose_covariances_graph(*K.args(g), pairs=pairs)
    assert np.isnan(got[1][16]).all() and np.isnan(got[2][hit]).all() and np.isnan(got[3][hit]).all() and np.isfinite(got[3][~hit]).all() and got[4][2] == hit.sum()
    _check_blocks(got, ref, "3x17m without object 16")
    _check_pairs(g, pairs, got, ref, "3x17m without object 16")


def test_a_fixed_object_is_zeros_without_a_cross_block():
    g = MP.graph("3x17m")
    g["obj_fixed"][16] = 1
    pairs = GK.pairs_of(g)
    ref = MP.CovRef(g)
    got = ba.pose_covariances_graph(*K.args(g), pairs=pairs)
    assert not got[1][16].any()
    for q, (a, b) in enumerate(pairs):
        if 3 + 16 in (a, b):
            assert not got[2][q].any(), (a, b)
    _check_blocks(got, ref, "3x17m with object 16 fixed")
    _check_pairs(g, pairs, got, ref, "3x17m with object 16 fixed")


def test_a_free_camera_without_a_counted_edge_nans_its_blocks_and_its_pairs():
    g = MP.graph("3x17m")
    g["edge_inlier"][g["edge_cam"] == 1] = 0
    pairs = GK.pairs_of(g)
    ref = MP.CovRef(g)
    hit = np.array([1 in (a, b) for a, b in pairs])
    assert list(ref.marginals().status) == [1, 0] and ref.pairs(pairs).n_nan == hit.sum()
    got = ba.pose_covariances_graph(*K.args(g), pairs=pairs)
    assert np.isnan(got[0][1]).all() and np.isnan(got[2][hit]).all() and np.isnan(got[3][hit]).all() and np.isfinite(got[3][~hit]).all()
    assert list(got[4]) == [1, 0, int(hit.sum())]
    _check_blocks(got, ref, "3x17m without camera 1")
    _check_pairs(g, pairs, got, ref, "3x17m without camera 1")


def test_covariances_after_optimize_leave_the_problem_unchanged():
    g = MP.graph("2x17")
    p = ba.Problem(*K.args(g), its=(10, 10), init_with_outliers=True)        # (the moved poses put every chi2 past the gate: start with all edges in)
    ba.optimize_batch([p])
    assert p.inlier.sum() >= 0.8 * len(p.inlier)
    fields = ("cam_T", "obj_T", "cam_fixed", "obj_fixed", "edge_cam", "edge_obj", "edge_camk", "edge_p", "edge_uv", "edge_info", "inlier", "chi2", "stats")
    before = {k: getattr(p, k).copy() for k in fields}
    pairs = GK.pairs_of(g)
    got = ba.pose_covariances_graph_batch([p], [pairs])[0]
    for k in fields:
        assert np.array_equal(getattr(p, k), before[k]), k
    state = dict(g, cam_T=p.cam_T.reshape(-1, 3, 4), obj_T=p.obj_T.reshape(-1, 3, 4), edge_inlier=p.inlier)
    ref = MP.CovRef(state)
    _check_blocks(got, ref, "2x17 after optimize")
    _check_pairs(state, pairs, got, ref, "2x17 after optimize")


def test_the_cap_is_refused_by_count_and_the_largest_map_below_it_runs():
    over = K.coupled(40, 2, CAP + 1, kp=(4, 4))
    with pytest.raises(_lib.SuoError, match=rf"code 1\).*{CAP + 1} free objects.*at most {CAP}"):
        ba.pose_covariances_graph(*K.args(over), pairs=[(0, 1)])
    g = K.coupled(41, 2, CAP, kp=(4, 4))
    pairs = np.array([(0, 1), (1, 0), (1, 2), (2 + 0, 2 + CAP - 1), (2 + CAP - 1, 2 + 0)], np.int32)
    cam, obj, cross, rel, status = ba.pose_covariances_graph(*K.args(g), pairs=pairs)
    assert list(status) == [0, 0, 0] and not cam[0].any()
    # no accuracy claim beyond n = 200 (the bound's constant is not derived there): finite, symmetric, positive
    for blk in [cam[1]] + list(obj) + [rel[0], rel[2], rel[3]]:
        assert np.isfinite(blk).all() and (np.diag(blk) > 0).all() and np.allclose(blk, blk.T, rtol=1e-9, atol=1e-9 * np.abs(blk).max())
    assert np.array_equal(cross[3], cross[4].T) and np.isfinite(cross).all()


def _run_slam(state_dict, n_views, n_obj, max_crops):
    from suo_slam_amd import synthetic as S
    from suo_slam_amd.object_slam import ObjectSLAM
    seq = S.make_slam_sequence(np.random.default_rng(3), n_views, n_obj)
    slam = ObjectSLAM(None, seq["mesh_db"], state_dict=state_dict, max_crops=max_crops, debug_gt_kp=True, manual_kp_std=0.01, run_network_in_debug=True)
    for vw in seq["views"]:
        slam.process_view(vw["view_id"], vw["image"], vw["K"], vw["obj_ids"].copy(), vw["bboxes"].copy(), vw["model_kps"], vw["model_kps_masks"], vw["kp_masks"],
                          uv_gt=vw["uv_gt"])
    return slam


def test_object_slam_reports_the_covariance_of_the_motion_between_consecutive_views(state_dict):
    slam = _run_slam(state_dict, 3, 6, 16)
    views = list(slam.cam_poses)
    assert len(views) == 3
    assert "rel_cams" not in slam.pose_covariances() and "rel_cams" not in slam.pose_covariances(relative=True)
    out = slam.pose_covariances(trajectory=True)
    assert set(out) == {"cams", "objs", "rel_cams"} and list(out["rel_cams"]) == [(views[0], views[1]), (views[1], views[2])]
    prob, (cam_index, obj_index, _, _, _) = slam.build_problem(False)
    steps = [(cam_index[a], cam_index[b]) for a, b in out["rel_cams"]]
    direct = ba.pose_covariances_graph_batch([prob], [np.array(steps, np.int32)])[0]
    for q, (k, S6) in enumerate(out["rel_cams"].items()):
        assert S6.shape == (6, 6) and np.isfinite(S6).all() and (np.diag(S6) > 0).all() and np.allclose(S6, S6.T, rtol=1e-9, atol=0), k
        assert np.array_equal(S6, direct[3][q]), k
    # the switch of entry changed nothing where the old entries answer
    rel = slam.pose_covariances(relative=True)
    keys = [(v, o) for v in views for o in obj_index]
    pairs = np.array([(cam_index[v], len(cam_index) + obj_index[o]) for v, o in keys], np.int32)
    old = ba.pose_covariances_pairs_batch([prob], [pairs])[0]
    for v, i in cam_index.items():
        assert np.array_equal(rel["cams"][v], old[0][i])
    for o, j in obj_index.items():
        assert np.array_equal(rel["objs"][o], old[1][j])
    for k, S6 in zip(keys, old[3]):
        assert np.array_equal(rel["rel"][k], S6), k
    both = slam.pose_covariances(relative=True, trajectory=True)
    assert list(both["rel"]) == list(rel["rel"]) and list(both["rel_cams"]) == list(out["rel_cams"])
    sub = slam.pose_covariances(view_ids=views[1:], trajectory=True)
    assert list(sub["rel_cams"]) == [(views[1], views[2])]


def test_object_slam_reports_covariances_on_a_map_of_seventeen_objects(state_dict):
    slam = _run_slam(state_dict, 3, 17, 32)
    prob, (cam_index, obj_index, _, _, _) = slam.build_problem(False)
    assert len(cam_index) == 3 and len(obj_index) == 17 and not np.asarray(prob.obj_fixed).any(), "one object more than the old entries take"
    with pytest.raises(_lib.SuoError, match=r"code 1\).*17 free objects"):
        ba.pose_covariances_batch([prob])
    out = slam.pose_covariances(relative=True, trajectory=True)
    views = list(slam.cam_poses)
    assert list(out["rel"]) == [(v, o) for v in views for o in slam.obj_poses] and list(out["rel_cams"]) == [(views[0], views[1]), (views[1], views[2])]
    for k, S6 in list(out["rel"].items()) + list(out["rel_cams"].items()) + list(out["objs"].items()):
        assert S6.shape == (6, 6) and np.isfinite(S6).all() and (np.diag(S6) > 0).all() and np.allclose(S6, S6.T, rtol=1e-9, atol=0), k
    with_cov = slam.collect_results(covariances=True)
    accepted = 0
    for v in with_cov:
        for o, entry in with_cov[v]["poses"].items():
            if entry["T_OtoC"] is None:
                assert entry["cov_OtoC"] is None
            else:
                accepted += 1
                assert np.isfinite(entry["cov_OtoC"]).all() and (np.diag(entry["cov_OtoC"]) > 0).all(), (v, o)
    assert accepted >= 3 * 15
