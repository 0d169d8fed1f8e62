"""suo_pose_covariances_graph (csrc/pose_cov_graph.hip: the coupled form with the reduced system in device memory, and (camera, camera) pairs) against the
finite-difference numpy references of tests/pose_cov_ref.py, tests/pose_cov_pairs_ref.py and tests/pose_cov_graph_ref.py, on the graphs of
tests/pose_cov_graph_cases.py and the graphs the old entries serve.

Tolerances, with b = pose_cov_ref.bound(ref) = 1e3 eps cond(H_ref) max|Sigma_ref| (every input asserts cond <= 1e9 first; the constant is for n <= 200):
  marginal and cross blocks      b
  rel of (camera, object)        b (1 + 6 a)^2, a = max|Ad(T_c)|            (tests/test_gpu_pose_cov_pairs.py)
  rel of (object, object)        4 * 36 * a^2 * b, a = max|Ad(T_b^-1)|      (tests/test_gpu_pose_cov_pairs.py)
  rel of (camera, camera)        b (1 + 6 a)^2, a = max|Ad(T_b T_a^-1)|: Sigma_bb plus 36 products a sigma a plus 2 x 6 products a sigma, as for (camera, object)
Observed error-to-tolerance ratios: profiles/pose_cov_graph.txt."""
import numpy as np
import pytest

from suo_slam_amd import _lib, ba
from tests import pose_cov_cases as K
from tests import pose_cov_graph_cases as GK
from tests import pose_cov_graph_ref as GR
from tests import pose_cov_pair_cases as PK
from tests import pose_cov_pairs_ref as PR
from tests import pose_cov_ref as R

pytestmark = pytest.mark.gpu

CAP = 64


def _rel_tol(g, a, b, bound):
    nc = len(g["cam_T"])
    if a < nc and b < nc:
        amax = np.abs(GR.adjoint(PR.vertex_pose(g, b) @ np.linalg.inv(PR.vertex_pose(g, a)))).max()
        return bound * (1 + 6 * amax) ** 2
    if a < nc or b < nc:
        amax = np.abs(PR.adjoint(PR.vertex_pose(g, min(a, b)))).max()
        return bound * (1 + 6 * amax) ** 2
    amax = np.abs(PR.adjoint(np.linalg.inv(PR.vertex_pose(g, b)))).max()
    return 4 * 36 * amax ** 2 * bound


def _check_blocks(got, ref, what):
    """every marginal block against the reference to the bound; NaN / zero blocks exactly where the reference has them; symmetric to the bound, positive diagonal"""
    assert ref["cond"] <= 1e9, (what, ref["cond"])
    tol = R.bound(ref)
    worst = 0.0
    for name, a, b in (("cam", got[0], ref["cam_cov"]), ("obj", got[1], ref["obj_cov"])):
        assert a.shape == b.shape
        for v in range(len(b)):
            if np.isnan(b[v]).any():
                assert np.isnan(a[v]).all(), (what, name, v)
            elif not b[v].any():
                assert not a[v].any(), (what, name, v, "a fixed vertex is 36 zeros")
            else:
                err = float(np.abs(a[v] - b[v]).max())
                worst = max(worst, err)
                assert err <= tol, (what, name, v, err, tol)
                assert np.abs(a[v] - a[v].T).max() <= tol and (np.diag(a[v]) > 0).all(), (what, name, v)
    assert list(got[-1][:2]) == list(ref["status"]), (what, got[-1], ref["status"])
    print(f"pose_cov_graph {what}: n {ref['H'].shape[0]}  cond {ref['cond']:.3e}  bound {tol:.3e}  marginal error {worst:.3e}  ratio {worst / tol:.4f}")


def _check_pairs(g, pairs, got, ref, ref_pairs, what):
    """every pair against the reference to its tolerance; NaN blocks exactly where the reference has them and status[2] counting them; rel symmetric with a positive
    diagonal; 36 zeros for two fixed vertices and for the rel of (c, c), whose cross is the marginal block; no cross block with a fixed vertex"""
    bound = R.bound(ref)
    cam, obj, cross, rel, status = got
    rcross, rrel, n_nan = ref_pairs
    assert cross.shape == rcross.shape and rel.shape == rrel.shape
    nc = len(g["cam_T"])
    fixed = np.r_[g["cam_fixed"], g["obj_fixed"]].astype(bool)
    worst = {"cross": 0.0, "cam-obj": 0.0, "obj-obj": 0.0, "cam-cam": 0.0}
    for q, (a, b) in enumerate(pairs):
        if np.isnan(rrel[q]).any():
            assert np.isnan(cross[q]).all() and np.isnan(rel[q]).all(), (what, q, a, b)
            continue
        tol = _rel_tol(g, a, b, bound)
        e_cross, e_rel = float(np.abs(cross[q] - rcross[q]).max()), float(np.abs(rel[q] - rrel[q]).max())
        kind = "cam-cam" if max(a, b) < nc else ("cam-obj" if min(a, b) < nc else "obj-obj")
        worst["cross"] = max(worst["cross"], e_cross / bound)
        worst[kind] = max(worst[kind], e_rel / tol)
        assert e_cross <= bound, (what, q, a, b, e_cross, bound)
        assert e_rel <= tol, (what, q, a, b, e_rel, tol)
        assert np.abs(rel[q] - rel[q].T).max() <= tol, (what, q)
        if a == b and a < nc:
            assert not rel[q].any() and np.array_equal(cross[q], cam[a]), (what, q, "(c, c): the marginal block and a relative pose that cannot move")
        elif fixed[a] and fixed[b]:
            assert not rel[q].any() and not cross[q].any(), (what, q, "two fixed vertices: 36 zeros")
        else:
            assert (np.diag(rel[q]) > 0).all(), (what, q, a, b)
        if (fixed[a] or fixed[b]) and a != b:
            assert not cross[q].any(), (what, q, "a fixed vertex has no cross block")
    assert list(status) == list(ref["status"]) + [n_nan], (what, status, ref["status"], n_nan)
    print(f"pose_cov_graph {what}: bound {bound:.3e}  error / tolerance: cross {worst['cross']:.4f}  rel cam-obj {worst['cam-obj']:.4f}  rel obj-obj {worst['obj-obj']:.4f}"
          f"  rel cam-cam {worst['cam-cam']:.4f}")


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
    g, ref = GK.case(name)
    got = ba.pose_covariances_graph(*K.args(g), pairs=NO_PAIRS)
    _check_blocks(got, ref, name)
    assert list(got[4]) == list(ref["status"]) + [0]
    assert _same_bits(got, ba.pose_covariances_graph(*K.args(g), pairs=NO_PAIRS)), "two calls give the same bits"


@pytest.mark.parametrize("name", GK.NAMES)
def test_pairs_of_large_maps_meet_the_tolerances(name):
    g, ref = GK.case(name)
    pairs = GK.pairs_of(g)
    C = len(g["cam_T"])
    assert (C + 15, C + 16) in {tuple(p) for p in pairs.tolist()} and (0, 0) in {tuple(p) for p in pairs.tolist()}
    ref_pairs = GR.relative(g, ref, pairs)
    got = ba.pose_covariances_graph(*K.args(g), pairs=pairs)
    _check_blocks(got, ref, name + " with pairs")
    _check_pairs(g, pairs, got, ref, ref_pairs, name)
    assert _transposes_to_the_bit(pairs, got[2], name) >= C * (C - 1) // 2 + 3
    un = GK.unseen_pair(g)
    if un is not None:                                     # dense over the objects: also where the camera does not see the object
        q = un[0] * len(g["obj_T"]) + un[1]
        assert tuple(pairs[q]) == (un[0], C + un[1]) and np.abs(got[2][q]).max() > 0 and np.abs(ref_pairs[0][q]).max() > 0
    assert _same_bits(got, ba.pose_covariances_graph(*K.args(g), pairs=pairs)), "two calls give the same bits"


@pytest.mark.parametrize("name", ["3x2", "5x16", "moved_cam_only"])
def test_camera_pairs_on_graphs_the_old_entry_serves(name):
    g, _, ref, _ = PK.case(name)
    pairs = np.array(GK.camera_pairs(g), np.int32)
    ref_pairs = GR.relative(g, ref, pairs)
    got = ba.pose_covariances_graph(*K.args(g), pairs=pairs)
    _check_blocks(got, ref, name + " with camera pairs")
    _check_pairs(g, pairs, got, ref, ref_pairs, name + " camera pairs")
    _transposes_to_the_bit(pairs, got[2], name)
    old = ba.pose_covariances(*K.args(g))
    b = R.bound(ref)
    assert np.abs(got[0] - old[0]).max() <= 2 * b and np.abs(got[1] - old[1]).max() <= 2 * b and list(got[4][:2]) == list(old[2])
    if name == "moved_cam_only":                           # no free object: the kernels of the old entry, one camera with itself
        assert _same_bits(got[:2], old[:2]) and np.array_equal(got[2][0], got[0][0]) and not got[3][0].any()
    else:                                                  # two free cameras share objects: their cross block is not zero
        assert np.abs(got[2][pairs.tolist().index([1, 2])]).max() > 0


def test_without_a_free_object_two_cameras_have_no_cross_block_and_rel_comes_from_the_marginal_blocks():
    rng = np.random.default_rng(51)
    g = K._graph(rng, K._arc(rng, 3), [1, 0, 0], 2, lambda c, o: True, (4, 4), obj_fixed=[1, 1])      # camera tracking: two free cameras, every object fixed
    pairs = np.array(GK.camera_pairs(g), np.int32)
    ref = R.covariances(g)
    got = ba.pose_covariances_graph(*K.args(g), pairs=pairs)
    _check_blocks(got, ref, "3 cameras, no free object")
    _check_pairs(g, pairs, got, ref, GR.relative(g, ref, pairs), "3 cameras, no free object")
    _transposes_to_the_bit(pairs, got[2], "3 cameras, no free object")
    assert _same_bits(got[:2], ba.pose_covariances(*K.args(g))[:2])
    for q, (a, b) in enumerate(pairs):
        assert a == b or not got[2][q].any(), (a, b)
    assert np.array_equal(got[3][pairs.tolist().index([0, 1])], got[0][1]), "(gauge, c): Sigma_cc"


@pytest.mark.parametrize("name", ["3x2", "5x16", "moved_1x17", "moved_cam_only", "1x33"])
def test_without_a_camera_pair_every_output_is_the_pair_entrys_bit_for_bit(name):
    if name in PK.CASES:
        g, pairs, _, _ = PK.case(name)
    else:
        g, _ = K.case(name)
        pairs = PK.pairs_of(g, [(0, 1), (3, 32)])
    old = ba.pose_covariances_pairs(*K.args(g), pairs=pairs)
    new = ba.pose_covariances_graph(*K.args(g), pairs=pairs)
    assert len(old) == len(new) == 5
    for x, y in zip(old, new):
        assert np.array_equal(x, y, equal_nan=True), name


def test_every_problem_of_a_batch_that_mixes_the_four_forms_equals_its_solo_bits():
    graphs = {"1x9": K.case("1x9")[0], "cam_only": K.case("cam_only")[0], "5x16": K.case("5x16")[0], "3x17m": GK.case("3x17m")[0], "2x32": GK.case("2x32")[0]}
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
    g, _ = GK.case("3x17m")
    g["edge_inlier"][g["edge_obj"] == 16] = 0
    pairs = GK.pairs_of(g)
    ref = R.covariances(g)
    ref_pairs = GR.relative(g, ref, pairs)
    hit = np.array([3 + 16 in (a, b) for a, b in pairs])
    assert list(ref["status"]) == [0, 1] and ref_pairs[2] == hit.sum() >= 3 + 4
    got = ba.pose_covariances_graph(*K.args(g), pairs=pairs)
    assert np.isnan(got[1][16]).all() and np.isnan(got[2][hit]).all() and np.isnan(got[3][hit]).all() and np.isfinite(got[3][~hit]).all() and got[4][2] == hit.sum()
    _check_blocks(got, ref, "3x17m without object 16")
    _check_pairs(g, pairs, got, ref, ref_pairs, "3x17m without object 16")


def test_a_fixed_object_is_zeros_without_a_cross_block():
    g, _ = GK.case("3x17m")
    g["obj_fixed"][16] = 1
    pairs = GK.pairs_of(g)
    ref = R.covariances(g)
    ref_pairs = GR.relative(g, ref, pairs)
    got = ba.pose_covariances_graph(*K.args(g), pairs=pairs)
    assert not got[1][16].any()
    for q, (a, b) in enumerate(pairs):
        if 3 + 16 in (a, b):
            assert not got[2][q].any(), (a, b)
    _check_blocks(got, ref, "3x17m with object 16 fixed")
    _check_pairs(g, pairs, got, ref, ref_pairs, "3x17m with object 16 fixed")


def test_a_free_camera_without_a_counted_edge_nans_its_blocks_and_its_pairs():
    g, _ = GK.case("3x17m")
    g["edge_inlier"][g["edge_cam"] == 1] = 0
    pairs = GK.pairs_of(g)
    ref = R.covariances(g)
    ref_pairs = GR.relative(g, ref, pairs)
    hit = np.array([1 in (a, b) for a, b in pairs])
    assert list(ref["status"]) == [1, 0] and ref_pairs[2] == hit.sum()
    got = ba.pose_covariances_graph(*K.args(g), pairs=pairs)
    assert np.isnan(got[0][1]).all() and np.isnan(got[2][hit]).all() and np.isnan(got[3][hit]).all() and np.isfinite(got[3][~hit]).all()
    assert list(got[4]) == [1, 0, int(hit.sum())]
    _check_blocks(got, ref, "3x17m without camera 1")
    _check_pairs(g, pairs, got, ref, ref_pairs, "3x17m without camera 1")


def test_covariances_after_optimize_leave_the_problem_unchanged():
    g, _ = GK.case("2x17")
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
    ref = R.covariances(state)
    _check_blocks(got, ref, "2x17 after optimize")
    _check_pairs(state, pairs, got, ref, GR.relative(state, ref, pairs), "2x17 after optimize")


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
