"""Cross blocks and relative-pose covariances of vertex pairs (csrc/pose_cov.hip through suo_pose_covariances_pairs) against the mp reference of
tests/pose_cov_mp_ref.py, on the graphs of tests/pose_cov_pair_cases.py.

Tolerances, entry by entry, K eps M with K fixed on the CPU by tests/test_pose_cov_mp_ref.py (which also shows each below the old tolerance everywhere):
  cross     M = the block of M_Sigma
  rel       M = |J| M_joint |J|^T + |J| |Sigma_joint| |J|^T, J the mp-differenced Jacobian of the relative pose (not the adjoint formula); M == 0 is an exact zero
Observed error-to-tolerance ratios: profiles/pose_cov.txt."""
import ctypes as C

import numpy as np
import pytest

from suo_slam_amd import _lib, ba
from tests import pose_cov_cases as K
from tests import pose_cov_pair_cases as PK
from tests import pose_cov_mp_ref as MP
from tests import pose_cov_pairs_ref as PR

pytestmark = pytest.mark.gpu

NAMES = ["moved_1x8", "moved_1x9", "moved_1x17", "moved_cam_only", "3x2", "5x16"]


def _case(name):
    """(graph, pairs [P,2], CovRef): the graph a deep copy, the reference shared and read-only"""
    g = MP.graph(name)
    return g, PK.pairs_of(g, PK.OBJ_PAIRS.get(name, [(0, 1)])), MP.case(name)


def _check(g, pairs, got, cr, what):
    """every pair against the reference to its tolerance; NaN blocks exactly where the reference has them and status[2] counting them; rel symmetric with a
    positive diagonal, 36 zeros exactly for two fixed objects"""
    cam, obj, cross, rel, status = got
    worst, pr = MP.check_pairs(pairs, cross, rel, status[2], cr, what)
    fixed = np.r_[g["cam_fixed"], g["obj_fixed"]].astype(bool)
    for q, (a, b) in enumerate(pairs):
        if np.isnan(pr.rel[q]).any():
            continue
        if fixed[a] and fixed[b]:
            assert not rel[q].any() and not cross[q].any(), (what, q, "two fixed vertices: 36 zeros")
        else:
            assert (np.diag(rel[q]) > 0).all(), (what, q, a, b)
        if fixed[a] or fixed[b]:
            assert not cross[q].any(), (what, q, "a fixed vertex has no cross block")
    assert list(status[:2]) == list(cr.marginals().status), (what, status)
    print(f"pose_cov_pairs {what}: error / tolerance: cross {worst['cross']:.4f}  rel cam-obj {worst['cam-obj']:.4f}  rel obj-obj {worst['obj-obj']:.4f}")
    return pr


def _same_bits(x, y):
    return all(np.array_equal(a, b, equal_nan=True) for a, b in zip(x, y))


@pytest.mark.parametrize("name", NAMES)
def test_pairs_meet_the_tolerances_and_the_marginal_blocks_keep_their_bits(name):
    g, pairs, ref = _case(name)
    got = ba.pose_covariances_pairs(*K.args(g), pairs=pairs)
    _check(g, pairs, got, ref, name)
    marg = ba.pose_covariances(*K.args(g))
    assert _same_bits((got[0], got[1], got[4][:2]), marg), "cam_cov / obj_cov / status[:2] are the existing entry's, bit for bit"
    assert _same_bits(got, ba.pose_covariances_pairs(*K.args(g), pairs=pairs)), "two calls give the same bits"


def test_rel_is_the_camera_block_where_the_object_is_fixed():
    g, pairs, ref = _case("moved_cam_only")
    cam, _, cross, rel, _ = ba.pose_covariances_pairs(*K.args(g), pairs=pairs)
    pr = ref.pairs(pairs)
    for q in (0, 1):                                     # (camera 0, object 0), (camera 0, object 1)
        assert (np.abs(rel[q] - cam[0]) <= MP.tol("rel", pr.M_rel[q]) + MP.tol("sigma", ref.marginals().M_cam[0])).all() and not cross[q].any()
    assert not rel[2].any() and not cross[2].any(), "two fixed objects: 36 zeros exactly"
    g = MP.graph("5x16")
    g["obj_fixed"][15] = 1
    pairs = PK.pairs_of(g, [(0, 15), (0, 1)])
    ref = MP.CovRef(g)
    got = ba.pose_covariances_pairs(*K.args(g), pairs=pairs)
    pr = _check(g, pairs, got, ref, "5x16 with object 15 fixed")
    for c in range(1, 5):
        q = c * 16 + 15
        assert tuple(pairs[q]) == (c, 5 + 15)
        assert not got[2][q].any() and (np.abs(got[3][q] - got[0][c]) <= MP.tol("rel", pr.M_rel[q]) + MP.tol("sigma", ref.marginals().M_cam[c])).all()


def test_cross_block_of_a_camera_and_an_object_it_does_not_see():
    g, pairs, ref = _case("5x16")
    pr = ref.pairs(pairs)
    rcross = pr.cross
    c, o = PK.UNSEEN
    assert not ((g["edge_cam"] == c) & (g["edge_obj"] == o)).any() and not g["cam_fixed"][c]
    q = c * 16 + o
    assert tuple(pairs[q]) == (c, 5 + o)
    cross = ba.pose_covariances_pairs(*K.args(g), pairs=pairs)[2]
    assert np.abs(cross[q]).max() > 0 and np.abs(rcross[q]).max() > 0
    assert (np.abs(cross[q] - rcross[q]) <= MP.tol("cross", pr.M_cross[q])).all()
    # the same pair named object first is the transpose, to the bit
    swapped = ba.pose_covariances_pairs(*K.args(g), pairs=[(5 + o, c), (5 + o, 5 + o)])
    assert np.array_equal(swapped[2][0], cross[q].T)
    assert np.array_equal(swapped[2][1], swapped[1][o]) and not swapped[3][1].any(), "a vertex with itself: its marginal block, and a relative pose that cannot move"


def test_every_problem_of_a_batch_that_mixes_the_forms_equals_its_solo_bits_and_a_duplicate_pair_repeats_its_bits():
    names = ("3x2", "moved_1x9", "moved_cam_only", "5x16", "moved_1x17")
    cases = [_case(n) for n in names]
    lists = [np.vstack([pairs, pairs[:3], pairs[-1:]]) for _, pairs, _ in cases]           # duplicates at the end
    batch = ba.pose_covariances_pairs_batch([ba.Problem(*K.args(g)) for g, _, _ in cases], lists)
    for n, (g, pairs, ref), lst, got in zip(names, cases, lists, batch):
        P = len(pairs)
        _check(g, pairs, (got[0], got[1], got[2][:P], got[3][:P], got[4]), ref, "mixed " + n)
        assert _same_bits(got, ba.pose_covariances_pairs(*K.args(g), pairs=lst)), n
        for blocks in (got[2], got[3]):
            assert np.array_equal(blocks[P:P + 3], blocks[:3]) and np.array_equal(blocks[P + 3], blocks[P - 1]), n


def test_relative_covariances_do_not_depend_on_the_gauge():
    g0 = MP.graph("3x2")
    g1 = {k: v.copy() for k, v in g0.items()}
    g1["cam_fixed"] = np.array([0, 1, 0], np.uint8)
    pairs = PK.pairs_of(g0, [(0, 1), (1, 0)])
    ref0, ref1 = MP.case("3x2"), MP.CovRef(g1)
    pr0, pr1 = ref0.pairs(pairs), ref1.pairs(pairs)
    rel0 = ba.pose_covariances_pairs(*K.args(g0), pairs=pairs)[3]
    got1 = ba.pose_covariances_pairs(*K.args(g1), pairs=pairs)
    rel1 = got1[3]
    worst = 0.0
    for q, (a, b) in enumerate(pairs):
        tol = MP.tol("rel", pr0.M_rel[q]) + MP.tol("rel", pr1.M_rel[q])
        err = float((np.abs(rel0[q] - rel1[q]) / tol).max())
        worst = max(worst, err)
        assert err <= 1.0, (q, a, b, err)
    print(f"pose_cov_pairs 3x2, camera 0 fixed against camera 1 fixed: difference / summed tolerance {worst:.4f}")
    marg0 = ba.pose_covariances(*K.args(g0))[1][0]
    both = MP.tol("sigma", ref0.marginals().M_obj[0]).max() + MP.tol("sigma", ref1.marginals().M_obj[0]).max()
    assert np.abs(marg0 - got1[1][0]).max() > 1e3 * both, "the marginal block of object 0 does depend on the gauge"


@pytest.mark.parametrize("name,o", [("1x8", 3), ("moved_1x8", 3), ("5x16", 7)])
def test_an_object_without_a_counted_edge_nans_its_pairs_and_the_others_still_meet_the_tolerances(name, o):
    g = MP.graph(name)
    g["edge_inlier"][g["edge_obj"] == o] = 0
    pairs = PK.pairs_of(g, [(0, 1), (o, 0), (1, o)])
    ref = MP.CovRef(g)
    nc = len(g["cam_T"])
    hit = np.array([nc + o in (a, b) for a, b in pairs])
    assert ref.pairs(pairs).n_nan == hit.sum() == nc + 2
    got = ba.pose_covariances_pairs(*K.args(g), pairs=pairs)
    assert np.isnan(got[2][hit]).all() and np.isnan(got[3][hit]).all() and np.isfinite(got[3][~hit]).all() and got[4][2] == nc + 2
    _check(g, pairs, got, ref, f"{name} without object {o}")


def _raw_call(g, pair_a, pair_b, n_pair=None):
    """suo_pose_covariances_pairs itself, with null outputs: (return code, error text)"""
    lib = _lib.lib()
    p = ba.Problem(*K.args(g))
    s = _lib.BaProblem()
    p._fill(s)
    a, b = np.asarray(pair_a, np.int32), np.asarray(pair_b, np.int32)
    rc = lib.suo_pose_covariances_pairs(C.byref(s), len(a) if n_pair is None else n_pair, a.ctypes.data, b.ctypes.data, None, None, None, None, None)
    return rc, lib.suo_last_error().decode()


def test_bad_pairs_and_seventeen_free_objects_are_refused_and_no_pairs_is_the_existing_call():
    g = MP.graph("3x2")
    for a, b, n, text in (([0], [5], None, "outside"), ([-1], [3], None, "outside"), ([3], [5], None, "outside"), ([0], [1], None, "camera, camera"),
                          ([2], [2], None, "camera, camera"), ([0], [3], -1, "n_pair")):
        rc, err = _raw_call(g, a, b, n)
        assert rc == 1 and text in err, (a, b, n, rc, err)
    with pytest.raises(_lib.SuoError, match=r"code 1\)"):
        ba.pose_covariances_pairs(*K.args(g), pairs=[(0, 3), (1, 2)])
    g17, _ = K.case("2x17")
    with pytest.raises(_lib.SuoError, match=r"code 1\).*17 free objects"):
        ba.pose_covariances_pairs(*K.args(g17), pairs=[(1, 2)])
    none = ba.pose_covariances_pairs(*K.args(g), pairs=np.zeros((0, 2), np.int32))
    assert none[2].shape == (0, 6, 6) and none[3].shape == (0, 6, 6) and none[4][2] == 0
    assert _same_bits((none[0], none[1], none[4][:2]), ba.pose_covariances(*K.args(g)))


def test_object_slam_reports_the_covariance_of_every_pose_it_reports(state_dict):
    from suo_slam_amd import synthetic as S
    from suo_slam_amd.object_slam import ObjectSLAM, to4x4
    seq = S.make_slam_sequence(np.random.default_rng(3), 3, 6)
    slam = ObjectSLAM(None, seq["mesh_db"], state_dict=state_dict, max_crops=16, debug_gt_kp=True, manual_kp_std=0.01, run_network_in_debug=True)
    for vw in seq["views"]:
        slam.process_view(vw["view_id"], vw["image"], vw["K"], vw["obj_ids"].copy(), vw["bboxes"].copy(), vw["model_kps"], vw["model_kps_masks"], vw["kp_masks"],
                          uv_gt=vw["uv_gt"])
    poses = ({v: T.copy() for v, T in slam.cam_poses.items()}, {o: T.copy() for o, T in slam.obj_poses.items()})
    inl = {(v, o): np.array(d["inliers"]) for v, det in slam.detections.items() for o, d in det.items()}
    plain = slam.collect_results()
    assert "rel" not in slam.pose_covariances()
    out = slam.pose_covariances(relative=True)
    assert set(out) == {"cams", "objs", "rel"} and list(out["rel"]) == [(v, o) for v in slam.cam_poses for o in slam.obj_poses]
    assert len(slam.cam_poses) == 3 and len(slam.obj_poses) >= 4
    for k, S6 in out["rel"].items():
        assert S6.shape == (6, 6) and np.isfinite(S6).all() and (np.diag(S6) > 0).all() and np.array_equal(S6, S6.T), k
    first = next(iter(slam.cam_poses))
    Tc = to4x4(slam.cam_poses[first])
    A = PR.adjoint(Tc)
    for o, So in out["objs"].items():
        tol = 36 * np.abs(A).max() ** 2 * np.finfo(np.float64).eps * np.abs(So).max() * 10
        assert np.abs(out["rel"][(first, o)] - A @ So @ A.T).max() <= tol, o
    with_cov = slam.collect_results(covariances=True)
    assert list(with_cov) == list(plain)
    for v in plain:
        assert list(with_cov[v]["poses"]) == list(plain[v]["poses"])
        for o, entry in plain[v]["poses"].items():
            assert "cov_OtoC" not in entry and set(entry) == {"T_OtoC", "score"}
            full = with_cov[v]["poses"][o]
            assert set(full) == {"T_OtoC", "score", "cov_OtoC"} and full["score"] == entry["score"]
            if entry["T_OtoC"] is None:
                assert full["T_OtoC"] is None and full["cov_OtoC"] is None
            else:
                assert np.array_equal(full["T_OtoC"], entry["T_OtoC"]) and np.array_equal(full["cov_OtoC"], out["rel"][(v, o)])
    sub = slam.pose_covariances(view_ids=[first], relative=True)
    assert list(sub["rel"]) == [(first, o) for o in slam.obj_poses]
    for v, T in slam.cam_poses.items():
        assert np.array_equal(T, poses[0][v])
    for o, T in slam.obj_poses.items():
        assert np.array_equal(T, poses[1][o])
    for (v, o), flags in inl.items():
        assert np.array_equal(slam.detections[v][o]["inliers"], flags)
