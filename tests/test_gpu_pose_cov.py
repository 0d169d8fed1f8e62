"""The pose-covariance kernels (csrc/pose_cov.hip) through the C ABI against the mp reference of tests/pose_cov_mp_ref.py (40 digits, no finite differences).

Tolerance of every element of every block: K["sigma"] eps M, M = |Sigma| MH |Sigma| + |Sigma| sqrt(diag H (x) diag H) |Sigma| entry by entry and K fixed on the CPU by
tests/test_pose_cov_mp_ref.py, which also shows it below the old bound 1e3 eps cond(H) max|Sigma| everywhere.  The graphs (tests/pose_cov_cases.py) are the smallest
at which each form can go wrong: the 8 -> 4 lanes-per-object switch, a full wave, passes of 16 with a partial last pass, the camera-only form, the smallest coupled
graph and the ns = 96 boundary.  Observed error-to-tolerance ratios: profiles/pose_cov.txt."""
import numpy as np
import pytest

from suo_slam_amd import _lib, ba
from tests import pose_cov_cases as K
from tests import pose_cov_mp_ref as MP

pytestmark = pytest.mark.gpu

FORMS = ["1x1_4edges", "1x8", "1x9", "1x16", "1x17", "1x33", "cam_only", "3x2", "5x16"]


def _check(got, cr, what):
    """every block against the reference (a CovRef) to the tolerance; NaN / zero blocks exactly where the reference has them; symmetric to the tolerance, positive
    diagonal"""
    cam, obj, status = got
    worst = MP.check_blocks(cam, obj, status, cr, what)
    print(f"pose_cov {what}: n {cr.n}  max M {cr.M_Sigma.max() if cr.n else 0.0:.3e}  error / tolerance {worst:.4f}")


@pytest.mark.parametrize("name", FORMS)
def test_blocks_meet_the_bound_and_two_calls_give_the_same_bits(name):
    g, ref = MP.graph(name), MP.case(name)
    got = ba.pose_covariances(*K.args(g))
    _check(got, ref, name)
    again = ba.pose_covariances(*K.args(g))
    for a, b in zip(got, again):
        assert np.array_equal(a, b, equal_nan=True)


def test_every_frame_of_a_batch_equals_the_same_frame_alone_bit_for_bit():
    graphs = [(MP.graph(n), MP.case(n)) for n in ("batch_3", "batch_16", "batch_1")]
    batch = ba.pose_covariances_batch([ba.Problem(*K.args(g)) for g, _ in graphs])
    for (g, ref), got in zip(graphs, batch):
        _check(got, ref, "batch")
        alone = ba.pose_covariances(*K.args(g))
        for a, b in zip(got, alone):
            assert np.array_equal(a, b, equal_nan=True)


def test_a_batch_may_mix_the_forms():
    names = ("3x2", "1x9", "cam_only", "5x16")
    graphs = [(MP.graph(n), MP.case(n)) for n in names]
    batch = ba.pose_covariances_batch([ba.Problem(*K.args(g)) for g, _ in graphs])
    for n, (g, ref), got in zip(names, graphs, batch):
        _check(got, ref, "mixed " + n)
        for a, b in zip(got, ba.pose_covariances(*K.args(g))):
            assert np.array_equal(a, b, equal_nan=True)


def test_seventeen_free_objects_next_to_free_cameras_are_refused():
    g, _ = K.case("2x17")
    with pytest.raises(_lib.SuoError, match=r"code 1\).*17 free objects"):
        ba.pose_covariances(*K.args(g))


@pytest.mark.parametrize("name,o", [("1x8", 3), ("1x17", 16), ("3x2", 1), ("5x16", 7)])
def test_an_object_without_a_counted_edge_is_nan_and_the_others_still_meet_the_bound(name, o):
    g = MP.graph(name)
    g["edge_inlier"][g["edge_obj"] == o] = 0
    ref = MP.CovRef(g)
    assert list(ref.marginals().status) == [0, 1] and np.isnan(ref.marginals().obj_cov[o]).all()
    _check(ba.pose_covariances(*K.args(g)), ref, f"{name} without object {o}")


@pytest.mark.parametrize("name,o", [("1x9", 8), ("3x2", 0), ("5x16", 15)])
def test_a_fixed_object_is_zeros(name, o):
    g = MP.graph(name)
    g["obj_fixed"][o] = 1
    ref = MP.CovRef(g)
    assert not ref.marginals().obj_cov[o].any()
    got = ba.pose_covariances(*K.args(g))
    assert not got[1][o].any()
    _check(got, ref, f"{name} with object {o} fixed")


@pytest.mark.parametrize("name", ["1x8", "3x2"])
def test_covariances_after_optimize_leave_the_problem_unchanged(name):
    g = MP.graph(name)
    p = ba.Problem(*K.args(g), its=(10, 10), init_with_outliers=True)        # (the moved poses put every chi2 past the gate: start with all edges in)
    ba.optimize_batch([p])
    assert p.inlier.sum() >= 0.8 * len(p.inlier)
    fields = ("cam_T", "obj_T", "cam_fixed", "obj_fixed", "edge_cam", "edge_obj", "edge_camk", "edge_p", "edge_uv", "edge_info", "inlier", "chi2", "stats")
    before = {k: getattr(p, k).copy() for k in fields}
    got = ba.pose_covariances_batch([p])[0]
    for k in fields:
        assert np.array_equal(getattr(p, k), before[k]), k
    state = dict(g, cam_T=p.cam_T.reshape(-1, 3, 4), obj_T=p.obj_T.reshape(-1, 3, 4), edge_inlier=p.inlier)
    _check(got, MP.CovRef(state), name + " after optimize")


def test_frame_chain_covariances_equal_the_host_built_graph_of_the_accepted_crops():
    import torch
    from suo_slam_amd import synthetic as S
    from suo_slam_amd.frame_geom import FrameGeometry, kbbox_terms
    rng = np.random.default_rng(21)
    n_obj = 8
    fr = S.make_frame(rng, n_obj, noise=0.004, outlier_frac=0.08, with_image=False)
    # make_frame works in millimetres, where rotations and translations differ by 1e3 in scale and cond(H) passes the cap: the same frame in metres (the
    # projection, hence uv / boxes / K_bbox, does not change under a uniform scale)
    fr["model_kps"] = (fr["model_kps"] * 1e-3).astype(np.float32)
    fr["diameter"] = fr["diameter"] * 1e-3
    mask = fr["model_kps_masks"] & (rng.random((n_obj, 41)) >= 0.25)
    mask[1] = False
    mask[1, np.nonzero(fr["model_kps_masks"][1])[0][:2]] = True           # two keypoints: PnP impossible, the crop is rejected
    fg = FrameGeometry(16, 1)
    kinv, camk = kbbox_terms(fr["K_bbox"].astype(np.float32))
    fg.launch([0, n_obj], torch.from_numpy(fr["uv"]).cuda(), torch.from_numpy(fr["cov"]).cuda(), torch.from_numpy(mask.astype(np.uint8)).cuda(),
              torch.from_numpy(fr["model_kps"].astype(np.float32)).cuda(), kinv, camk, 0.5 * fr["diameter"], seed=5)
    assert "obj_cov" not in fg.fetch() and not fg.device_result().obj_cov, "without the call the field is NULL"
    cov = fg.covariances()
    r = fg.fetch()
    assert np.array_equal(r["obj_cov"], cov) and fg.device_result().obj_cov
    acc = r["accepted"]
    assert not acc[1] and acc.sum() >= 6
    assert not cov[~acc].any(), "rejected crops are zeros"
    # the graph of the accepted crops as the chain built it: slots = valid keypoints in mask order, fp64 closed-form inverse of the float32 covariance
    objs = np.nonzero(acc)[0]
    Kb = fr["K_bbox"].astype(np.float32).astype(np.float64)
    e_obj, e_k, e_p, e_uv, e_info, e_inl = [], [], [], [], [], []
    for j, o in enumerate(objs):
        n = int(mask[o].sum())
        c = fr["cov"][o][mask[o]].astype(np.float64)
        det = c[:, 0, 0] * c[:, 1, 1] - c[:, 0, 1] * c[:, 1, 0]
        e_obj.append(np.full(n, j, np.int32)); e_k.append(np.tile([Kb[o][0, 0], Kb[o][1, 1], Kb[o][0, 2], Kb[o][1, 2]], (n, 1)))
        e_p.append(fr["model_kps"][o][mask[o]].astype(np.float64)); e_uv.append(fr["uv"][o][mask[o]].astype(np.float64))
        e_info.append(np.stack([c[:, 1, 1] / det, 0.5 * (-c[:, 0, 1] / det + -c[:, 1, 0] / det), c[:, 0, 0] / det], -1))
        e_inl.append(r["inlier"][o][:n].astype(np.uint8))
    E = sum(len(x) for x in e_obj)
    g = {"cam_T": np.eye(4)[None, :3], "cam_fixed": np.array([1], np.uint8), "obj_T": r["T_opt"][objs], "obj_fixed": np.zeros(len(objs), np.uint8),
         "edge_cam": np.zeros(E, np.int32), "edge_obj": np.concatenate(e_obj), "edge_camk": np.concatenate(e_k), "edge_p": np.concatenate(e_p),
         "edge_uv": np.concatenate(e_uv), "edge_info": np.concatenate(e_info), "edge_inlier": np.concatenate(e_inl)}
    ref = MP.CovRef(g)
    host = ba.pose_covariances(*K.args(g))
    tol = MP.tol("sigma", ref.marginals().M_obj)
    assert (np.abs(cov[objs] - host[1]) <= tol).all(), float((np.abs(cov[objs] - host[1]) / tol).max())
    _check((np.zeros((1, 6, 6)), cov[objs], np.array([0, 0])), ref, "frame chain")
    fg.close()


def test_object_slam_reports_a_block_for_every_pose_of_the_map(state_dict):
    from suo_slam_amd import synthetic as S
    from suo_slam_amd.object_slam import ObjectSLAM
    seq = S.make_slam_sequence(np.random.default_rng(3), 3, 6)
    slam = ObjectSLAM(None, seq["mesh_db"], state_dict=state_dict, max_crops=16, debug_gt_kp=True, manual_kp_std=0.01, run_network_in_debug=True)
    for vw in seq["views"]:
        slam.process_view(vw["view_id"], vw["image"], vw["K"], vw["obj_ids"].copy(), vw["bboxes"].copy(), vw["model_kps"], vw["model_kps_masks"], vw["kp_masks"],
                          uv_gt=vw["uv_gt"])
    poses = ({v: T.copy() for v, T in slam.cam_poses.items()}, {o: T.copy() for o, T in slam.obj_poses.items()})
    out = slam.pose_covariances()
    assert list(out["cams"]) == list(slam.cam_poses) and list(out["objs"]) == list(slam.obj_poses) and len(out["cams"]) == 3 and len(out["objs"]) >= 4
    first = next(iter(slam.cam_poses))
    assert not out["cams"][first].any(), "the gauge camera is fixed"
    for k, S6 in list(out["cams"].items())[1:] + list(out["objs"].items()):
        assert S6.shape == (6, 6) and np.isfinite(S6).all() and (np.diag(S6) > 0).all() and np.allclose(S6, S6.T, rtol=1e-9, atol=0), k
    for v, T in slam.cam_poses.items():
        assert np.array_equal(T, poses[0][v])
    for o, T in slam.obj_poses.items():
        assert np.array_equal(T, poses[1][o])
    assert list(slam.pose_covariances(view_ids=[first])["cams"]) == [first]
