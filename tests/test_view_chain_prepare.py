"""The prepare half of a SLAM pass on the device chain (suo_slam_amd/view_chain.py: ChainPass.__init__, vote_block) on a tiny hand-made state: 2 pass-A and
2 pass-B objects, one of each in the map, 41 keypoints with a few masked.  Pure numpy: what goes to the device, and where it lies in the staged list, is
decided here and seen by no other CPU test."""
import itertools

import numpy as np
import pytest

from suo_slam_amd.frame_geom import kbbox_terms
from suo_slam_amd.geometry import fix_K_for_bbox_ndc
from suo_slam_amd.view_chain import ChainPass, vote_block
from tests import slam_states as SS
from tests.slam_vote_ref import A_IN, A_K, A_T, B_IN, B_K, B_T, BLOCK, NUM_KP

K = SS.K_YCBV
MESH_DB = {3: {"diameter": 172.0}, 7: {"diameter": 93.5}, 11: {"diameter": 250.25}, 12: {"diameter": 61.0}}
FLAGS = dict(no_network_cov=False, bbox_thresh=0.9, kp_var_thresh=0.2)


def _objs(rng, ids, bboxes):
    L = len(ids)
    model_masks = np.ones((L, NUM_KP), bool)
    model_masks[0, [4, 17]] = False
    model_masks[1, 30:] = False
    gt_masks = model_masks & (rng.uniform(size=(L, NUM_KP)) > 0.2)
    return (np.array(ids), np.array(bboxes, np.float64), rng.uniform(-80, 80, (L, NUM_KP, 3)), model_masks, gt_masks,
            rng.uniform(-1, 1, (L, NUM_KP, 2)).astype(np.float32))


@pytest.fixture(scope="module")
def state():
    rng = np.random.default_rng(5)
    A = _objs(rng, [3, 7], [[101.5, 60.25, 233.0, 201.75], [300.0, 122.5, 480.5, 297.0]])
    B = _objs(rng, [11, 12], [[20.0, 250.5, 150.25, 401.0], [410.75, 33.0, 520.0, 140.5]])
    T4 = np.eye(4)
    T4[:3] = rng.uniform(-2, 2, (3, 4))
    obj_poses = {7: rng.uniform(-2, 2, (3, 4)), 11: T4}          # ([3,4] and [4,4] both occur in the map); 3 and 12 are not in it
    return A, B, obj_poses


def _pass(objs, seed=0, debug_gt_kp=False, **kw):
    rng = np.random.default_rng(seed)
    return ChainPass(K, objs, MESH_DB, rng, debug_gt_kp=debug_gt_kp, **FLAGS, **kw), rng


def _K_bbox32(objs):
    return np.stack([fix_K_for_bbox_ndc(K, bb) for bb in objs[1]]).astype(np.float32)


def test_vote_block_is_the_kernels_layout(state):
    A, B, obj_poses = state
    pa, _ = _pass(A)
    blk = vote_block(K, A[0], pa.K_bbox, B[0], B[1], obj_poses)
    want = np.zeros(BLOCK)
    want[A_IN + 1] = 1.0
    want[A_T + 12:A_T + 24] = obj_poses[7].reshape(-1)
    want[B_IN + 0] = 1.0
    want[B_T:B_T + 12] = obj_poses[11][:3].reshape(-1)
    for k in range(2):
        want[A_K + 9 * k:A_K + 9 * k + 9] = fix_K_for_bbox_ndc(K, A[1][k]).astype(np.float32).astype(np.float64).reshape(-1)   # the float32 container
        want[B_K + 9 * k:B_K + 9 * k + 9] = fix_K_for_bbox_ndc(K, B[1][k]).reshape(-1)                                         # the double
    assert blk.dtype == np.float64 and blk.shape == (BLOCK,)
    assert np.array_equal(blk, want)
    assert not np.array_equal(want[A_K:A_K + 9], fix_K_for_bbox_ndc(K, A[1][0]).reshape(-1))     # (the two containers do differ on these boxes)
    pb, _ = _pass(B, block=blk)
    assert pb.host_arrays[pb.pos["block"]] is blk


def test_ground_truth_draws_are_the_host_routes(state):
    """The host route (_run_kp_model) computes uv_gt[k][m] + rng.normal(scale=0.01, size=...) object by object, pass A's objects then pass B's."""
    A, B, _ = state
    rng = np.random.default_rng(42)
    got = []
    for objs in (A, B):
        cp = ChainPass(K, objs, MESH_DB, rng, debug_gt_kp=True, **FLAGS)
        got.append((cp.host_arrays[cp.pos["gt_mask"]], cp.host_arrays[cp.pos["gt_uv"]]))
    ref = np.random.default_rng(42)
    for objs, (gt_mask, gt_uv) in zip((A, B), got):
        assert gt_mask.dtype == np.uint8 and np.array_equal(gt_mask.astype(bool), objs[4])
        assert gt_uv.dtype == np.float32 and gt_uv.shape == (2, NUM_KP, 2)
        for k in range(2):
            m = objs[4][k]
            uv_pred = objs[5][k][m].astype(np.float64)
            uv_pred = uv_pred + ref.normal(scale=0.01, size=uv_pred.shape)
            assert np.array_equal(gt_uv[k][m], uv_pred.astype(np.float32))
            assert not gt_uv[k][~m].any()
    assert rng.bit_generator.state == ref.bit_generator.state
    cp, rng = _pass(A, seed=42)                                  # without ground truth nothing is drawn
    assert rng.bit_generator.state == np.random.default_rng(42).bit_generator.state


def test_per_crop_terms(state):
    A, B, _ = state
    for objs in (A, B):
        cp, _ = _pass(objs)
        Kb = _K_bbox32(objs)
        assert cp.K_bbox.dtype == np.float32 and np.array_equal(cp.K_bbox, Kb)
        kinv, camk = kbbox_terms(Kb)
        assert np.array_equal(cp.kinv, kinv) and np.array_equal(cp.camk, camk)
        assert cp.min_depth.dtype == np.float64 and np.array_equal(cp.min_depth, [0.5 * MESH_DB[o]["diameter"] for o in objs[0]])
        assert cp.vt == 0.2 and cp.use_cov
    given, _ = _pass(A, K_bbox=_K_bbox32(A))                     # (a caller that has K_bbox already)
    assert np.array_equal(given.kinv, kbbox_terms(_K_bbox32(A))[0])
    flags = dict(FLAGS, no_network_cov=True)
    cp = ChainPass(K, A, MESH_DB, np.random.default_rng(0), debug_gt_kp=False, **flags)
    assert cp.vt == 1e30 and not cp.use_cov


@pytest.mark.parametrize("priors,gt", list(itertools.product((False, True), repeat=2)))
def test_named_positions_of_the_host_arrays(state, priors, gt):
    A, B, _ = state
    ids, bboxes, kps, model_masks, gt_masks, uv_gt = B
    prior = (np.random.default_rng(9).uniform(-1, 1, (NUM_KP, 2)).astype(np.float32), model_masks[1].astype(np.uint8))
    cp, _ = _pass(B, debug_gt_kp=gt, prior_dets={12: prior} if priors else None)
    names = ["kps", "boxes", "class_mask"] + (["gt_mask", "gt_uv"] if gt else []) + (["prior_uv", "prior_mask"] if priors else [])
    assert sorted(cp.pos, key=cp.pos.get) == names and sorted(cp.pos.values()) == list(range(len(cp.host_arrays)))
    at = lambda name: cp.host_arrays[cp.pos[name]]  # noqa: E731
    assert at("kps").dtype == np.float32 and np.array_equal(at("kps"), kps.astype(np.float32))
    assert at("boxes").dtype == np.float32 and np.array_equal(at("boxes"), bboxes.astype(np.float32))
    assert at("class_mask").dtype == np.uint8 and np.array_equal(at("class_mask"), model_masks)
    if gt:
        assert at("gt_mask").shape == (2, NUM_KP) and np.array_equal(at("gt_mask"), gt_masks)
        assert at("gt_uv").shape == (2, NUM_KP, 2) and at("gt_uv").dtype == np.float32
    if priors:
        assert at("prior_uv").dtype == np.float32 and at("prior_mask").dtype == np.uint8
        assert not at("prior_uv")[0].any() and not at("prior_mask")[0].any()          # object 11 has no prior
        assert np.array_equal(at("prior_uv")[1], prior[0]) and np.array_equal(at("prior_mask")[1], prior[1])
    blk = np.arange(float(BLOCK))
    with_block, _ = _pass(B, debug_gt_kp=gt, block=blk)         # the vote's block takes the place behind the class mask
    assert sorted(with_block.pos, key=with_block.pos.get) == ["kps", "boxes", "class_mask", "block"] + (["gt_mask", "gt_uv"] if gt else [])
