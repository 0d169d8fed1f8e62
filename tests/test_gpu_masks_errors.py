"""suo_pose_errors_masks (csrc/eval_masks.hip, row N4) on the device, through BopErrors.mask_errors: what the toolkit's pose_error.cus and cou_bb_proj take
from two renders.

Yardsticks: union, intersection and the two boxes of the numpy rasteriser's renders (tests/points_errors_ref.mask_counts over tests/vsd_ref.render_depth),
and the toolkit's own cus / cou_bb_proj on the same pairs over that rasteriser (tests/golden/siso_golden.npz, recorded by tests/golden/make_siso_golden.py).
Tolerance: none.  The device writes integers, compared as integers; the quotients are formed from them in fp64 exactly as the toolkit forms them and are
compared bit for bit.  One condition, asserted by the generator and again here on the regenerated inputs: no sample of either render lies within the NEAR
band of a triangle edge in the numpy rasteriser -- the only place where the device's coverage may differ from it.
Cases (tests/golden/siso_cases.mask_pairs, images 160 x 96 = 3 x 2 tiles, the last column and row partial): the pairs of the SISO tree, renders that miss
each other (a union of two, intersection 0), an estimate off the image (an empty box: cou_bb_proj 1.0 where the toolkit raises), both off the image
(union 0: cus 1.0), renders across the 64-pixel tile boundaries, est == gt."""
import os

import numpy as np
import pytest

from suo_slam_amd import _lib, bop_eval
from tests import points_errors_ref as PR
from tests import vsd_ref as VR
from tests.golden import siso_cases as SC

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "siso_golden.npz"))
KEYS = ("cus", "cou_bb_proj", "union", "inter", "box_est", "box_gt")


@pytest.fixture(scope="module")
def be():
    e = bop_eval.BopErrors(SC.mesh_db(), SC.models_info())
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases():
    mp = SC.mask_pairs()
    return [p[0] for p in mp], [p[1] + 1 for p in mp], np.stack([p[2] for p in mp]), np.stack([p[3] for p in mp]), np.stack([p[4] for p in mp])


@pytest.fixture(scope="module")
def reference(cases):
    labels, objs, Te, Tg, K = cases
    db, out = SC.mesh_db(), []
    for lab, o, e, g, k in zip(labels, objs, Te, Tg, K):
        renders = {}
        for T in (e, g):
            renders[T.tobytes()], near = VR.render_depth(db[o]["points"], db[o]["faces"], T, k, SC.W, SC.H, with_near=True)
            assert not near.any(), lab
        out.append(PR.mask_counts(None, None, e, g, k, SC.W, SC.H, renders=lambda T: renders[T.tobytes()]))
    return out


@pytest.fixture(scope="module")
def batch(be, cases):
    return be.mask_errors(cases[1], cases[2], cases[3], cases[4], (SC.H, SC.W))


def test_counts_and_boxes_equal_the_numpy_rasteriser(cases, reference, batch):
    assert tuple(batch) == KEYS and batch["union"].dtype == np.int64 and batch["box_est"].dtype == np.int32
    for i, (lab, (u, n, be_, bg)) in enumerate(zip(cases[0], reference)):
        print(f"{lab:22s} union {u:5d} inter {n:5d} box_est {be_} box_gt {bg}  device {int(batch['union'][i])} {int(batch['inter'][i])} "
              f"{batch['box_est'][i].tolist()} {batch['box_gt'][i].tolist()}")
        assert (int(batch["union"][i]), int(batch["inter"][i]), batch["box_est"][i].tolist(), batch["box_gt"][i].tolist()) == (u, n, be_, bg), lab


def test_quotients_equal_the_toolkit_bit_for_bit(cases, batch):
    assert len(cases[0]) == len(GOLD["masks"])
    for i, (lab, (cus, bb)) in enumerate(zip(cases[0], GOLD["masks"])):
        assert batch["cus"][i] == cus, lab
        if np.isnan(bb):                                                       # the toolkit raised on an empty mask: 1.0 here, as include/suo_hip.h says
            assert batch["cou_bb_proj"][i] == 1.0 and -1 in (batch["box_est"][i][2], batch["box_gt"][i][2]), lab
        else:
            assert batch["cou_bb_proj"][i] == bb, lab


def test_the_cases_hold_what_they_were_designed_to_hold(cases, reference):
    by = dict(zip(cases[0], reference))
    u, n, be_, bg = by["apart"]
    assert n == 0 and u > 0 and be_[2] > 0 and bg[2] > 0                        # two renders that miss each other
    u, n, be_, bg = by["est_off_image"]
    assert be_ == [-1] * 4 and bg[2] > 0 and n == 0 and u > 0
    assert by["both_off_image"] == (0, 0, [-1] * 4, [-1] * 4)
    for lab in ("across_tiles", "across_tiles_border"):
        u, n, be_, bg = by[lab]
        assert bg[0] < 64 <= bg[0] + bg[2] or bg[0] < 128 <= bg[0] + bg[2], lab      # the ground truth's box crosses a tile column ...
        assert bg[1] < 64 <= bg[1] + bg[3], lab                                      # ... and the tile row
    u, n, be_, bg = by["same"]
    assert u == n > 0 and be_ == bg
    assert by["across_tiles_border"][3][0] + by["across_tiles_border"][3][2] == SC.W - 1      # clipped by the image's right border: the partial tile column


def test_a_pair_has_the_same_values_alone_and_in_any_batch(be, cases, batch):
    labels, objs, Te, Tg, K = cases
    for i in range(len(objs)):
        one = be.mask_errors(objs[i:i + 1], Te[i:i + 1], Tg[i:i + 1], K[i:i + 1], (SC.H, SC.W))
        for k in KEYS:
            assert np.array_equal(one[k][0], batch[k][i]), (labels[i], k)
    rev = be.mask_errors(objs[::-1], Te[::-1], Tg[::-1], K[::-1], (SC.H, SC.W))
    for k in KEYS:
        assert np.array_equal(rev[k][::-1], batch[k]), k
    empty = be.mask_errors([], np.zeros((0, 3, 4)), np.zeros((0, 3, 4)), K[0], (SC.H, SC.W))
    assert empty["cus"].shape == (0,) and empty["box_est"].shape == (0, 4)


def test_more_pairs_than_one_launch_are_split_inside(be, cases, batch):
    labels, objs, Te, Tg, K = cases
    i = labels.index("across_tiles")
    n = 1030                                                                   # one launch takes 1024 pairs
    out = be.mask_errors([objs[i]] * n, np.repeat(Te[i:i + 1], n, 0), np.repeat(Tg[i:i + 1], n, 0), K[i], (SC.H, SC.W))
    for k in KEYS:
        assert np.all(out[k] == batch[k][i]), k


def test_bad_arguments_are_refused(be, cases):
    labels, objs, Te, Tg, K = cases
    bad = Te[:1].copy()
    bad[0, 0, 0] = np.nan
    with pytest.raises(_lib.SuoError, match="not finite"):
        be.mask_errors(objs[:1], bad, Tg[:1], K[:1], (SC.H, SC.W))
    with pytest.raises(_lib.SuoError, match="width and height"):
        be.mask_errors(objs[:1], Te[:1], Tg[:1], K[:1], (0, SC.W))
    points_only = bop_eval.BopErrors({1: {"points": SC.mesh_db()[1]["points"]}}, {1: {"diameter": 1.0}})
    try:
        with pytest.raises(_lib.SuoError, match="no faces"):
            points_only.mask_errors([1], Te[:1], Tg[:1], K[:1], (SC.H, SC.W))
    finally:
        points_only.close()
