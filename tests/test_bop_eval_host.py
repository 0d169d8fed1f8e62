"""Host side of the BOP-19 MSSD / MSPD recall (row N5) against the reference's vendored bop_toolkit as recorded in tests/golden/bop19_golden.npz
(tests/golden/make_bop19_golden.py): the symmetry sets, the numpy restatement of the two errors that the GPU tests measure against, and Bop19Meter's
selection, gating, normalisation, matching and recall."""
import os

import numpy as np
import pytest

from suo_slam_amd import bop_eval
from tests import bop_errors_ref as REF
from tests.golden import bop19_cases as BC

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bop19_golden.npz"))


@pytest.mark.parametrize("step", BC.SYM_STEPS)
@pytest.mark.parametrize("name", list(BC.SYM_INFOS))
def test_symmetry_transformations_equal_the_toolkits(name, step):
    """Count and order exact, values to 1e-15."""
    want = GOLD[f"sym_{name}_{step}"]
    got = bop_eval.symmetry_transformations(BC.SYM_INFOS[name], step)
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.abs(got - want).max() <= 1e-15
    if step == 0.01:
        assert len(got) == {"none": 1, "disc1": 2, "disc3": 4, "cont0": 314, "cont_off": 314, "both1": 628, "both3": 1256}[name]


def test_restatement_equals_the_recorded_toolkit_errors():
    """Same tolerance as the device test (abs 1e-9 + rel 1e-12, derived there); the pairs behind the camera (the last N_BEHIND) are finite and included."""
    syms = {name: bop_eval.symmetry_transformations(info, 0.01) for name, info in BC.SYM_INFOS.items()}
    pairs = BC.pairs(lambda name: syms[name])
    assert len(pairs) == len(GOLD["mssd"]) == BC.N_PAIRS + BC.N_BEHIND
    worst = 0.0
    for i, (m, Te, Tg, K) in enumerate(pairs):
        e3, e2 = REF.pose_errors(BC.model_points(m), Te, Tg, K, syms[BC.MODELS[m][1]])
        for got, want in ((e3, GOLD["mssd"][i]), (e2, GOLD["mspd"][i])):
            assert np.isfinite(want) and abs(got - want) <= 1e-9 + 1e-12 * abs(want), (i, got, want)
            worst = max(worst, abs(got - want))
    print("max |restatement - toolkit| =", worst)
    assert np.isfinite(GOLD["mssd"][BC.N_PAIRS:]).all() and (GOLD["mspd"][BC.N_PAIRS:] > 0).all()


def test_restatement_reports_inf_for_non_finite_pairs():
    pts = np.array([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0]], np.float32)
    I = np.eye(3, 4)
    K = np.array([[600.0, 0, 320], [0, 600, 240], [0, 0, 1]])
    T0 = I.copy()                                                    # point 0 at z exactly 0: the projection divides by zero, the 3-D distance is fine
    e3, e2 = REF.pose_errors(pts, T0, T0, K, I[None])
    assert e3 == 0.0 and e2 == np.inf
    Tn = I.copy()
    Tn[0, 3] = np.nan
    assert REF.pose_errors(pts, Tn, T0 + [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 500.0]], K, I[None]) == (np.inf, np.inf)


# ---- the meter ---------------------------------------------------------------------------------------------
class _TableErrors:
    """Stand-in for BopErrors that must not be called: the matching tests feed error tables directly."""
    models_info, max_sym_disc_step = {}, 0.01

    def errors(self, *a):
        raise AssertionError("no device call expected")


@pytest.mark.parametrize("tag,scale,thresholds", [("mssd", 1.0, bop_eval.MSSD_THRESHOLDS), ("mspd", 100.0, bop_eval.MSPD_THRESHOLDS)])
def test_matching_and_recalls_equal_the_toolkits(tag, scale, thresholds):
    """match_poses_scene + calc_localization_scores on the synthetic table (several instances per class, ties in score, invalid ground truths, estimates beyond
    n_top): the estimate matched to every ground truth at every threshold, and the ten recalls, exactly."""
    gt_obj_ids, gt_valid, inst_count, ests = BC.match_case()
    assert any(len(rows) > inst_count[k] for k, rows in ests.items()) and any(not all(v) for v in gt_valid.values())
    assert any(len({r["score"] for r in rows}) < len(rows) for rows in ests.values())
    est_of_gt = []
    for th in thresholds:
        row = []
        for im, objs in gt_obj_ids.items():
            errs = {}
            for (im2, o), rows in ests.items():
                if im2 == im:
                    errs[o] = [{"est_id": i, "score": r["score"], "errors": {g: scale * e for g, e in r["errors"].items()}}
                               for i, r in bop_eval.top_estimates(rows, inst_count[(im, o)])]
            row += bop_eval.match_poses_image(objs, gt_valid[im], errs, float(th))
        est_of_gt.append(row)
    assert np.array_equal(np.array(est_of_gt), GOLD[f"match_{tag}_est"])
    valid = np.concatenate([gt_valid[im] for im in gt_obj_ids])
    recalls = [float(((np.array(r) != -1) & valid).sum()) / float(valid.sum()) for r in est_of_gt]
    assert recalls == GOLD[f"match_{tag}_recall"].tolist() and int(valid.sum()) == int(GOLD[f"match_{tag}_targets"])


def _one_object_meter(T_ests, scores, T_gts, visib, inst_count, diameter=100.0, im_width=640, obj_pts=None):
    """A meter over one image of one object class (id 5) with the restatement as its error source."""
    pts = np.array([[0, 0, 0], [40, 0, 0], [0, 30, 0], [0, 0, 20]], np.float32) if obj_pts is None else obj_pts
    info = {5: {"diameter": diameter}}
    errs = REF.RefErrors({5: {"points": pts}}, info)
    gt = {1: {7: [{"cam_R_m2c": T[:, :3].ravel().tolist(), "cam_t_m2c": T[:, 3].tolist(), "obj_id": 5} for T in T_gts]}}
    gi = {1: {7: [{"visib_fract": v} for v in visib]}}
    meter = bop_eval.Bop19Meter(errs, [{"scene_id": 1, "im_id": 7, "obj_id": 5, "inst_count": inst_count}], gt, gi, im_width)
    K = np.array([[600.0, 0, 320], [0, 600, 240], [0, 0, 1]])
    for T, s in zip(T_ests, scores):
        meter.add(1, 7, 5, s, T, K)
    return meter, errs


def _pose(tx=0.0, tz=800.0):
    T = np.eye(3, 4)
    T[:, 3] = [tx, 0.0, tz]
    return T


def test_sphere_gate_from_both_sides():
    """|t_est - t_gt| < diameter is evaluated; >= diameter is inf for MSSD (MSPD is still computed), eval_calc_errors.py:306-325."""
    just_inside, on_the_edge = np.nextafter(100.0, 0.0), 100.0
    for shift, gated in ((just_inside, False), (on_the_edge, True), (150.0, True)):
        meter, errs = _one_object_meter([_pose(shift)], [1.0], [_pose()], [1.0], 1)
        row = meter.error_table()[1][7][5][0]
        e3, e2 = row["errors"][0]
        assert (e3 == np.inf) == gated, (shift, e3)
        assert np.isfinite(e2) and e2 > 0
        if not gated:
            assert abs(e3 - shift) <= 1e-9                              # a pure translation moves every point by it


def test_both_normalisations_from_both_sides():
    """MSSD / diameter against 0.05 .. 0.5 and MSPD * 640 / width against 5 .. 50, each just below and just above a threshold (strict <)."""
    # a translation of 9.99 / 10.01 mm at diameter 100: 0.0999 < 0.1 is a hit from the second threshold on, 0.1001 from the third
    for shift, hits in ((9.99, 9), (10.01, 8)):
        meter, _ = _one_object_meter([_pose(shift)], [1.0], [_pose()], [1.0], 1)
        res = meter.result()
        assert res["mssd"]["recalls"] == [0.0] * (10 - hits) + [1.0] * hits and res["n_targets"] == 1 and res["n_estimates"] == 1
    # 600 px focal length at z = 800: a shift of x mm moves the projections of the z = 800 points by 0.75 x px; width 1280 halves it
    pts = np.array([[0, 0, 0], [40, 0, 0], [0, 30, 0]], np.float32)
    for shift, width, hits in ((13.2, 640, 9), (13.4, 640, 8), (26.4, 1280, 9), (26.8, 1280, 8)):       # 9.9 / 10.05 px after normalisation
        meter, _ = _one_object_meter([_pose(shift)], [1.0], [_pose()], [1.0], 1, im_width=width, obj_pts=pts)
        assert meter.result()["mspd"]["recalls"] == [0.0] * (10 - hits) + [1.0] * hits, (shift, width)


def test_selection_validity_and_missing_targets():
    """inst_count keeps the best-scored estimates (ties: first given), the most visible ground truths are the valid ones, a target without estimates counts."""
    good, bad = _pose(1.0), _pose(60.0)
    # two ground truths 300 mm apart, inst_count 1: only the more visible (the second) is valid; the kept estimate is the first of the tied pair
    gts = [_pose(0.0), _pose(300.0)]
    meter, errs = _one_object_meter([_pose(301.0), _pose(1.0), _pose(2.0)], [2.0, 2.0, 1.0], gts, [0.4, 0.9], 1)
    res = meter.result()
    assert res["n_estimates"] == 1 and res["n_targets"] == 1 and errs.calls == 2
    assert res["mssd"]["recalls"] == [1.0] * 10                         # estimate 0 sits 1 mm from the valid ground truth
    meter, _ = _one_object_meter([_pose(1.0), _pose(301.0)], [2.0, 2.0], gts, [0.4, 0.9], 1)
    assert meter.result()["mssd"]["ar"] == 0.0                          # now the kept one matches only the invalid ground truth
    meter, _ = _one_object_meter([], [], gts, [0.4, 0.9], 2)
    res = meter.result()
    assert res["n_targets"] == 2 and res["n_estimates"] == 0 and res["mssd"]["ar"] == 0.0 and res["mspd"]["ar"] == 0.0
    assert res["max_sym_disc_step"] == 0.01 and len(res["mspd"]["recalls"]) == 10


def test_load_models_info_and_tree_reader(tmp_path):
    from tests import bop_tree
    desc = bop_tree.build(str(tmp_path), dset="tless", seed=3, n_scenes=2, n_views=2)
    info = bop_eval.load_models_info(os.path.join(desc["data_root"], "models_eval"))
    assert set(info) == set(range(1, 31)) and "symmetries_continuous" in info[7] and "symmetries_discrete" in info[5]
    assert len(bop_eval.symmetry_transformations(info[7])) == 314 and len(bop_eval.symmetry_transformations(info[35 if 35 in info else 5])) == 2
    meter = bop_eval.Bop19Meter.from_dataset_tree(_TableErrors(), os.path.join(desc["data_root"], desc["split"]),
                                                  os.path.join(desc["data_root"], "all_target_tless.json"), 640)
    # unfiltered: the ground truth at 5 % visibility that BopDataset drops is still there
    assert any(i["visib_fract"] < 0.1 for ims in meter.scene_gt_info.values() for infos in ims.values() for i in infos)
    assert sum(len(o) for ims in meter.targets.values() for o in ims.values()) > 0
