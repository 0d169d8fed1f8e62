"""Evaluator(bop19=True, bop19_vsd=True) end to end on the GPU (row N6): the synthetic T-LESS tree with depth images (the ground truths drawn by the numpy
rasteriser, a background plane, an occluding slab, missing depth) through the hot path.  The VSD recalls it reports are counts of matched targets and must be
the ones a Bop19Meter over the numpy rasteriser and the numpy VSD of tests/vsd_ref.py computes from the CSV it wrote; AR is the mean of the three terms; and
without bop19_vsd the run returns what it returned before."""
import json
import os

import numpy as np
import pytest

from suo_slam_amd import bop, bop_eval, evaluator
from tests import bop_tree
from tests import vsd_ref as VR

pytestmark = pytest.mark.gpu

PARENT_KEYS = {"method", "csv_path", "summary_path", "result", "saved_result", "num_views", "num_cam_poses_found", "fp16_range_reissues", "matrix_pipe_at_end",
               "bop_eval", "seconds"}
BOP19_KEYS = {"mssd", "mspd", "n_targets", "n_estimates", "max_sym_disc_step"}


def _cpu_meter(desc, csv_path, mesh):
    root, split = desc["data_root"], desc["split"]
    ds = bop.BopDataset(root, split, bop_dset="tless", ignore_symmetry=True)
    errs = VR.RefVsdErrors(mesh, bop_eval.load_models_info(os.path.join(root, "models_eval")))
    meter = bop_eval.Bop19Meter.from_dataset_tree(errs, os.path.join(root, split), os.path.join(root, "all_target_tless.json"), 640, depth_loader=ds.read_depth,
                                                  vsd_delta=bop_eval.VSD_DELTAS["tless"])
    cams = {}
    for ln in open(csv_path).read().strip().split("\n"):
        s, v, o, score, R, t, _ = ln.split(",")
        s, v = int(s), int(v)
        if s not in cams:
            cams[s] = json.load(open(os.path.join(root, split, f"{s:06d}", "scene_camera.json")))
        T = np.hstack((np.array(R.split(), float).reshape(3, 3), np.array(t.split(), float).reshape(3, 1)))
        meter.add(s, v, int(o), float(score), T, np.array(cams[s][str(v)]["cam_K"]).reshape(3, 3))
    return meter


def test_vsd_recalls_of_a_run_equal_the_numpy_meter_on_its_csv(tmp_path):
    desc = bop_tree.build(str(tmp_path), dset="tless", seed=31, n_scenes=2, n_views=2)
    with pytest.raises(ValueError, match="depth"):
        evaluator.Evaluator("tless", desc["data_root"], None, nviews=1, debug_gt_kp=True, out_dir=str(tmp_path / "none"), bop19=True, bop19_vsd=True)
    with pytest.raises(ValueError, match="bop19"):
        evaluator.Evaluator("tless", desc["data_root"], None, nviews=1, debug_gt_kp=True, out_dir=str(tmp_path / "none"), bop19_vsd=True)
    mesh = bop.load_mesh_db(os.path.join(desc["data_root"], "models_eval"), faces=True)
    VR.add_depth(desc, mesh, seed=9)
    ev = evaluator.Evaluator("tless", desc["data_root"], None, nviews=1, debug_gt_kp=True, out_dir=str(tmp_path / "on"), bop19=True, bop19_vsd=True)
    out = ev.run()
    got = out["bop19"]
    assert set(got) == BOP19_KEYS | {"vsd", "ar"} and set(out) == PARENT_KEYS | {"bop19"}

    meter = _cpu_meter(desc, out["csv_path"], mesh)
    vtable = meter.vsd_table(bop_eval.VSD_TAUS)
    es = np.array([e for ims in vtable.values() for objs in ims.values() for rows in objs.values() for r in rows for v in r["errors"].values() for e in v])
    print("VSD errors of the run:", len(es), "values, min", es.min(), "max", es.max(), "distance to a threshold", np.abs(es[:, None] - bop_eval.VSD_THRESHOLDS).min())
    # the recalls compare errors = ratios of pixel counts with thresholds: equal counts give equal errors, whatever their distance to a threshold
    want = meter.result()
    assert got["vsd"]["recalls"] == want["vsd"]["recalls"], (got["vsd"], want["vsd"])
    rec = np.array(got["vsd"]["recalls"])
    assert rec.shape == (10, 10) and rec.max() > 0
    assert got["vsd"]["ar"] == float(np.mean(rec)) == want["vsd"]["ar"]
    assert got["ar"] == float(np.mean([got["vsd"]["ar"], got["mssd"]["ar"], got["mspd"]["ar"]]))
    txt = open(out["summary_path"]).read()
    for name in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR"):
        assert txt.count(f"BOP-19 {name}:") == 1
    assert f"BOP-19 AR: {got['ar']:.4f}" in txt and f"BOP-19 AR_VSD: {got['vsd']['ar']:.4f}" in txt

    # bop19_vsd=False: exactly the keys and values of before, the depth images never read
    ev2 = evaluator.Evaluator("tless", desc["data_root"], None, nviews=1, debug_gt_kp=True, out_dir=str(tmp_path / "off"), bop19=True)
    ev2.dataset.read_depth = None
    out2 = ev2.run()
    assert set(out2["bop19"]) == BOP19_KEYS and out2["bop19"] == {k: got[k] for k in BOP19_KEYS}
    assert open(out2["csv_path"]).read() == open(out["csv_path"]).read()
    txt2 = open(out2["summary_path"]).read()
    assert "AR_VSD" not in txt2 and "BOP-19 AR:" not in txt2 and txt2.count("BOP-19 AR_MSSD:") == 1


def test_calls_split_into_runs_give_what_one_call_gives(monkeypatch):
    """BopErrors.vsd and Bop19Meter.vsd_table cut their pairs into runs of VSD_PAIRS_PER_CALL, each with the images it names re-indexed.  With runs of 3 --
    images shared within a run, across two runs and used once -- errors, counts and the table are those of a single call."""
    from tests.golden import vsd_cases as VC
    models = VC.models()
    mesh = {m + 1: {"points": models[m][1], "faces": models[m][2]} for m in range(len(models))}
    info = {m + 1: {"diameter": models[m][3]} for m in range(len(models))}
    be = bop_eval.BopErrors(mesh, info)
    pairs = VC.vsd_pairs()
    n = len(pairs)
    ids = [p["m"] + 1 for p in pairs]
    Te, Tg, K = np.stack([p["Te"] for p in pairs]), np.stack([p["Tg"] for p in pairs]), np.stack([p["K"] for p in pairs])
    images = [pairs[i]["test"] for i in (0, 3, 4, 10, 11)]
    image_index = [0, 0, 1, 1, 1, 2, 4, 4, 0, 3, 3, 2]                          # run 1 ends and run 2 begins on image 1; images 0 and 2 come back later
    monkeypatch.setattr(bop_eval, "VSD_PAIRS_PER_CALL", 64)
    e1, c1 = be.vsd(ids, Te, Tg, K, images, image_index, delta=VC.DELTA, taus=VC.TAUS, return_counts=True)
    monkeypatch.setattr(bop_eval, "VSD_PAIRS_PER_CALL", 3)
    e3, c3 = be.vsd(ids, Te, Tg, K, images, image_index, delta=VC.DELTA, taus=VC.TAUS, return_counts=True)
    assert np.array_equal(e1, e3) and np.array_equal(c1, c3) and (c1[:, 0] > 0).sum() >= 6 and len(np.unique(e1)) > 5
    for k in (2, 9):                                                            # and they are the numpy figures
        _, P, F, diam = models[pairs[k]["m"]]
        de, dg = VR.render_depth(P, F, Te[k], K[k], VC.W, VC.H), VR.render_depth(P, F, Tg[k], K[k], VC.W, VC.H)
        assert VR.vsd_from_depth(de, dg, images[image_index[k]], K[k], VC.DELTA, VC.TAUS, True, diam)[1] == c3[k].tolist()

    # the meter: image im holds the ground truths and estimates of the pairs that name it; every pair of an (image, object) is scored against every ground truth
    scene_gt, scene_gt_info, targets = {1: {}}, {1: {}}, []
    for im in range(len(images)):
        ks = [k for k in range(n) if image_index[k] == im]
        scene_gt[1][im] = [{"obj_id": ids[k], "cam_R_m2c": Tg[k][:, :3].ravel().tolist(), "cam_t_m2c": Tg[k][:, 3].tolist()} for k in ks]
        scene_gt_info[1][im] = [{"visib_fract": 0.9 - 0.01 * j} for j in range(len(ks))]
        for o in sorted({ids[k] for k in ks}):
            targets.append({"scene_id": 1, "im_id": im, "obj_id": o, "inst_count": sum(1 for k in ks if ids[k] == o)})
    loads = []

    def loader(s, im):
        loads.append(im)
        return images[im]
    tables = []
    for per_call in (64, 3):
        monkeypatch.setattr(bop_eval, "VSD_PAIRS_PER_CALL", per_call)
        del loads[:]
        meter = bop_eval.Bop19Meter(be, targets, scene_gt, scene_gt_info, VC.W, depth_loader=loader, vsd_delta=VC.DELTA)
        for k in range(n):
            meter.add(1, image_index[k], ids[k], 1.0 - 0.01 * k, Te[k], K[k])
        tables.append((meter.vsd_table(VC.TAUS), list(loads)))
    (t64, l64), (t3, l3) = tables
    assert t64 == t3
    n_pairs = sum(len(r["errors"]) for objs in t3[1].values() for rows in objs.values() for r in rows)
    assert n_pairs > n and sorted(l64) == sorted(set(l64)) and len(l3) > len(l64)      # more pairs than estimates; one load each in one call; an image straddling two runs is loaded again
    be.close()
