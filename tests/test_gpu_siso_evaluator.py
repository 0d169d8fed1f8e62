"""Evaluator(siso=True) end to end on the GPU (row N4): the synthetic T-LESS tree with depth images (tests/bop_tree.py + tests/vsd_ref.add_depth, 2 scenes x
2 views) through the hot path.  run()["siso"] -- the SISO recall of VSD with scripts/eval_siso.py's parameters -- consists of counts of matched targets and
must be what a LocalizationMeter over the numpy rasteriser and the numpy VSD (tests/points_errors_ref.RefSisoErrors) computes from the CSV the run wrote,
exactly; tools/eval_siso.py over that CSV must write the same scores; and without siso=True the run returns the keys and the CSV it returned before."""
import importlib.util
import json
import os

import numpy as np
import pytest

from suo_slam_amd import bop, bop_eval, evaluator
from tests import bop_tree
from tests import points_errors_ref as PR
from tests import vsd_ref as VR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_KEYS = {"method", "csv_path", "summary_path", "result", "saved_result", "num_views", "num_cam_poses_found", "fp16_range_reissues", "matrix_pipe_at_end",
               "bop_eval", "seconds"}
SCORE_KEYS = {"recall", "obj_recalls", "mean_obj_recall", "scene_recalls", "mean_scene_recall", "gt_count", "targets_count", "tp_count"}
PARAMETERS = {"error_type": "vsd", "n_top": 1, "visib_gt_min": 0.1, "correct_th": [0.3], "vsd_delta": 15, "vsd_tau": 20.0, "vsd_normalized_by_diameter": False}


def _cpu_meter(desc, csv_path, mesh):
    root, split = desc["data_root"], desc["split"]
    ds = bop.BopDataset(root, split, bop_dset="tless", ignore_symmetry=True)
    errs = PR.RefSisoErrors(mesh, bop_eval.load_models_info(os.path.join(root, "models_eval")))
    scenes = sorted(int(d) for d in os.listdir(os.path.join(root, split)) if d.isdigit())
    meter = bop_eval.LocalizationMeter.from_dataset_tree(errs, os.path.join(root, split), os.path.join(root, "all_target_tless.json"), depth_loader=ds.read_depth,
                                                         scene_ids=scenes, obj_ids=sorted(mesh), symmetric_obj_ids=[o for o, m in mesh.items() if m["is_symmetric"]],
                                                         **bop_eval.SISO_PARAMS)
    cams = {}
    for ln in open(csv_path).read().strip().split("\n"):
        s, v, o, score, R, t, _ = ln.split(",")
        s, v = int(s), int(v)
        if s not in cams:
            cams[s] = json.load(open(os.path.join(root, split, f"{s:06d}", "scene_camera.json")))
        T = np.hstack((np.array(R.split(), float).reshape(3, 3), np.array(t.split(), float).reshape(3, 1)))
        meter.add(s, v, int(o), float(score), T, np.array(cams[s][str(v)]["cam_K"]).reshape(3, 3))
    return meter


def test_siso_recall_of_a_run_equals_the_numpy_meter_on_its_csv(tmp_path):
    desc = bop_tree.build(str(tmp_path), dset="tless", seed=31, n_scenes=2, n_views=2)
    kw = dict(nviews=1, debug_gt_kp=True)
    with pytest.raises(ValueError, match="calc_scene_gt_info"):                # no depth/ yet
        evaluator.Evaluator("tless", desc["data_root"], None, out_dir=str(tmp_path / "none"), siso=True, **kw)
    mesh = bop.load_mesh_db(os.path.join(desc["data_root"], "models_eval"), faces=True)
    VR.add_depth(desc, mesh, seed=9)
    first = os.path.join(desc["data_root"], desc["split"], sorted(os.listdir(os.path.join(desc["data_root"], desc["split"])))[0], "scene_gt_info.json")
    os.rename(first, first + ".away")
    with pytest.raises(ValueError, match="scene_gt_info.json"):
        evaluator.Evaluator("tless", desc["data_root"], None, out_dir=str(tmp_path / "none"), siso=True, **kw)
    os.rename(first + ".away", first)

    ev = evaluator.Evaluator("tless", desc["data_root"], None, out_dir=str(tmp_path / "on"), siso=True, **kw)
    out = ev.run()
    got = out["siso"]
    assert set(out) == PARENT_KEYS | {"siso"} and set(got) == SCORE_KEYS | set(PARAMETERS)
    assert {k: got[k] for k in PARAMETERS} == PARAMETERS

    meter = _cpu_meter(desc, out["csv_path"], mesh)
    want = meter.result()
    es = [e[0] for recs in meter.error_records().values() for r in recs for e in r["errors"].values()]
    print("VSD errors of the run (numpy):", np.round(es, 4).tolist(), " scores:", want)
    assert {k: got[k] for k in SCORE_KEYS} == want
    assert got["recall"] > 0 and got["targets_count"] > 0 and got["tp_count"] == round(got["recall"] * got["targets_count"])
    txt = open(out["summary_path"]).read()
    assert txt.count("SISO VSD recall (tau 20, th 0.3, visib >= 0.1): ") == 1 and f"visib >= 0.1): {got['recall']:.4f} " in txt

    # the command line over the CSV the run wrote
    spec = importlib.util.spec_from_file_location("eval_siso_tool", os.path.join(ROOT, "tools", "eval_siso.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    written = tool.main(["--result_filenames", os.path.basename(out["csv_path"]), "--results_path", os.path.dirname(out["csv_path"]), "--eval_path",
                         str(tmp_path / "eval"), "--datasets_path", os.path.dirname(desc["data_root"]), "--targets_filename", "all_target_tless.json"])
    assert len(written) == 1 and written[0].endswith(os.path.join("error=vsd_ntop=1_delta=15.000_tau=20.000", "scores_th=0.300_min-visib=0.100.json"))
    scores = json.load(open(written[0]), object_hook=lambda d: {int(k) if k.isdigit() else k: v for k, v in d.items()})
    assert scores == want
    matches = json.load(open(written[0].replace("scores_", "matches_")))
    assert [(m["scene_id"], m["im_id"], m["gt_id"], m["est_id"], m["valid"], m["error"]) for m in matches] == \
        [(m["scene_id"], m["im_id"], m["gt_id"], m["est_id"], m["valid"], m["error"]) for m in meter.matches()]

    # siso=False: exactly the keys and the CSV of before, the depth images never read
    ev2 = evaluator.Evaluator("tless", desc["data_root"], None, out_dir=str(tmp_path / "off"), **kw)
    ev2.dataset.read_depth = None
    out2 = ev2.run()
    assert set(out2) == PARENT_KEYS and ev2.bop_errors is None and all("faces" not in m for m in ev2.mesh_db.values())
    assert open(out2["csv_path"]).read() == open(out["csv_path"]).read()
    assert "SISO" not in open(out2["summary_path"]).read() and out2["bop_eval"]["argv"][:2] == out["bop_eval"]["argv"][:2]
    with pytest.raises(ValueError, match="targets file"):
        evaluator.Evaluator("ycbv", desc["data_root"], None, out_dir=str(tmp_path / "none"), siso=True, **kw)
