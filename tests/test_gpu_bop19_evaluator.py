"""Evaluator(bop19=True) end to end on the GPU (row N5): the synthetic T-LESS tree (discrete and continuous symmetries, a targets file, a ground truth under
10 % visibility) through the hot path; the BOP-19 MSSD / MSPD recalls it reports must be the ones a Bop19Meter over the numpy restatement computes from the
CSV it wrote."""
import json
import os

import numpy as np
import pytest

from suo_slam_amd import bop, bop_eval, evaluator
from tests import bop_errors_ref as REF
from tests import bop_tree

pytestmark = pytest.mark.gpu

PARENT_KEYS = {"method", "csv_path", "summary_path", "result", "saved_result", "num_views", "num_cam_poses_found", "fp16_range_reissues", "matrix_pipe_at_end",
               "bop_eval", "seconds"}


def _cpu_meter(desc, csv_path):
    root, split = desc["data_root"], desc["split"]
    info = bop_eval.load_models_info(os.path.join(root, "models_eval"))
    errs = REF.RefErrors(bop.load_mesh_db(os.path.join(root, "models_eval")), info)
    meter = bop_eval.Bop19Meter.from_dataset_tree(errs, os.path.join(root, split), os.path.join(root, "all_target_tless.json"), 640)
    cams = {}
    for ln in open(csv_path).read().strip().split("\n"):
        s, v, o, score, R, t, _ = ln.split(",")
        s, v = int(s), int(v)
        if s not in cams:
            cams[s] = json.load(open(os.path.join(root, split, f"{s:06d}", "scene_camera.json")))
        T = np.hstack((np.array(R.split(), float).reshape(3, 3), np.array(t.split(), float).reshape(3, 1)))
        meter.add(s, v, int(o), float(score), T, np.array(cams[s][str(v)]["cam_K"]).reshape(3, 3))
    return meter


def test_bop19_recalls_of_a_run_equal_the_cpu_meter_on_its_csv(tmp_path, monkeypatch):
    desc = bop_tree.build(str(tmp_path), dset="tless", seed=31, n_scenes=2, n_views=2)
    ev = evaluator.Evaluator("tless", desc["data_root"], None, nviews=1, debug_gt_kp=True, out_dir=str(tmp_path / "on"), bop19=True)
    out = ev.run()
    got = out["bop19"]
    meter = _cpu_meter(desc, out["csv_path"])
    table = meter.normalised(meter.error_table())
    # the condition under which the recalls must agree exactly: no normalised error within 1e-6 (relative) of a threshold
    for which, ths in ((0, bop_eval.MSSD_THRESHOLDS), (1, bop_eval.MSPD_THRESHOLDS)):
        es = np.array([e[which] for ims in table.values() for objs in ims.values() for rows in objs.values() for r in rows for e in r["errors"].values()])
        es = es[np.isfinite(es)]
        assert len(es) > 0 and (np.abs(es[:, None] - ths[None, :]) > 1e-6 * ths[None, :]).all()
    want = meter.result()
    assert got == want, (got, want)
    n_lines = len(open(out["csv_path"]).read().strip().split("\n"))
    assert got["n_estimates"] == n_lines > 0 and got["n_targets"] > n_lines          # the target under 10 % visibility has no estimate and still counts
    assert max(got["mssd"]["recalls"]) > 0 and max(got["mspd"]["recalls"]) > 0
    assert got["mssd"]["ar"] == float(np.mean(got["mssd"]["recalls"])) and len(got["mspd"]["recalls"]) == 10
    txt = open(out["summary_path"]).read()
    assert txt.count("BOP-19 AR_MSSD:") == 1 and txt.count("BOP-19 AR_MSPD:") == 1 and f"{got['mssd']['ar']:.4f}" in txt
    assert set(out) == PARENT_KEYS | {"bop19"}

    # the default: nothing differs from before -- same keys, same CSV, no BOP-19 lines, models_info.json never read by the new module
    def boom(*a, **k):
        raise AssertionError("bop19=False must not read models_info")
    monkeypatch.setattr(bop_eval, "load_models_info", boom)
    ev2 = evaluator.Evaluator("tless", desc["data_root"], None, nviews=1, debug_gt_kp=True, out_dir=str(tmp_path / "off"))
    out2 = ev2.run()
    assert set(out2) == PARENT_KEYS and ev2.bop_errors is None
    assert open(out2["csv_path"]).read() == open(out["csv_path"]).read()
    txt2 = open(out2["summary_path"]).read()
    assert "BOP-19" not in txt2
    strip = lambda t: [ln for ln in t.split("\n") if not ln.startswith("BOP-19") and "TIMING" not in ln]      # noqa: E731
    body, body2 = strip(txt), strip(txt2)
    while body and body[-1] == "":
        body.pop()
    while body2 and body2[-1] == "":
        body2.pop()
    assert body[:len(body2)] == body2


def test_bop19_needs_a_targets_file(tmp_path):
    desc = bop_tree.build(str(tmp_path), dset="ycbv", seed=2, n_scenes=1, n_views=1)
    with pytest.raises(ValueError, match="targets file"):
        evaluator.Evaluator("ycbv", desc["data_root"], None, nviews=1, debug_gt_kp=True, out_dir=str(tmp_path / "out"), bop19=True)
