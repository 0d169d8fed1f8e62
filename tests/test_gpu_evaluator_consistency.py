"""Evaluator(consistency=True) end to end on the GPU: the synthetic T-LESS tree (discrete and continuous symmetries) through the hot path.  The option reports
run()["consistency"] and three lines of summary.txt and changes nothing else; off, everything is what it was.  No statement about the values: the synthetic
network weights are random."""
import numpy as np
import pytest

from suo_slam_amd import bop_eval, evaluator
from tests import bop_tree

pytestmark = pytest.mark.gpu

PARENT_KEYS = {"method", "csv_path", "summary_path", "result", "saved_result", "num_views", "num_cam_poses_found", "fp16_range_reissues", "matrix_pipe_at_end",
               "bop_eval", "seconds"}
FIVE = {"n", "n_nan", "mean_nees", "frac_95", "frac_99"}


def _body(txt):
    return [ln for ln in txt.split("\n") if "TIMING" not in ln]                # (wall-clock lines differ between any two runs)


def test_consistency_reports_and_changes_nothing_else(tmp_path, monkeypatch):
    desc = bop_tree.build(str(tmp_path), dset="tless", seed=31, n_scenes=2, n_views=2)
    reached = []
    real_update = evaluator.EvalMeter.update

    ev = evaluator.Evaluator("tless", desc["data_root"], None, nviews=1, debug_gt_kp=True, out_dir=str(tmp_path / "on"), consistency=True, do_add=True)
    monkeypatch.setattr(evaluator.EvalMeter, "update", lambda self, ids, *a, **k: (reached.extend(ids), real_update(self, ids, *a, **k))[1])
    out = ev.run()
    monkeypatch.undo()
    c = out["consistency"]
    assert set(out) == PARENT_KEYS | {"consistency"} and set(c) == {"pose", "keypoint"}
    assert set(c["pose"]) == FIVE | {"per_object", "n_skipped_continuous"}
    assert set(c["keypoint"]) == {"n", "n_nan", "n_skipped", "mean_chi2", "frac_95", "frac_99"}
    info = bop_eval.load_models_info(f"{desc['data_root']}/models_eval")
    n_cont = sum(1 for o in reached if info[int(o)].get("symmetries_continuous"))
    assert len(reached) > 0 and n_cont > 0
    assert c["pose"]["n_skipped_continuous"] == n_cont and c["pose"]["n"] == len(reached) - n_cont
    assert sum(v["n"] for v in c["pose"]["per_object"].values()) == c["pose"]["n"] and all(set(v) == FIVE for v in c["pose"]["per_object"].values())
    assert not any(info[int(o)].get("symmetries_continuous") for o in c["pose"]["per_object"])
    # debug_gt_kp replaces the network's keypoints on the host route, which carries no covariance: every detection is skipped and counted
    assert c["keypoint"]["n"] == 0 and c["keypoint"]["n_skipped"] == len(reached)
    txt = open(out["summary_path"]).read()
    assert txt.count("Consistency, poses:") == 1 and txt.count("Consistency, poses per object") == 1 and txt.count("Consistency, keypoints:") == 1

    # off: the parent's keys, CSV and summary; models_info.json is never read
    def boom(*a, **k):
        raise AssertionError("consistency=False must not read models_info")
    monkeypatch.setattr(bop_eval, "load_models_info", boom)
    ev2 = evaluator.Evaluator("tless", desc["data_root"], None, nviews=1, debug_gt_kp=True, out_dir=str(tmp_path / "off"), do_add=True)
    out2 = ev2.run()
    assert set(out2) == PARENT_KEYS and ev2.bop_errors is None
    assert open(out2["csv_path"], "rb").read() == open(out["csv_path"], "rb").read()
    txt2 = open(out2["summary_path"]).read()
    assert "Consistency" not in txt2
    body, body2 = [ln for ln in _body(txt) if not ln.startswith("Consistency")], _body(txt2)
    while body and body[-1] == "":
        body.pop()
    while body2 and body2[-1] == "":
        body2.pop()
    assert body[:len(body2)] == body2 and all(ln == "" for ln in body[len(body2):])
    assert repr(out2["result"]) == repr(out["result"])


def test_keypoints_of_the_network_route_are_counted(tmp_path):
    """Saved detections through the network and the device chain (view_chain.py fills the detection dicts): the keypoints carry the network's covariances."""
    from suo_slam_amd import bop, weights
    desc = bop_tree.build(str(tmp_path), dset="tless", seed=31, n_scenes=2, n_views=2)
    reader = bop.BopDataset(desc["data_root"], desc["split"], bop_dset="tless", ignore_symmetry=True)
    bop_tree.write_saved_detections_pix2pose(str(tmp_path), desc, reader, seed=4)
    sd = weights.make_random_state_dict(seed=0, logit_gain=8.0)
    sd["classifier.2.bias"] = (np.asarray(sd["classifier.2.bias"]) + 4.0).astype(np.float32)       # "visible", as tests/test_gpu_tless.py
    outs = []
    for on in (True, False):
        ev = evaluator.Evaluator("tless", desc["data_root"], None, nviews=1, detection_type="saved", out_dir=str(tmp_path / f"out{int(on)}"), state_dict=sd,
                                 consistency=on)
        outs.append(ev.run())
    assert open(outs[0]["csv_path"], "rb").read() == open(outs[1]["csv_path"], "rb").read() and "consistency" not in outs[1]
    c = outs[0]["consistency"]
    n_poses = c["pose"]["n"] + c["pose"]["n_skipped_continuous"]
    assert n_poses > 0 and c["keypoint"]["n_skipped"] == 0 and c["keypoint"]["n"] >= 4 * n_poses
    assert c["keypoint"]["n_nan"] <= c["keypoint"]["n"]


def test_consistency_refuses_the_batched_route(tmp_path):
    desc = bop_tree.build(str(tmp_path), dset="ycbv", seed=2, n_scenes=1, n_views=2)
    with pytest.raises(ValueError, match="frames_per_call"):
        evaluator.Evaluator("ycbv", desc["data_root"], None, nviews=1, debug_gt_kp=True, out_dir=str(tmp_path / "out"), consistency=True, frames_per_call=2)
