"""Pin the SISO evaluation (row N4) against the REFERENCE's vendored bop_toolkit (imported from /root/reference in the build container): its two scripts,
scripts/eval_calc_errors.py and scripts/eval_calc_scores.py, are run THEMSELVES, unmodified, with runpy.run_path on the small tree this generator writes
from tests/golden/siso_cases.py, once per recorded run (siso_cases.RUNS: vsd at tau 20 unnormalised, add, adi, ad, proj, cus and rete; n_top 1, -1 and 0; both
rules of visib_gt_min).  The toolkit's renderer needs OpenGL, so ``renderer.create_renderer`` returns a stub whose ``render_object`` draws with the numpy
rasteriser of tests/vsd_ref.py -- what is pinned is everything after the renderer.  The other stubs only point the scripts at the tree (dataset_params) and
stand in for the absent codecs (inout.load_depth: PIL; inout.load_ply: the seeded meshes).

Recorded (tests/golden/siso_golden.npz, results only): the parsed errors_*.json, matches_*.json and scores_*.json of every run as one JSON text, and the
direct calls of pose_error.add / adi / proj on siso_cases.point_pairs() and of pose_error.cus / cou_bb_proj on siso_cases.mask_pairs() (NaN where the
toolkit's cou_bb_proj raises: an empty mask).

    python tests/golden/make_siso_golden.py
"""
import contextlib
import io
import json
import os
import runpy
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TOOLKIT = "/root/reference/thirdparty/bop_toolkit"
sys.path.insert(0, ROOT)
sys.path.insert(0, TOOLKIT)
np.float = float                                  # the vendored toolkit predates numpy 1.24
for _absent in ("imageio", "png"):                # image codecs imported at the top of inout.py; replaced below where the scripts use them
    sys.modules.setdefault(_absent, types.ModuleType(_absent))

from bop_toolkit_lib import dataset_params, inout, misc, pose_error, renderer  # noqa: E402

from suo_slam_amd import bop_eval  # noqa: E402
from tests import vsd_ref as VR  # noqa: E402
from tests.golden import siso_cases as SC  # noqa: E402


class StubRenderer:
    def __init__(self, width, height, models):
        self.width, self.height, self.models = width, height, models

    def add_object(self, obj_id, model_path, **kwargs):
        assert obj_id - 1 in range(len(self.models))

    def render_object(self, obj_id, R, t, fx, fy, cx, cy):
        _, p, f, _ = self.models[obj_id - 1]
        K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
        return {"depth": VR.render_depth(p, f, np.hstack((R, np.reshape(t, (3, 1)))), K, self.width, self.height)}


def check_conditions(t, models):
    """What makes every recorded figure one that can be compared exactly: no VSD pixel decides within a rounding of delta or tau, no sample of a render of
    the mask pairs within the NEAR band of an edge, the designed situations present."""
    info = SC.scene_gt_info(t)
    fr = [e["visib_fract"] for e in info[1][0]]
    assert fr[0] > 0.9 and 0.0 < fr[2] < 0.1, fr                               # two instances of object 1, the second below 0.1 and not zero
    worst = (np.inf, np.inf)
    for e in t["ests"]:
        v = t["scenes"][e["scene_id"]][e["im_id"]]
        for o, Tg in v["gts"]:
            if o != e["obj_id"] or not bop_eval.overlapping_sphere_projections(0.5 * models[o - 1][3], e["T"][:, 3], Tg[:, 3]):
                continue
            de, dg = (VR.render_depth(models[o - 1][1], models[o - 1][2], T, v["K"], SC.W, SC.H) for T in (e["T"], Tg))
            m = VR.decision_margins(de, dg, SC.read_raw(v["raw"]), v["K"], SC.DELTA, SC.VSD["vsd_taus"], False, models[o - 1][3])
            assert m[0] > 1e-3 and m[1] > 1e-6, (e["scene_id"], e["im_id"], o, m)
            worst = (min(worst[0], m[0]), min(worst[1], m[1]))
    for lab, m, Te, Tg, K in SC.mask_pairs():
        for T in (Te, Tg):
            _, near = VR.render_depth(models[m][1], models[m][2], T, K, SC.W, SC.H, with_near=True)
            assert not near.any(), (lab, int(near.sum()))
    return worst


def run_script(name, argv):
    sys.argv = [name] + argv
    with contextlib.redirect_stdout(io.StringIO()):
        runpy.run_path(os.path.join(TOOLKIT, "scripts", name), run_name="__main__")


if __name__ == "__main__":
    from PIL import Image
    models = SC.models()
    t = SC.tree()
    print("conditions hold; smallest VSD margins (mm to delta, mm to tau):", check_conditions(t, models))
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        base = SC.write_tree(tmp, t)
        split = {"im_size": (SC.W, SC.H), "base_path": base, "scene_ids": list(SC.SCENE_IDS),
                 "scene_camera_tpath": os.path.join(base, "test", "{scene_id:06d}", "scene_camera.json"),
                 "scene_gt_tpath": os.path.join(base, "test", "{scene_id:06d}", "scene_gt.json"),
                 "scene_gt_info_tpath": os.path.join(base, "test", "{scene_id:06d}", "scene_gt_info.json"),
                 "depth_tpath": os.path.join(base, "test", "{scene_id:06d}", "depth", "{im_id:06d}.png")}
        dataset_params.get_split_params = lambda *a, **k: split
        dataset_params.get_model_params = lambda *a, **k: {"obj_ids": list(SC.OBJ_IDS), "symmetric_obj_ids": list(SC.SYMMETRIC_OBJ_IDS),
                                                           "model_tpath": os.path.join(base, "obj_{obj_id:06d}.ply"),
                                                           "models_info_path": os.path.join(base, "models_eval", "models_info.json")}
        renderer.create_renderer = lambda width, height, *a, **k: StubRenderer(width, height, models)
        inout.load_depth = lambda path: np.asarray(Image.open(path)).astype(np.float32)
        inout.load_ply = lambda path: {"pts": models[int(os.path.basename(path)[4:10]) - 1][1].astype(np.float64)}
        common = ["--eval_path", os.path.join(tmp, "eval"), "--datasets_path", os.path.join(tmp, "ds"), "--targets_filename", SC.TARGETS_FILENAME]
        done = set()
        for et, n_top, vmin, th in SC.RUNS:
            esign = misc.get_error_signature(et, n_top, vsd_delta=SC.DELTA, vsd_tau=SC.VSD["vsd_taus"][0])
            edir = os.path.join(tmp, "eval", SC.RESULT_NAME, esign)
            if (et, n_top) not in done:
                done.add((et, n_top))
                run_script("eval_calc_errors.py", common + ["--n_top", str(n_top), "--error_type", et, "--result_filenames", SC.RESULT_NAME + ".csv", "--results_path",
                                                            os.path.join(tmp, "results"), "--vsd_taus", ",".join(map(str, SC.VSD["vsd_taus"])),
                                                            "--vsd_normalized_by_diameter", ""])      # bool(""): the script's only way to say False
            argv = common + ["--error_dir_paths", os.path.join(SC.RESULT_NAME, esign), "--visib_gt_min", str(vmin)]
            if th is not None:
                argv += ["--correct_th_" + et, ",".join(map(str, th))]
            run_script("eval_calc_scores.py", argv)
            th_used = bop_eval.CORRECT_TH[et] if th is None else th
            ssign = misc.get_score_signature(th_used, vmin)
            rec = {"error_type": et, "n_top": n_top, "visib_gt_min": vmin, "correct_th": th, "error_sign": esign, "score_sign": ssign,
                   "errors": {str(s): inout.load_json(os.path.join(edir, f"errors_{s:06d}.json")) for s in SC.SCENE_IDS},
                   "matches": inout.load_json(os.path.join(edir, f"matches_{ssign}.json")), "scores": inout.load_json(os.path.join(edir, f"scores_{ssign}.json"))}
            runs.append(rec)
            print(f"{et:5s} n_top {n_top:2d} visib {vmin:4} th {th}: recall {rec['scores']['recall']:.3f} targets {rec['scores']['targets_count']} "
                  f"tp {rec['scores']['tp_count']} gt {rec['scores']['gt_count']}")
    out = {"runs": np.frombuffer(json.dumps(runs, sort_keys=True).encode(), np.uint8)}

    pm = SC.point_models()
    direct = []
    for m, Te, Tg, K in SC.point_pairs():
        pts = pm[m].astype(np.float64)
        a = (Te[:, :3], Te[:, 3:], Tg[:, :3], Tg[:, 3:])
        direct.append([pose_error.add(*a, pts), pose_error.adi(*a, pts), pose_error.proj(*a, K, pts)])
    out["points"] = np.array(direct, np.float64)
    ren = StubRenderer(SC.W, SC.H, models)
    masks = []
    for lab, m, Te, Tg, K in SC.mask_pairs():
        a = (Te[:, :3], Te[:, 3:], Tg[:, :3], Tg[:, 3:], K, ren, m + 1)
        try:
            bb = pose_error.cou_bb_proj(*a)
        except ValueError:                                                     # min() of an empty array: an empty mask
            bb = np.nan
        masks.append([pose_error.cus(*a), bb])
        print(f"{lab:22s} cus {masks[-1][0]:.4f} cou_bb_proj {masks[-1][1]:.4f}")
    out["masks"] = np.array(masks, np.float64)
    path = os.path.join(ROOT, "tests", "golden", "siso_golden.npz")
    np.savez_compressed(path, **out)
    print("recorded", {k: v.shape for k, v in out.items()}, os.path.getsize(path), "bytes")
