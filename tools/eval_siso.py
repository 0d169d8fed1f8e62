"""SISO evaluation of a BOP results file, in process (row N4): what bop_toolkit's scripts/eval_siso.py does by driving eval_calc_errors.py and
eval_calc_scores.py -- errors of every estimate against the ground truths, greedy matching, recall -- over suo_slam_amd.bop_eval.LocalizationMeter and the
HIP kernels instead of the toolkit's OpenGL renderer.  The defaults are eval_siso.py's: VSD at tau 20 (not normalised by the diameter), threshold 0.3,
n_top 1, ground truths with visib_fract >= 0.1.

    python tools/eval_siso.py --result_filenames <method>_<dataset>-<split>.csv --results_path <dir> --eval_path <dir> --datasets_path <bop root>
                              --targets_filename all_target_tless.json [--error_type adi --n_top 1 --visib_gt_min 0.1 --correct_th 0.1]

Writes, with the toolkit's signatures and its JSON layout, under <eval_path>/<result name>/<error signature>/:
    errors_%06d.json (one per scene of the targets), matches_<score signature>.json, scores_<score signature>.json
and prints one line per results file."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from suo_slam_amd import bop, bop_eval, bop_gt_info  # noqa: E402

MODEL_DIRS = {"tless": "models_eval", "ycbv": "models_bop-compat_eval"}


def save_json(path, content):
    """inout.save_json (inout.py:86-114): one line per element of a list or per key of a dictionary, each through json.dumps(..., sort_keys=True)."""
    with open(path, "w") as f:
        if isinstance(content, dict):
            items = sorted(content.items(), key=lambda x: x[0])
            f.write("{\n" + "".join('  "{}": {}'.format(k, json.dumps(v, sort_keys=True)) + ("," if i != len(items) - 1 else "") + "\n"
                                    for i, (k, v) in enumerate(items)) + "}")
        else:
            f.write("[\n" + "".join("  {}".format(json.dumps(e, sort_keys=True)) + ("," if i != len(content) - 1 else "") + "\n" for i, e in enumerate(content)) + "]")


def load_results(path):
    """inout.load_bop_results (inout.py:222-262): ``[(scene_id, im_id, obj_id, score, T [3,4])]`` in the file's order; a header line is skipped."""
    out = []
    with open(path, "r") as f:
        for k, line in enumerate(f):
            if not line.strip() or (k == 0 and "scene_id,im_id,obj_id,score,R,t,time" in line):
                continue
            e = line.split(",")
            if len(e) != 7:
                raise ValueError("A line does not have 7 comma-sep. elements: {}".format(line))
            T = np.hstack((np.array(list(map(float, e[4].split()))).reshape(3, 3), np.array(list(map(float, e[5].split()))).reshape(3, 1)))
            out.append((int(e[0]), int(e[1]), int(e[2]), float(e[3]), T))
    return out


def split_dir_of(datasets_path, result_name):
    """(dataset, its folder, the split's folder) from ``<method>_<dataset>-<split>[-<split type>]`` (eval_calc_errors.py:142-149); the method may hold no
    underscore.  T-LESS's ``test`` is ``test_primesense``, the toolkit's default split type for it."""
    info = result_name.split("_")
    d = info[1].split("-")
    dataset, split, split_type = d[0], d[1], (d[2] if len(d) > 2 else None)
    base = os.path.join(datasets_path, dataset)
    for cand in ([f"{split}_{split_type}"] if split_type else []) + [split, "_".join([split] + info[2:])] + (["test_primesense"] if dataset == "tless" else []):
        if os.path.isdir(os.path.join(base, cand)):
            return dataset, base, os.path.join(base, cand)
    raise ValueError(f"no folder of split {split!r} under {base}")


def evaluate(result_filename, a, errors_cache):
    result_name = os.path.splitext(os.path.basename(result_filename))[0]
    dataset, base, split_dir = split_dir_of(a.datasets_path, result_name)
    model_dir = a.model_dir or os.path.join(base, MODEL_DIRS.get(dataset, "models_eval"))
    if model_dir not in errors_cache:
        mesh = bop.load_mesh_db(model_dir, faces=True)
        errors_cache[model_dir] = (bop_eval.BopErrors(mesh, bop_eval.load_models_info(model_dir)), mesh)
    errors, mesh = errors_cache[model_dir]
    cams = {}

    def cam(s):
        if s not in cams:
            with open(os.path.join(split_dir, f"{s:06d}", "scene_camera.json"), "r") as f:
                cams[s] = {int(k): v for k, v in json.load(f).items()}
        return cams[s]

    def depth(s, im):
        return bop_gt_info.read_depth(os.path.join(split_dir, f"{s:06d}"), im, cam(s)[im]["depth_scale"])
    targets_path = os.path.join(base, a.targets_filename)
    with open(targets_path, "r") as f:
        first = json.load(f)[0]
    H, W = depth(first["scene_id"], first["im_id"]).shape if a.error_type in ("vsd", "cus") else (None, a.im_width)
    th = bop_eval.CORRECT_TH[a.error_type] if a.correct_th is None else [float(t) for t in a.correct_th.split(",")]
    scene_ids = sorted(int(d) for d in os.listdir(split_dir) if d.isdigit() and os.path.isdir(os.path.join(split_dir, d)))
    meter = bop_eval.LocalizationMeter.from_dataset_tree(
        errors, split_dir, targets_path, error_type=a.error_type, n_top=a.n_top, visib_gt_min=a.visib_gt_min, correct_th=th,
        vsd_delta=bop_eval.VSD_DELTAS.get(dataset, 15) if a.vsd_delta is None else a.vsd_delta, vsd_taus=[float(t) for t in a.vsd_taus.split(",")],
        vsd_normalized_by_diameter=a.vsd_normalized_by_diameter, symmetric_obj_ids=[o for o, m in mesh.items() if m["is_symmetric"]],
        im_width=W or a.im_width, im_hw=(H, W) if H else None, depth_loader=depth, scene_ids=scene_ids, obj_ids=sorted(mesh))
    for s, im, o, score, T in load_results(os.path.join(a.results_path, result_filename)):
        if s in meter.targets and im in meter.targets[s]:
            meter.add(s, im, o, score, T, np.array(cam(s)[im]["cam_K"], np.float64).reshape(3, 3))
    written = []
    for t in range(len(meter.vsd_taus) if a.error_type == "vsd" else 1):
        out_dir = os.path.join(a.eval_path, result_name, meter.error_sign(t))
        os.makedirs(out_dir, exist_ok=True)
        for s in meter.targets:
            save_json(os.path.join(out_dir, f"errors_{s:06d}.json"), meter.errors_json(s, t))
        scores = meter.result(t)
        save_json(os.path.join(out_dir, f"matches_{meter.score_sign()}.json"), meter.matches(t))
        save_json(os.path.join(out_dir, f"scores_{meter.score_sign()}.json"), scores)
        print(f"{result_name} {meter.error_sign(t)} {meter.score_sign()}: recall {scores['recall']:.4f} ({scores['tp_count']} of {scores['targets_count']} targets), "
              f"mean object recall {scores['mean_obj_recall']:.4f}, mean scene recall {scores['mean_scene_recall']:.4f}")
        written.append(os.path.join(out_dir, f"scores_{meter.score_sign()}.json"))
    return written


def main(argv=None):
    p = bop_eval.SISO_PARAMS
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--result_filenames", required=True, help="comma-separated names of results files, <method>_<dataset>-<split>.csv")
    ap.add_argument("--results_path", default="", help="folder of the results files")
    ap.add_argument("--eval_path", required=True, help="folder for the errors, matches and scores")
    ap.add_argument("--datasets_path", required=True, help="folder of the BOP datasets (holds <dataset>/)")
    ap.add_argument("--targets_filename", default="test_targets_bop19.json", help="file with the estimation targets, in the dataset's folder")
    ap.add_argument("--error_type", default=p["error_type"], choices=bop_eval.ERROR_TYPES)
    ap.add_argument("--n_top", type=int, default=p["n_top"], help="estimates per (image, object): k, 0 = all, -1 = the target's inst_count")
    ap.add_argument("--visib_gt_min", type=float, default=p["visib_gt_min"], help="least visible fraction of a valid ground truth; -1: the inst_count most visible")
    ap.add_argument("--correct_th", default=None, help="comma-separated thresholds of correctness, one per error element; default: the toolkit's for the error type")
    ap.add_argument("--vsd_delta", type=float, default=None, help="default: the dataset's (15 mm, ITODD 5)")
    ap.add_argument("--vsd_taus", default=",".join(str(t) for t in p["vsd_taus"]))
    ap.add_argument("--vsd_normalized_by_diameter", action="store_true")
    ap.add_argument("--model_dir", default=None, help="folder with models_info.json and obj_%%06d.ply; default: the dataset's evaluation models")
    ap.add_argument("--im_width", type=float, default=640.0, help="image width, for the normalisation of mspd")
    a = ap.parse_args(argv)
    cache, written = {}, []
    try:
        for name in a.result_filenames.split(","):
            written += evaluate(name, a, cache)
    finally:
        for errors, _ in cache.values():
            errors.close()
    return written


if __name__ == "__main__":
    main()
