"""scene_gt_info.json and the ground-truth masks of a BOP-format tree, from its raw annotations.

Stands in for bop_toolkit's ``scripts/calc_gt_info.py`` and ``scripts/calc_gt_masks.py``, whose OpenGL renderer was the only producer of the files that
bop.BopDataset, bop_eval.valid_gt_mask and Bop19Meter.from_dataset_tree read:

    format_scene_gt_info(info)                      the text inout.save_json writes for {im_id: [entry, ...]}
    calc_scene_gt_info(errors, split_dir, ...)      walks <split>/<scene>/: scene_camera.json, scene_gt.json, depth/%06d.png
                                                    -> BopErrors.gt_info / .gt_masks -> HIP, csrc/gt_info.hip (suo_gt_info, suo_gt_masks)
                                                    -> scene_gt_info.json, mask/%06d_%06d.png, mask_visib/%06d_%06d.png

``errors`` is a bop_eval.BopErrors over a mesh database with faces (bop.load_mesh_db(model_dir, faces=True)).  The readers are not changed: they read the
files this writes.  tools/calc_gt_info.py is the command line."""
from __future__ import annotations

import json
import os

import numpy as np

IMAGES_PER_CALL = 32                               # images of one device call: their depth (1.6 MB each at 720 x 540) is uploaded once per call
KEYS = ("bbox_obj", "bbox_visib", "px_count_all", "px_count_valid", "px_count_visib", "visib_fract")


def format_scene_gt_info(info):
    """The text ``inout.save_json(path, info)`` writes (inout.py:86-102): one line per image in ascending key order, each value through
    ``json.dumps(..., sort_keys=True)``, no trailing newline."""
    items = sorted(info.items(), key=lambda kv: kv[0])
    lines = ['  "{}": {}'.format(k, json.dumps(v, sort_keys=True)) + ("," if i != len(items) - 1 else "") for i, (k, v) in enumerate(items)]
    return "{\n" + "".join(ln + "\n" for ln in lines) + "}"


def read_depth(scene_dir, im_id, depth_scale):
    """float32 [H,W] mm of ``depth/%06d.png`` (``.tif`` first where it exists, as the script's fallback has it): the float32 product with ``depth_scale``
    exactly as bop.BopDataset.read_depth forms it."""
    from PIL import Image
    path = os.path.join(scene_dir, "depth", f"{im_id:06d}.tif")
    if not os.path.exists(path):
        path = path.replace(".tif", ".png")
    raw = np.asarray(Image.open(path))
    assert raw.ndim == 2 and raw.size > 0, f"{path}: not a single-channel depth image"
    return raw.astype(np.float32) * np.float32(depth_scale)


def _scene_ids(split_dir):
    return sorted(int(d) for d in os.listdir(split_dir) if d.isdigit() and os.path.isdir(os.path.join(split_dir, d)))


def calc_scene_gt_info(errors, split_dir, scene_ids=None, delta=15, masks=False, write=True, images_per_call=IMAGES_PER_CALL):
    """``{scene_id: {im_id: [entry, ...]}}`` for the scenes of ``split_dir`` (``scene_ids``: which; default all), an entry per ground truth of scene_gt.json
    in its order, with the toolkit's six keys.  ``masks``: also compute mask / mask_visib and, with ``write``, save them as 8-bit PNGs; ``write``: save
    scene_gt_info.json (and the PNGs).  ``images_per_call`` images of one size go into one device call."""
    out = {}
    for scene_id in (_scene_ids(split_dir) if scene_ids is None else scene_ids):
        sdir = os.path.join(split_dir, f"{int(scene_id):06d}")
        with open(os.path.join(sdir, "scene_camera.json"), "r") as f:
            cam = {int(k): v for k, v in json.load(f).items()}
        with open(os.path.join(sdir, "scene_gt.json"), "r") as f:
            gt = {int(k): v for k, v in json.load(f).items()}
        info = {im_id: [] for im_id in gt}
        if masks and write:
            for d in ("mask", "mask_visib"):
                os.makedirs(os.path.join(sdir, d), exist_ok=True)
        im_ids = sorted(gt)
        for b in range(0, len(im_ids), max(1, int(images_per_call))):
            batch, by_size = im_ids[b:b + max(1, int(images_per_call))], {}
            for im_id in batch:
                if gt[im_id]:
                    depth = read_depth(sdir, im_id, cam[im_id]["depth_scale"])
                    by_size.setdefault(depth.shape, []).append((im_id, depth))
            for group in by_size.values():                                      # one size per device call
                obj_ids, Ts, Ks, ii, where = [], [], [], [], []
                for k, (im_id, _) in enumerate(group):
                    K = np.array(cam[im_id]["cam_K"], np.float64).reshape(3, 3)
                    for gt_id, g in enumerate(gt[im_id]):
                        obj_ids.append(int(g["obj_id"]))
                        Ts.append(np.hstack((np.array(g["cam_R_m2c"], np.float64).reshape(3, 3), np.array(g["cam_t_m2c"], np.float64).reshape(3, 1))))
                        Ks.append(K)
                        ii.append(k)
                        where.append((im_id, gt_id))
                depths = [d for _, d in group]
                entries = errors.gt_info(obj_ids, np.stack(Ts), np.stack(Ks), depths, ii, delta)
                for (im_id, _), e in zip(where, entries):
                    info[im_id].append(e)
                if masks:
                    m, mv = errors.gt_masks(obj_ids, np.stack(Ts), np.stack(Ks), depths, ii, delta)
                    if write:
                        from PIL import Image
                        for (im_id, gt_id), a, av in zip(where, m, mv):
                            Image.fromarray(a).save(os.path.join(sdir, "mask", f"{im_id:06d}_{gt_id:06d}.png"))
                            Image.fromarray(av).save(os.path.join(sdir, "mask_visib", f"{im_id:06d}_{gt_id:06d}.png"))
        if write:
            with open(os.path.join(sdir, "scene_gt_info.json"), "w") as f:
                f.write(format_scene_gt_info(info))
        out[int(scene_id)] = info
    return out
