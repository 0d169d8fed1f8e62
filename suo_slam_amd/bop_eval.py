"""BOP-19 average recall: MSSD / MSPD, the renderer-free two of the three terms of the BOP-19 score, and, opt-in, VSD (row N6).

Host mirror of what the reference's vendored bop_toolkit does between a results CSV and the two recall tables
(``scripts/eval_bop19.py`` driving ``eval_calc_errors.py`` and ``eval_calc_scores.py``) for the error types ``mssd`` and ``mspd``:

    symmetry_transformations(model_info, step)      misc.get_symmetry_transformations + transform.rotation_matrix
    load_models_info(model_dir)                     inout.load_json(models_info.json, keys_to_int=True)
    BopErrors(mesh_db, models_info).errors(...)     pose_error.mssd / pose_error.mspd          -> HIP, csrc/eval_bop.hip (suo_pose_errors_bop)
    Bop19Meter(errors, targets, scene_gt, scene_gt_info, im_width)
        .add(scene_id, im_id, obj_id, score, T_est, K) / .result()
                                                    eval_calc_errors.py:196-325 (n_top = -1, the sphere gate of MSSD),
                                                    eval_calc_scores.py:205-268 (visib_gt_min = -1, the two normalisations),
                                                    pose_matching.match_poses / match_poses_scene, score.calc_localization_scores

The max-over-points inside min-over-symmetries runs on the GPU in fp64; sorting, greedy matching and counting are a few thousand scalars and stay on the
host exactly as in the toolkit.  VSD, the third term, needs a renderer and depth images and stays the external hand-off of row N4 unless opted in, below.

Opt-in since row N6, with nothing above changed when it is not asked for: a mesh database with ``"faces"`` (bop.load_mesh_db(..., faces=True)) and a
``depth_loader`` give the third term without an external tool:

    BopErrors.pose_nees / .keypoint_nees            consistency figures of reported covariances (consistency.py) -> HIP, csrc/eval_nees.hip
    BopErrors.render_depth(obj_ids, T, K, hw)       Renderer.render_object(...)["depth"]       -> HIP, csrc/raster.hip (suo_render_depth)
    BopErrors.vsd(obj_ids, T_est, T_gt, K, depth_images, image_index, delta, taus, normalized)
                                                    pose_error.vsd (cost 'step', mode 'bop19')  -> HIP, csrc/eval_vsd.hip (suo_pose_errors_vsd)
    BopErrors.gt_info / .gt_masks(obj_ids, T_gt, K, depth_images, image_index, delta)
                                                    scripts/calc_gt_info.py, calc_gt_masks.py   -> HIP, csrc/gt_info.hip (row N7; bop_gt_info.py walks a tree)
    overlapping_sphere_projections(radius, p1, p2)  misc.overlapping_sphere_projections (the gate of eval_calc_errors.py:295-312)
    Bop19Meter(..., depth_loader=..., vsd_delta=15) adds "vsd" (one recall per tau and threshold, eval_bop19.py:178-225) and "ar", the mean of the three.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os

import numpy as np

from . import _lib

MSSD_THRESHOLDS = np.arange(0.05, 0.51, 0.05)          # eval_bop19.py:44, fractions of the object diameter
MSPD_THRESHOLDS = np.arange(5, 51, 5)                  # eval_bop19.py:49, pixels at an image width of 640
VSD_TAUS = VSD_THRESHOLDS = np.arange(0.05, 0.51, 0.05)  # eval_bop19.py:37,39: misalignment tolerances (fractions of the diameter) and thresholds of correctness
VSD_DELTAS = {"hb": 15, "icbin": 15, "icmi": 15, "itodd": 5, "lm": 15, "lmo": 15, "ruapc": 15, "tless": 15, "tudl": 15, "tyol": 15, "ycbv": 15}   # eval_bop19.py:24-36, mm
VSD_PAIRS_PER_CALL = 32                                # pairs of one device call: two 640 x 480 renders each stay on the device, 2.4 MB a pair


# ---- symmetries ------------------------------------------------------------------------------------------
def _rotation_matrix(angle, direction):
    """3x3 rotation about ``direction`` through the origin, with the arithmetic of transform.rotation_matrix (transform.py:327-336)."""
    sina, cosa = math.sin(angle), math.cos(angle)
    d = np.array(direction[:3], dtype=np.float64, copy=True)
    d /= math.sqrt(np.dot(d, d))
    R = np.diag([cosa, cosa, cosa])
    R += np.outer(d, d) * (1.0 - cosa)
    d *= sina
    R += np.array([[0.0, -d[2], d[1]], [d[2], 0.0, -d[0]], [-d[1], d[0], 0.0]])
    return R


def symmetry_transformations(model_info, max_sym_disc_step=0.01):
    """The set of symmetry transformations of one model, ``[S,3,4]`` rows [R|t], in the toolkit's order (misc.py:43-91): the identity and the discrete
    symmetries, each combined with the rotations i * 2 pi / ceil(pi / step), i >= 1, about every continuous axis.  With a continuous symmetry the
    un-rotated transformations themselves are NOT in the set (the toolkit's loop starts at i = 1): 314 - 1 per discrete one at step 0.01."""
    disc = [(np.eye(3), np.zeros((3, 1)))]
    for sym in model_info.get("symmetries_discrete", []):
        M = np.reshape(sym, (4, 4))
        disc.append((M[:3, :3], M[:3, 3].reshape((3, 1))))
    cont = []
    for sym in model_info.get("symmetries_continuous", []):
        axis = np.array(sym["axis"])
        offset = np.array(sym["offset"]).reshape((3, 1))
        steps = int(np.ceil(np.pi / max_sym_disc_step))
        step = 2.0 * np.pi / steps
        for i in range(1, steps):
            R = _rotation_matrix(i * step, axis)
            cont.append((R, -R.dot(offset) + offset))
    out = []
    for Rd, td in disc:
        if cont:
            for Rc, tc in cont:
                out.append(np.hstack((Rc.dot(Rd), Rc.dot(td) + tc)))
        else:
            out.append(np.hstack((Rd, td)))
    return np.array(out, dtype=np.float64).reshape(len(out), 3, 4)


def load_models_info(model_dir):
    """``{obj_id: models_info.json entry}`` with integer keys (diameter, symmetries_discrete, symmetries_continuous, ...)."""
    with open(os.path.join(model_dir, "models_info.json"), "r") as f:
        return {int(k): v for k, v in json.load(f).items()}


# ---- errors on the device ---------------------------------------------------------------------------------
def _pack34(T, n):
    if hasattr(T, "detach"):
        T = T.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(T, np.float64).reshape(n, -1, 4)[:, :3, :]).reshape(n, 12)


class BopErrors:
    """Owns a mesh database handle with the models' symmetry transformations.  ``mesh_db``: ``{obj_id: {"points": [P,3] mm, ...}}`` (bop.load_mesh_db);
    ``models_info``: ``{obj_id: {...}}`` (load_models_info).  No CPU fallback: without the HIP library or a GPU this raises."""

    def __init__(self, mesh_db, models_info, max_sym_disc_step=0.01):
        self.lib = _lib.lib()
        _lib.require_gpu()
        self.models_info = models_info
        self.max_sym_disc_step = max_sym_disc_step
        ids = list(mesh_db.keys())
        self._index = {o: i for i, o in enumerate(ids)}
        clouds = []
        for o in ids:
            p = mesh_db[o]["points"]
            if hasattr(p, "detach"):
                p = p.detach().cpu().numpy()
            clouds.append(np.ascontiguousarray(p, np.float32).reshape(-1, 3))
        self.syms = {o: symmetry_transformations(models_info[o], max_sym_disc_step) for o in ids}
        n_pts = np.array([c.shape[0] for c in clouds], np.int32)
        allpts = np.ascontiguousarray(np.concatenate(clouds, 0))
        h = C.c_void_p()
        _lib.check(self.lib.suo_mesh_db_create(len(clouds), n_pts.ctypes.data, allpts.ctypes.data, C.byref(h)), "suo_mesh_db_create")
        self._h = h
        n_sym = np.array([self.syms[o].shape[0] for o in ids], np.int32)
        allsym = np.ascontiguousarray(np.concatenate([self.syms[o].reshape(-1, 12) for o in ids], 0))
        _lib.check(self.lib.suo_mesh_db_set_symmetries(self._h, n_sym.ctypes.data, allsym.ctypes.data), "suo_mesh_db_set_symmetries")
        self.has_faces = any("faces" in mesh_db[o] for o in ids)
        if self.has_faces:                                          # the triangles of the VSD renderer; a model without them cannot be rendered
            tris = [np.ascontiguousarray(mesh_db[o].get("faces", np.zeros((0, 3))), np.int32).reshape(-1, 3) for o in ids]
            n_faces = np.array([t.shape[0] for t in tris], np.int32)
            allf = np.ascontiguousarray(np.concatenate(tris, 0))
            if allf.size == 0:
                allf = np.zeros((1, 3), np.int32)
            _lib.check(self.lib.suo_mesh_db_set_faces(self._h, n_faces.ctypes.data, allf.ctypes.data), "suo_mesh_db_set_faces")

    def close(self):
        if getattr(self, "_h", None) is not None:
            self.lib.suo_mesh_db_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def errors(self, obj_ids, T_est, T_gt, K):
        """(MSSD[n] in mm, MSPD[n] in px) of n (object, estimated pose, ground-truth pose, camera matrix) items; poses [n,3|4,4], K [n,3,3] or one [3,3]."""
        n = len(obj_ids)
        mssd, mspd = np.zeros(n, np.float64), np.zeros(n, np.float64)
        if n == 0:
            return mssd, mspd
        idx = np.array([self._index[int(o)] for o in obj_ids], np.int32)
        Te, Tg = _pack34(T_est, n), _pack34(T_gt, n)
        Kn = np.ascontiguousarray(np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 3, 3), (n, 3, 3))).reshape(n, 9)
        _lib.check(self.lib.suo_pose_errors_bop(self._h, n, idx.ctypes.data, Te.ctypes.data, Tg.ctypes.data, Kn.ctypes.data, mssd.ctypes.data, mspd.ctypes.data),
                   "suo_pose_errors_bop")
        return mssd, mspd

    def pose_nees(self, obj_ids, T_est, T_gt, cov):
        """NEES of n (object, estimated pose, ground-truth pose, 6x6 covariance) items against T_ref = T_gt S of the MSSD-minimising symmetry:
        ``{"nees", "xi", "sym_index", "T_ref", "n_nan"}`` (consistency.pose_nees; include/suo_hip.h: suo_pose_nees)."""
        from . import consistency
        return consistency.pose_nees(self, obj_ids, T_est, T_gt, cov)

    def keypoint_nees(self, dets, T_ref):
        """chi2 of the keypoints of ObjectSLAM detection dicts at the poses T_ref: ``{"chi2", "err", "n_skipped"}`` (consistency.keypoint_nees)."""
        from . import consistency
        return consistency.keypoint_nees(self, dets, T_ref)

    def render_depth(self, obj_ids, T, K, hw):
        """float32 [n,H,W] depth images (mm, 0 where nothing is drawn) of the objects under poses [n,3|4,4] and K [n,3,3] or one [3,3]; ``hw`` = (H, W).
        The rules are those of include/suo_hip.h (suo_render_depth)."""
        n, (H, W) = len(obj_ids), hw
        out = np.zeros((n, int(H), int(W)), np.float32)
        idx = np.array([self._index[int(o)] for o in obj_ids], np.int32)
        Tn = _pack34(T, n) if n else np.zeros((0, 12))
        Kn = np.ascontiguousarray(np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 3, 3), (n, 3, 3))).reshape(n, 9)
        _lib.check(self.lib.suo_render_depth(self._h, n, idx.ctypes.data, Tn.ctypes.data, Kn.ctypes.data, int(W), int(H), out.ctypes.data), "suo_render_depth")
        return out

    def vsd(self, obj_ids, T_est, T_gt, K, depth_images, image_index, delta=15, taus=VSD_TAUS, normalized=True, return_counts=False):
        """VSD errors [n, len(taus)] of n (object, estimated pose, ground-truth pose, camera matrix, test depth image) items: ``depth_images`` a sequence of
        float32 [H,W] in mm, ``image_index[n]`` into it.  Both poses are rendered on the device; a call takes VSD_PAIRS_PER_CALL pairs with the images they
        name.  ``return_counts``: also int64 [n, 2 + len(taus)] union, intersection and cost per tau."""
        n = len(obj_ids)
        taus = np.ascontiguousarray(taus, np.float64)
        errors, counts = np.ones((n, len(taus)), np.float64), np.zeros((n, 2 + len(taus)), np.int64)
        if n:
            idx = np.array([self._index[int(o)] for o in obj_ids], np.int32)
            Te, Tg = _pack34(T_est, n), _pack34(T_gt, n)
            Kn = np.ascontiguousarray(np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 3, 3), (n, 3, 3))).reshape(n, 9)
            diam = np.array([float(self.models_info[int(o)]["diameter"]) for o in obj_ids], np.float64)
            image_index = [int(i) for i in image_index]
            H, W = np.asarray(depth_images[image_index[0]]).shape
        for b in range(0, n, VSD_PAIRS_PER_CALL):
            sl = slice(b, min(n, b + VSD_PAIRS_PER_CALL))
            used = sorted(set(image_index[sl]))
            test = np.ascontiguousarray(np.stack([np.asarray(depth_images[i], np.float32) for i in used]))
            assert test.shape[1:] == (H, W), "the depth images of a call must have one size"
            ii = np.array([used.index(i) for i in image_index[sl]], np.int32)
            m = sl.stop - sl.start
            e, c = np.zeros((m, len(taus)), np.float64), np.zeros((m, 2 + len(taus)), np.int64)
            i_, te, tg, kk, dd = (np.ascontiguousarray(a[sl]) for a in (idx, Te, Tg, Kn, diam))
            _lib.check(self.lib.suo_pose_errors_vsd(self._h, m, i_.ctypes.data, te.ctypes.data, tg.ctypes.data, kk.ctypes.data, int(W), int(H), len(used),
                                                    test.ctypes.data, ii.ctypes.data, float(delta), len(taus), taus.ctypes.data, int(bool(normalized)),
                                                    dd.ctypes.data, e.ctypes.data, c.ctypes.data), "suo_pose_errors_vsd")
            errors[sl], counts[sl] = e, c
        return (errors, counts) if return_counts else errors

    def _gt_args(self, obj_ids, T_gt, K, depth_images, image_index):
        n = len(obj_ids)
        idx = np.array([self._index[int(o)] for o in obj_ids], np.int32)
        Tn = _pack34(T_gt, n)
        Kn = np.ascontiguousarray(np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 3, 3), (n, 3, 3))).reshape(n, 9)
        image_index = [int(i) for i in image_index]
        used = sorted(set(image_index))
        test = np.ascontiguousarray(np.stack([np.asarray(depth_images[i], np.float32) for i in used]))
        assert test.ndim == 3, "the depth images of a call must have one size"
        ii = np.array([used.index(i) for i in image_index], np.int32)
        return n, idx, Tn, Kn, test, ii

    def gt_info(self, obj_ids, T_gt, K, depth_images, image_index, delta=15):
        """What scripts/calc_gt_info.py writes per ground-truth instance (row N7; include/suo_hip.h: suo_gt_info): a list of dictionaries with the toolkit's
        six keys -- px_count_all / valid / visib, visib_fract, bbox_obj, bbox_visib -- as Python int / float.  Poses [n,3|4,4], K [n,3,3] or one [3,3],
        ``depth_images`` a sequence of float32 [H,W] in mm, ``image_index[n]`` into it."""
        if len(obj_ids) == 0:
            return []
        n, idx, Tn, Kn, test, ii = self._gt_args(obj_ids, T_gt, K, depth_images, image_index)
        counts, bo, bv = np.zeros((n, 3), np.int64), np.zeros((n, 4), np.int32), np.zeros((n, 4), np.int32)
        _lib.check(self.lib.suo_gt_info(self._h, n, idx.ctypes.data, Tn.ctypes.data, Kn.ctypes.data, test.shape[2], test.shape[1], len(test), test.ctypes.data,
                                        ii.ctypes.data, float(delta), counts.ctypes.data, bo.ctypes.data, bv.ctypes.data), "suo_gt_info")
        out = []
        for c, o, v in zip(counts.tolist(), bo.tolist(), bv.tolist()):
            out.append({"px_count_all": c[0], "px_count_valid": c[1], "px_count_visib": c[2], "visib_fract": c[2] / float(c[0]) if c[0] > 0 else 0.0,
                        "bbox_obj": o, "bbox_visib": v})
        return out

    def gt_masks(self, obj_ids, T_gt, K, depth_images, image_index, delta=15):
        """``(mask, mask_visib)`` uint8 [n,H,W], 0 / 255, as scripts/calc_gt_masks.py writes them (include/suo_hip.h: suo_gt_masks)."""
        if len(obj_ids) == 0:
            return np.zeros((0, 0, 0), np.uint8), np.zeros((0, 0, 0), np.uint8)
        n, idx, Tn, Kn, test, ii = self._gt_args(obj_ids, T_gt, K, depth_images, image_index)
        mask, mask_visib = np.zeros((n,) + test.shape[1:], np.uint8), np.zeros((n,) + test.shape[1:], np.uint8)
        _lib.check(self.lib.suo_gt_masks(self._h, n, idx.ctypes.data, Tn.ctypes.data, Kn.ctypes.data, test.shape[2], test.shape[1], len(test), test.ctypes.data,
                                         ii.ctypes.data, float(delta), mask.ctypes.data, mask_visib.ctypes.data), "suo_gt_masks")
        return mask, mask_visib


def overlapping_sphere_projections(radius, p1, p2):
    """misc.overlapping_sphere_projections (misc.py:309-331): do the projections of two spheres of one radius about p1 and p2 overlap (approximated)."""
    p1, p2 = np.asarray(p1, np.float64).reshape(3), np.asarray(p2, np.float64).reshape(3)
    if p1[2] == 0 or p2[2] == 0:
        return False
    proj1 = (p1 / p1[2])[:2]
    proj2 = (p2 / p2[2])[:2]
    proj_dist = np.linalg.norm(proj1 - proj2)
    proj_dist_thresh = radius * (1.0 / p1[2] + 1.0 / p2[2])
    return bool(proj_dist < proj_dist_thresh)


def kernel_partition(n, max_points, max_syms):
    """How suo_pose_errors_bop deals a call to workgroups (csrc/eval_bop.hip, restated for the placement tests and the benchmark): ``(points per
    workgroup, points per wave-row, symmetries per workgroup)``.  Point i of a tile sits in thread i % 256 (wave (i % 256) // 64), register i // 256; the
    symmetry chunk brings the grid to 1024 workgroups where it can, within 4 .. 64."""
    tile, block, target = 1024, 256, 1024
    wgs = n * ((max_points + tile - 1) // tile)
    want = max(1, (target + wgs - 1) // wgs)
    chunk = min(max_syms, max(4, min(64, (max_syms + want - 1) // want)))
    return tile, block, chunk


# ---- matching and recall (host) ---------------------------------------------------------------------------
def top_estimates(ests, n_top):
    """``[(est_id, est)]``: the ``n_top`` estimates of one (scene, image, object) with the highest score, ties in the order given
    (eval_calc_errors.py:258-262: a stable sort by descending score of the enumerated list)."""
    return sorted(enumerate(ests), key=lambda x: x[1]["score"], reverse=True)[:n_top]


def valid_gt_mask(im_gt_obj_ids, im_visib_fract, im_targets):
    """visib_gt_min = -1 (eval_calc_scores.py:224-238): per object the ``inst_count`` most visible ground truths of the image are valid.
    ``im_targets``: ``{obj_id: inst_count}``."""
    order = sorted(range(len(im_gt_obj_ids)), key=lambda g: im_visib_fract[g], reverse=True)
    to_add = dict(im_targets)
    valid = [False] * len(im_gt_obj_ids)
    for g in order:
        o = im_gt_obj_ids[g]
        if to_add.get(o, 0) > 0:
            valid[g] = True
            to_add[o] -= 1
    return valid


def match_poses(errs, threshold, gt_valid):
    """Greedy matching of the estimates of one (image, object) to its ground truths (pose_matching.match_poses with one error element and
    max_ests_count <= 0): by descending score, each estimate takes the valid, unmatched ground truth with the smallest error strictly below the threshold.
    ``errs``: ``[{"est_id", "score", "errors": {gt_id: error}}]``.  Returns ``[(est_id, gt_id, error)]``."""
    matches, taken = [], []
    for e in sorted(errs, key=lambda e: e["score"], reverse=True):
        best_gt, best = -1, threshold
        for gt_id, err in e["errors"].items():
            if gt_valid[gt_id] and gt_id not in taken and err < best:
                best_gt, best = gt_id, err
        if best_gt >= 0:
            taken.append(best_gt)
            matches.append((e["est_id"], best_gt, best))
    return matches


def match_poses_image(im_gt_obj_ids, gt_valid, im_errs, threshold):
    """One image of pose_matching.match_poses_scene: ``est_id`` per ground truth (-1: unmatched).  ``im_errs``: ``{obj_id: errs}`` as in match_poses."""
    est = [-1] * len(im_gt_obj_ids)
    for obj_id in set(im_gt_obj_ids):
        for est_id, gt_id, _ in match_poses(im_errs.get(obj_id, []), threshold, gt_valid):
            est[gt_id] = est_id
    return est


class Bop19Meter:
    """Collects pose estimates and turns them into the MSSD and MSPD recalls of eval_bop19.py.

    ``errors``: a BopErrors (or anything with ``.errors(obj_ids, T_est, T_gt, K)``, ``.models_info`` and ``.max_sym_disc_step``);
    ``targets``: the list of the targets file (``{"scene_id", "im_id", "obj_id", "inst_count"}``); ``scene_gt`` / ``scene_gt_info``:
    ``{scene_id: {im_id: [ground truths of scene_gt.json / scene_gt_info.json, unfiltered]}}``; ``im_width``: width of the split's images in pixels."""

    def __init__(self, errors, targets, scene_gt, scene_gt_info, im_width, depth_loader=None, vsd_delta=15):
        """``depth_loader(scene_id, im_id)`` -> float32 [H,W] depth in mm (BopDataset.read_depth): with it ``result()`` also carries VSD (``errors`` then
        needs ``.vsd``, a BopErrors over a mesh database with faces) and the mean of the three terms; without it nothing changes."""
        self.errors = errors
        self.depth_loader, self.vsd_delta = depth_loader, vsd_delta
        self.im_width = float(im_width)
        self.scene_gt, self.scene_gt_info = scene_gt, scene_gt_info
        self.targets = {}                                         # scene -> image -> obj -> inst_count, in the file's order
        for t in targets:
            self.targets.setdefault(t["scene_id"], {}).setdefault(t["im_id"], {})[t["obj_id"]] = t["inst_count"]
        self.ests = {}                                            # (scene, image, obj) -> [{"score", "T", "K"}]
        self.n_estimates = 0                                      # the estimates that were scored (top inst_count of a target), after result()

    @classmethod
    def from_dataset_tree(cls, errors, split_dir, targets_filename, im_width, depth_loader=None, vsd_delta=15):
        """Targets file + the ``scene_gt.json`` / ``scene_gt_info.json`` of every scene it names, read unfiltered."""
        with open(targets_filename, "r") as f:
            targets = json.load(f)
        scene_gt, scene_gt_info = {}, {}
        for s in sorted({t["scene_id"] for t in targets}):
            for name, dst in (("scene_gt.json", scene_gt), ("scene_gt_info.json", scene_gt_info)):
                with open(os.path.join(split_dir, f"{s:06d}", name), "r") as f:
                    dst[s] = {int(k): v for k, v in json.load(f).items()}
        return cls(errors, targets, scene_gt, scene_gt_info, im_width, depth_loader=depth_loader, vsd_delta=vsd_delta)

    def add(self, scene_id, im_id, obj_id, score, T_est, K):
        """One line of the results file: pose [3|4,4] object to camera in mm, the image's camera matrix."""
        T = np.asarray(T_est, np.float64).reshape(-1, 4)[:3, :]
        self.ests.setdefault((int(scene_id), int(im_id), int(obj_id)), []).append({"score": score, "T": T, "K": np.asarray(K, np.float64).reshape(3, 3)})

    def error_table(self):
        """eval_calc_errors.py:196-325 for both error types: ``{scene: {im: {obj: [{"est_id", "score", "errors": {gt_id: (mssd, mspd)}}]}}}``, raw errors
        (mm, px).  MSSD of a pair whose centres lie a diameter or more apart is inf without a device call."""
        table, pairs = {}, []
        self.n_estimates = 0
        for s, ims in self.targets.items():
            for im, objs in ims.items():
                for o, inst_count in objs.items():
                    kept = top_estimates(self.ests.get((s, im, o), []), inst_count)
                    self.n_estimates += len(kept)
                    diameter = self.errors.models_info[o]["diameter"]
                    for est_id, est in kept:
                        row = {"est_id": est_id, "score": est["score"], "errors": {}}
                        table.setdefault(s, {}).setdefault(im, {}).setdefault(o, []).append(row)
                        for gt_id, gt in enumerate(self.scene_gt[s][im]):
                            if gt["obj_id"] != o:
                                continue
                            Tg = np.hstack((np.reshape(gt["cam_R_m2c"], (3, 3)), np.reshape(gt["cam_t_m2c"], (3, 1)))).astype(np.float64)
                            overlap = np.linalg.norm(est["T"][:, 3] - Tg[:, 3]) < diameter
                            pairs.append((row, gt_id, o, est["T"], Tg, est["K"], bool(overlap)))
        if pairs:
            mssd, mspd = self.errors.errors([p[2] for p in pairs], np.stack([p[3] for p in pairs]), np.stack([p[4] for p in pairs]),
                                            np.stack([p[5] for p in pairs]))
            for (row, gt_id, _, _, _, _, overlap), e3, e2 in zip(pairs, mssd.tolist(), mspd.tolist()):
                row["errors"][gt_id] = (e3 if overlap else float("inf"), e2)
        return table

    def vsd_table(self, taus=VSD_TAUS):
        """eval_calc_errors.py:196-325 for the error type ``vsd``: the table of error_table with ``errors: {gt_id: [e per tau]}`` (already normalised by the
        diameter inside the error).  A pair whose sphere projections do not overlap gets 1.0 for every tau without a device call (:295-312)."""
        table, pairs, images, slot = {}, [], [], {}
        for s, ims in self.targets.items():
            for im, objs in ims.items():
                for o, inst_count in objs.items():
                    radius = 0.5 * self.errors.models_info[o]["diameter"]
                    for est_id, est in top_estimates(self.ests.get((s, im, o), []), inst_count):
                        row = {"est_id": est_id, "score": est["score"], "errors": {}}
                        table.setdefault(s, {}).setdefault(im, {}).setdefault(o, []).append(row)
                        for gt_id, gt in enumerate(self.scene_gt[s][im]):
                            if gt["obj_id"] != o:
                                continue
                            Tg = np.hstack((np.reshape(gt["cam_R_m2c"], (3, 3)), np.reshape(gt["cam_t_m2c"], (3, 1)))).astype(np.float64)
                            if not overlapping_sphere_projections(radius, est["T"][:, 3], Tg[:, 3]):
                                row["errors"][gt_id] = [1.0] * len(taus)
                                continue
                            if (s, im) not in slot:
                                slot[(s, im)] = len(images)
                                images.append((s, im))
                            pairs.append((row, gt_id, o, est["T"], Tg, est["K"], slot[(s, im)]))
        # device calls over runs of pairs that share few images: the pairs come image by image, so a run of VSD_PAIRS_PER_CALL names a handful
        for b in range(0, len(pairs), VSD_PAIRS_PER_CALL):
            run = pairs[b:b + VSD_PAIRS_PER_CALL]
            used = sorted({p[6] for p in run})
            depth = [np.asarray(self.depth_loader(*images[i]), np.float32) for i in used]
            errs = self.errors.vsd([p[2] for p in run], np.stack([p[3] for p in run]), np.stack([p[4] for p in run]), np.stack([p[5] for p in run]),
                                   depth, [used.index(p[6]) for p in run], delta=self.vsd_delta, taus=taus, normalized=True)
            for (row, gt_id, *_), e in zip(run, np.asarray(errs).tolist()):
                row["errors"][gt_id] = e
        return table

    def normalised(self, table):
        """eval_calc_scores.py:246-258: MSSD divided by the object's diameter, MSPD multiplied by 640 / image width."""
        factor = 640.0 / self.im_width
        out = {}
        for s, ims in table.items():
            for im, objs in ims.items():
                for o, rows in objs.items():
                    diameter = float(self.errors.models_info[o]["diameter"])
                    out.setdefault(s, {}).setdefault(im, {})[o] = [
                        {"est_id": r["est_id"], "score": r["score"], "errors": {g: (e[0] / diameter, factor * e[1]) for g, e in r["errors"].items()}} for r in rows]
        return out

    def recalls(self, table, which, thresholds):
        """score.calc_localization_scores' ``recall`` for every threshold: valid ground truths with a matched estimate / valid ground truths,
        over the images of the targets file.  ``table``: normalised errors; ``which``: 0 = MSSD, 1 = MSPD."""
        out, n_targets = [], 0
        for th in thresholds:
            tp = tars = 0
            for s, ims in self.targets.items():
                for im, objs in ims.items():
                    gt_ids = [g["obj_id"] for g in self.scene_gt[s][im]]
                    valid = valid_gt_mask(gt_ids, [i["visib_fract"] for i in self.scene_gt_info[s][im]], objs)
                    errs = {o: [{"est_id": r["est_id"], "score": r["score"], "errors": {g: e[which] for g, e in r["errors"].items()}} for r in rows]
                            for o, rows in table.get(s, {}).get(im, {}).items()}
                    est = match_poses_image(gt_ids, valid, errs, float(th))
                    tars += sum(valid)
                    tp += sum(1 for g, v in enumerate(valid) if v and est[g] != -1)
            n_targets = tars
            out.append(tp / float(tars) if tars else 0.0)
        return out, n_targets

    def result(self):
        """``{"mssd": {"recalls": [10], "ar"}, "mspd": {...}, "n_targets", "n_estimates", "max_sym_disc_step"}``; ``ar`` is the mean of the ten recalls.
        With a depth loader also ``"vsd": {"recalls": [[10] per tau], "ar"}`` (100 recalls: the errors of each tau matched at each of the ten thresholds;
        ``ar`` their mean) and ``"ar"``, the mean of the three terms."""
        table = self.normalised(self.error_table())
        out = {}
        for name, which, ths in (("mssd", 0, MSSD_THRESHOLDS), ("mspd", 1, MSPD_THRESHOLDS)):
            rec, n_targets = self.recalls(table, which, ths)
            out[name] = {"recalls": rec, "ar": float(np.mean(rec))}
            out["n_targets"] = int(n_targets)
        out["n_estimates"] = int(self.n_estimates)
        out["max_sym_disc_step"] = self.errors.max_sym_disc_step
        if self.depth_loader is not None:
            vtable = self.vsd_table(VSD_TAUS)                      # VSD errors are not normalised again (eval_calc_scores.py:246-258 touches mssd / mspd only)
            rec = [self.recalls(vtable, t, VSD_THRESHOLDS)[0] for t in range(len(VSD_TAUS))]
            out["vsd"] = {"recalls": rec, "ar": float(np.mean(rec))}
            out["ar"] = float(np.mean([out["vsd"]["ar"], out["mssd"]["ar"], out["mspd"]["ar"]]))      # eval_bop19.py:240-241
        return out
