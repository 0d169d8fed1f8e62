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

Beside it since row N4, with nothing above changed: the protocol of scripts/eval_siso.py and the error functions eval_calc_errors.py offers beyond the three:

    BopErrors.point_errors(obj_ids, T_est, T_gt, K, which)      pose_error.add / adi / proj                 -> HIP, csrc/eval_points.hip (suo_pose_errors_points)
    BopErrors.mask_errors(obj_ids, T_est, T_gt, K, hw)          pose_error.cus / cou_bb_proj                -> HIP, csrc/eval_masks.hip (suo_pose_errors_masks)
    rotation_error / translation_error                          pose_error.re / te (host numpy)
    LocalizationMeter(errors, targets, scene_gt, scene_gt_info, error_type, n_top, visib_gt_min, correct_th, ...)
        .add(...) / .result() / .errors_json(scene_id) / .matches()
                                                                eval_calc_errors.py:192-388 + eval_calc_scores.py:184-269 for one error type, any n_top, both
                                                                rules of visib_gt_min; SISO_PARAMS are eval_siso.py's (Evaluator(siso=True), tools/eval_siso.py)

Written once, for everything above: stage_pairs / stage_images (what every BopErrors method and consistency.py hand to C: model indices, [n,12] poses, [n,9]
camera matrices; the test images of a call stacked and re-indexed), _Meter (the base of both meters: targets index, add, from_dataset_tree and _walk -- scene ->
image -> object -> kept estimates -> ground truths, in the scripts' order), projections_overlap / centres_within (the two shortcut gates), vsd_runs (runs of
VSD_PAIRS_PER_CALL pairs, each with exactly the images it names) and match_poses_elements (the greedy rule; match_poses is its one-element form).
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
def _numpy(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else x


def pack_poses(T, n):
    """float64 [n,12], C-contiguous: the rows [R|t] of n poses [n,3|4,4], torch or numpy."""
    return np.ascontiguousarray(np.asarray(_numpy(T), np.float64).reshape(n, -1, 4)[:, :3, :]).reshape(n, 12) if n else np.zeros((0, 12), np.float64)


def stage_pairs(index, obj_ids, K, *poses):
    """What every C entry over the mesh database takes, staged once: ``(n, idx, K, *poses)`` with ``idx`` int32 [n] the model indices of ``obj_ids`` under
    ``index`` ({obj_id: model index}; an unknown object is a KeyError), ``K`` float64 [n,9] from one [3,3] or [n,3,3] (None stays None) and every pose
    [n,3|4,4] as pack_poses gives it.  All C-contiguous; no device."""
    n = len(obj_ids)
    idx = np.array([index[int(o)] for o in obj_ids], np.int32)
    if K is not None:
        K = np.ascontiguousarray(np.broadcast_to(np.asarray(_numpy(K), np.float64).reshape(-1, 3, 3), (n, 3, 3))).reshape(n, 9)
    return (n, idx, K) + tuple(pack_poses(T, n) for T in poses)


def stage_images(depth_images, image_index):
    """The test images a call names, stacked and re-indexed: ``(float32 [k,H,W] of the images ``image_index`` names, in ascending order of their index;
    int32 [n] indices into that stack)``."""
    image_index = [int(i) for i in image_index]
    used = sorted(set(image_index))
    test = np.ascontiguousarray(np.stack([np.asarray(depth_images[i], np.float32) for i in used]))
    assert test.ndim == 3, "the depth images of a call must have one size"
    return test, np.array([used.index(i) for i in image_index], np.int32)


POINT_ERROR_BITS = {"add": 1, "adi": 2, "proj": 4}      # SUO_POINTS_ADD / _ADI / _PROJ of include/suo_hip.h


def cus_from_counts(union, inter):
    """pose_error.cus from the two pixel counts (pose_error.py:281-285): 1 - inter / float(union), 1.0 for an empty union."""
    return 1.0 - int(inter) / float(union) if union > 0 else 1.0


def iou_boxes(bb_a, bb_b):
    """misc.iou of two boxes (x, y, w, h) as misc.calc_2d_bbox forms them (misc.py:236-263)."""
    tl_a, br_a = (bb_a[0], bb_a[1]), (bb_a[0] + bb_a[2], bb_a[1] + bb_a[3])
    tl_b, br_b = (bb_b[0], bb_b[1]), (bb_b[0] + bb_b[2], bb_b[1] + bb_b[3])
    w_inter = min(br_a[0], br_b[0]) - max(tl_a[0], tl_b[0])
    h_inter = min(br_a[1], br_b[1]) - max(tl_a[1], tl_b[1])
    if w_inter > 0 and h_inter > 0:
        area_inter = w_inter * h_inter
        return area_inter / float(bb_a[2] * bb_a[3] + bb_b[2] * bb_b[3] - area_inter)
    return 0.0


def cou_bb_from_boxes(box_est, box_gt):
    """pose_error.cou_bb_proj from the two masks' boxes (pose_error.py:323-329); 1.0 when a mask is empty (box [-1,-1,-1,-1]; the toolkit raises there)."""
    if box_est[2] < 0 or box_gt[2] < 0:
        return 1.0
    return 1.0 - iou_boxes([int(v) for v in box_est], [int(v) for v in box_gt])


def rotation_error(R_est, R_gt):
    """pose_error.re (pose_error.py:187-202): the angle of R_est R_gt^-1 in degrees."""
    R_est, R_gt = np.asarray(R_est, np.float64).reshape(3, 3), np.asarray(R_gt, np.float64).reshape(3, 3)
    error_cos = float(0.5 * (np.trace(R_est.dot(np.linalg.inv(R_gt))) - 1.0))
    error_cos = min(1.0, max(-1.0, error_cos))
    return 180.0 * math.acos(error_cos) / np.pi


def translation_error(t_est, t_gt):
    """pose_error.te (pose_error.py:205-214): |t_gt - t_est| in the poses' unit."""
    return np.linalg.norm(np.asarray(t_gt, np.float64).reshape(3, 1) - np.asarray(t_est, np.float64).reshape(3, 1))


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
        n, idx, Kn, Te, Tg = stage_pairs(self._index, obj_ids, K, T_est, T_gt)
        mssd, mspd = np.zeros(n, np.float64), np.zeros(n, np.float64)
        if n == 0:
            return mssd, mspd
        _lib.check(self.lib.suo_pose_errors_bop(self._h, n, idx.ctypes.data, Te.ctypes.data, Tg.ctypes.data, Kn.ctypes.data, mssd.ctypes.data, mspd.ctypes.data),
                   "suo_pose_errors_bop")
        return mssd, mspd

    def point_errors(self, obj_ids, T_est, T_gt, K=None, which=("add", "adi", "proj")):
        """The toolkit's pose_error.add / adi / proj (row N4; include/suo_hip.h: suo_pose_errors_points) of n (object, estimated pose, ground-truth pose,
        camera matrix) items: ``{name: float64 [n]}`` for the names in ``which``, mm for add / adi and px for proj.  ``adi`` is the exact mean nearest-neighbour
        distance from the ground-truth points to the estimated-pose points (the toolkit's direction); only it costs P^2.  ``K`` is needed for proj only."""
        which = tuple(which)
        unknown = set(which) - set(POINT_ERROR_BITS)
        if unknown:
            raise ValueError(f"point_errors: unknown error {sorted(unknown)}; known: {sorted(POINT_ERROR_BITS)}")
        if "proj" in which and K is None:
            raise ValueError("point_errors: proj needs the camera matrix K")
        n, idx, Kn, Te, Tg = stage_pairs(self._index, obj_ids, K, T_est, T_gt)
        out = {w: np.zeros(n, np.float64) for w in POINT_ERROR_BITS}
        if n and which:
            mask = sum(POINT_ERROR_BITS[w] for w in set(which))
            _lib.check(self.lib.suo_pose_errors_points(self._h, n, idx.ctypes.data, Te.ctypes.data, Tg.ctypes.data, None if Kn is None else Kn.ctypes.data, mask,
                                                       out["add"].ctypes.data, out["adi"].ctypes.data, out["proj"].ctypes.data), "suo_pose_errors_points")
        return {w: out[w] for w in which}

    def mask_errors(self, obj_ids, T_est, T_gt, K, hw):
        """The toolkit's pose_error.cus and cou_bb_proj (row N4; include/suo_hip.h: suo_pose_errors_masks) of n items on images of ``hw`` = (H, W):
        ``{"cus", "cou_bb_proj": float64 [n], "union", "inter": int64 [n], "box_est", "box_gt": int32 [n,4]}``.  Both poses are rendered on the device and
        reduced there to integers; the quotients are formed here in fp64.  An empty mask gives cou_bb_proj 1.0 (the toolkit raises)."""
        (n, idx, Kn, Te, Tg), (H, W) = stage_pairs(self._index, obj_ids, K, T_est, T_gt), hw
        counts, be, bg = np.zeros((n, 2), np.int64), np.full((n, 4), -1, np.int32), np.full((n, 4), -1, np.int32)
        if n:
            _lib.check(self.lib.suo_pose_errors_masks(self._h, n, idx.ctypes.data, Te.ctypes.data, Tg.ctypes.data, Kn.ctypes.data, int(W), int(H),
                                                      counts.ctypes.data, be.ctypes.data, bg.ctypes.data), "suo_pose_errors_masks")
        return {"cus": np.array([cus_from_counts(u, i) for u, i in counts.tolist()], np.float64),
                "cou_bb_proj": np.array([cou_bb_from_boxes(a, b) for a, b in zip(be.tolist(), bg.tolist())], np.float64),
                "union": counts[:, 0].copy(), "inter": counts[:, 1].copy(), "box_est": be, "box_gt": bg}

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
        (n, idx, Kn, Tn), (H, W) = stage_pairs(self._index, obj_ids, K, T), hw
        out = np.zeros((n, int(H), int(W)), np.float32)
        _lib.check(self.lib.suo_render_depth(self._h, n, idx.ctypes.data, Tn.ctypes.data, Kn.ctypes.data, int(W), int(H), out.ctypes.data), "suo_render_depth")
        return out

    def vsd(self, obj_ids, T_est, T_gt, K, depth_images, image_index, delta=15, taus=VSD_TAUS, normalized=True, return_counts=False):
        """VSD errors [n, len(taus)] of n (object, estimated pose, ground-truth pose, camera matrix, test depth image) items: ``depth_images`` a sequence of
        float32 [H,W] in mm, ``image_index[n]`` into it.  Both poses are rendered on the device; a call takes VSD_PAIRS_PER_CALL pairs with the images they
        name.  ``return_counts``: also int64 [n, 2 + len(taus)] union, intersection and cost per tau."""
        n, idx, Kn, Te, Tg = stage_pairs(self._index, obj_ids, K, T_est, T_gt)
        taus = np.ascontiguousarray(taus, np.float64)
        errors, counts = np.ones((n, len(taus)), np.float64), np.zeros((n, 2 + len(taus)), np.int64)
        if n:
            diam = np.array([float(self.models_info[int(o)]["diameter"]) for o in obj_ids], np.float64)
            image_index = list(image_index)
            H, W = np.asarray(depth_images[int(image_index[0])]).shape
        for b in range(0, n, VSD_PAIRS_PER_CALL):
            sl = slice(b, min(n, b + VSD_PAIRS_PER_CALL))
            test, ii = stage_images(depth_images, image_index[sl])
            assert test.shape[1:] == (H, W), "the depth images of a call must have one size"
            m = sl.stop - sl.start
            e, c = np.zeros((m, len(taus)), np.float64), np.zeros((m, 2 + len(taus)), np.int64)
            i_, te, tg, kk, dd = (np.ascontiguousarray(a[sl]) for a in (idx, Te, Tg, Kn, diam))
            _lib.check(self.lib.suo_pose_errors_vsd(self._h, m, i_.ctypes.data, te.ctypes.data, tg.ctypes.data, kk.ctypes.data, int(W), int(H), len(test),
                                                    test.ctypes.data, ii.ctypes.data, float(delta), len(taus), taus.ctypes.data, int(bool(normalized)),
                                                    dd.ctypes.data, e.ctypes.data, c.ctypes.data), "suo_pose_errors_vsd")
            errors[sl], counts[sl] = e, c
        return (errors, counts) if return_counts else errors

    def _gt_args(self, obj_ids, T_gt, K, depth_images, image_index):
        n, idx, Kn, Tn = stage_pairs(self._index, obj_ids, K, T_gt)
        return (n, idx, Tn, Kn) + stage_images(depth_images, image_index)

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
    ``errs``: ``[{"est_id", "score", "errors": {gt_id: error}}]``.  Returns ``[(est_id, gt_id, error)]``.  The rule itself is match_poses_elements'."""
    one = [{"est_id": e["est_id"], "score": e["score"], "errors": {g: (err,) for g, err in e["errors"].items()}} for e in errs]
    return [(m["est_id"], m["gt_id"], m["error"][0]) for m in match_poses_elements(one, (threshold,), 0, gt_valid)]


def match_poses_image(im_gt_obj_ids, gt_valid, im_errs, threshold):
    """One image of pose_matching.match_poses_scene: ``est_id`` per ground truth (-1: unmatched).  ``im_errs``: ``{obj_id: errs}`` as in match_poses."""
    est = [-1] * len(im_gt_obj_ids)
    for obj_id in set(im_gt_obj_ids):
        for est_id, gt_id, _ in match_poses(im_errs.get(obj_id, []), threshold, gt_valid):
            est[gt_id] = est_id
    return est


# ---- what the two meters share: collection, the pair walk, the two shortcut gates, the VSD runs ----------
def projections_overlap(diameter, T_est, T_gt):
    """The gate of vsd and cus (eval_calc_errors.py:295-312): a pair whose sphere projections do not overlap is 1.0 without a device call."""
    return overlapping_sphere_projections(0.5 * diameter, T_est[:, 3], T_gt[:, 3])


def centres_within(diameter, T_est, T_gt):
    """The gate of mssd, ad, add and adi (eval_calc_errors.py:314-323): a pair whose centres lie a diameter or more apart is inf without a device call."""
    return bool(np.linalg.norm(T_est[:, 3] - T_gt[:, 3]) < diameter)


def _stacked(pairs):
    """``(obj_ids, T_est [n,3,4], T_gt [n,3,4], K [n,3,3])`` of pairs ``[(scene, im, obj, T_est, T_gt, K)]``."""
    return [p[2] for p in pairs], np.stack([p[3] for p in pairs]), np.stack([p[4] for p in pairs]), np.stack([p[5] for p in pairs])


def vsd_runs(errors, depth_loader, pairs, **kw):
    """``errors.vsd`` over pairs ``[(scene, im, obj, T_est, T_gt, K)]`` in runs of VSD_PAIRS_PER_CALL (read at call time): the pairs come image by image, so
    a run names a handful of images.  Exactly those are loaded, in the order they were first seen among all pairs, and the run's ``image_index`` counts
    into them.  ``kw``: delta, taus, normalized.  Returns the error lists, one per pair."""
    slot, out, per_call = {}, [], VSD_PAIRS_PER_CALL
    slots = [slot.setdefault((p[0], p[1]), len(slot)) for p in pairs]
    images = list(slot)
    for b in range(0, len(pairs), per_call):
        used = sorted(set(slots[b:b + per_call]))
        depth = [np.asarray(depth_loader(*images[i]), np.float32) for i in used]
        out += np.asarray(errors.vsd(*_stacked(pairs[b:b + per_call]), depth, [used.index(i) for i in slots[b:b + per_call]], **kw)).tolist()
    return out


class _Meter:
    """Collection and the pair walk of Bop19Meter and LocalizationMeter.  ``targets``: the list of the targets file (``{"scene_id", "im_id", "obj_id",
    "inst_count"}``); ``scene_gt`` / ``scene_gt_info``: ``{scene_id: {im_id: [ground truths of scene_gt.json / scene_gt_info.json, unfiltered]}}``."""

    def __init__(self, errors, targets, scene_gt, scene_gt_info):
        self.errors, self.scene_gt, self.scene_gt_info = errors, scene_gt, scene_gt_info
        self.targets = {}                                         # scene -> image -> obj -> inst_count, in the file's order
        for t in targets:
            self.targets.setdefault(t["scene_id"], {}).setdefault(t["im_id"], {})[t["obj_id"]] = t["inst_count"]
        self.ests = {}                                            # (scene, image, obj) -> [{"score", "T", "K"}]
        self.n_estimates = 0                                      # the estimates that were scored (the top n of a target), after a walk

    @classmethod
    def from_dataset_tree(cls, errors, split_dir, targets_filename, *args, **kw):
        """Targets file + the ``scene_gt.json`` / ``scene_gt_info.json`` of every scene it names, read unfiltered; ``args``, ``kw`` as for the constructor
        behind ``scene_gt_info``."""
        with open(targets_filename, "r") as f:
            targets = json.load(f)
        scene_gt, scene_gt_info = {}, {}
        for s in sorted({t["scene_id"] for t in targets}):
            for name, dst in (("scene_gt.json", scene_gt), ("scene_gt_info.json", scene_gt_info)):
                with open(os.path.join(split_dir, f"{s:06d}", name), "r") as f:
                    dst[s] = {int(k): v for k, v in json.load(f).items()}
        return cls(errors, targets, scene_gt, scene_gt_info, *args, **kw)

    def add(self, scene_id, im_id, obj_id, score, T_est, K):
        """One line of the results file: pose [3|4,4] object to camera in mm, the image's camera matrix."""
        T = np.asarray(T_est, np.float64).reshape(-1, 4)[:3, :]
        self.ests.setdefault((int(scene_id), int(im_id), int(obj_id)), []).append({"score": score, "T": T, "K": np.asarray(K, np.float64).reshape(3, 3)})

    def _walk(self, n_top):
        """Scene -> image -> object of the targets, in the file's order, -> the kept estimates by descending score (eval_calc_errors.py:232-262: ``n_top``
        k, 0 = all, -1 = the target's inst_count): yields ``(scene, im, obj, est_id, est, [(gt_id, T_gt [3,4])])`` with the ground truths of that object in
        the image, in their order.  Counts the kept estimates into ``n_estimates``."""
        self.n_estimates = 0
        for s, ims in self.targets.items():
            for im, objs in ims.items():
                for o, inst_count in objs.items():
                    kept = top_estimates(self.ests.get((s, im, o), []), None if n_top == 0 else inst_count if n_top == -1 else n_top)
                    self.n_estimates += len(kept)
                    gts = [(g, np.hstack((np.reshape(gt["cam_R_m2c"], (3, 3)), np.reshape(gt["cam_t_m2c"], (3, 1)))).astype(np.float64))
                           for g, gt in enumerate(self.scene_gt[s][im]) if kept and gt["obj_id"] == o]
                    for est_id, est in kept:
                        yield s, im, o, est_id, est, gts


class Bop19Meter(_Meter):
    """Collects pose estimates and turns them into the MSSD and MSPD recalls of eval_bop19.py.  Its own: ONE ``errors.errors`` call that serves both MSSD
    and MSPD, and the ten thresholds.  ``errors``: a BopErrors (or anything with ``.errors(obj_ids, T_est, T_gt, K)``, ``.models_info`` and
    ``.max_sym_disc_step``); ``targets``, ``scene_gt``, ``scene_gt_info``: as for _Meter; ``im_width``: width of the split's images in pixels."""

    def __init__(self, errors, targets, scene_gt, scene_gt_info, im_width, depth_loader=None, vsd_delta=15):
        """``depth_loader(scene_id, im_id)`` -> float32 [H,W] depth in mm (BopDataset.read_depth): with it ``result()`` also carries VSD (``errors`` then
        needs ``.vsd``, a BopErrors over a mesh database with faces) and the mean of the three terms; without it nothing changes."""
        super().__init__(errors, targets, scene_gt, scene_gt_info)
        self.depth_loader, self.vsd_delta = depth_loader, vsd_delta
        self.im_width = float(im_width)

    def _table(self, gated):
        """The walk as the nested table of both error types: ``(table, pairs, where)`` with ``where[k] = (row, gt_id)`` of ``pairs[k]``.  ``gated(est, Tg,
        diameter)``: None to send the pair to the device, else the value a shortcut gives it at once."""
        table, pairs, where = {}, [], []
        for s, im, o, est_id, est, gts in self._walk(-1):
            row = {"est_id": est_id, "score": est["score"], "errors": {}}
            table.setdefault(s, {}).setdefault(im, {}).setdefault(o, []).append(row)
            for gt_id, Tg in gts:
                value = gated(est, Tg, self.errors.models_info[o]["diameter"])
                if value is None:
                    pairs.append((s, im, o, est["T"], Tg, est["K"]))
                    where.append((row, gt_id))
                else:
                    row["errors"][gt_id] = value
        return table, pairs, where

    def error_table(self):
        """eval_calc_errors.py:196-325 for both error types: ``{scene: {im: {obj: [{"est_id", "score", "errors": {gt_id: (mssd, mspd)}}]}}}``, raw errors
        (mm, px).  MSSD of a pair whose centres lie a diameter or more apart is inf without a device call (MSPD has no shortcut: every pair is sent)."""
        table, pairs, where = self._table(lambda est, Tg, diameter: None)
        if pairs:
            mssd, mspd = self.errors.errors(*_stacked(pairs))
            for (row, gt_id), p, e3, e2 in zip(where, pairs, mssd.tolist(), mspd.tolist()):
                row["errors"][gt_id] = (e3 if centres_within(self.errors.models_info[p[2]]["diameter"], p[3], p[4]) else float("inf"), e2)
        return table

    def vsd_table(self, taus=VSD_TAUS):
        """eval_calc_errors.py:196-325 for the error type ``vsd``: the table of error_table with ``errors: {gt_id: [e per tau]}`` (already normalised by the
        diameter inside the error).  A pair whose sphere projections do not overlap gets 1.0 for every tau without a device call (:295-312)."""
        table, pairs, where = self._table(lambda est, Tg, diameter: None if projections_overlap(diameter, est["T"], Tg) else [1.0] * len(taus))
        for (row, gt_id), e in zip(where, vsd_runs(self.errors, self.depth_loader, pairs, delta=self.vsd_delta, taus=taus, normalized=True)):
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


# ---- the general localisation meter: eval_calc_errors.py + eval_calc_scores.py for one error type (row N4) ----
ERROR_TYPES = ("vsd", "mssd", "mspd", "ad", "add", "adi", "cus", "proj", "re", "te", "rete")
CORRECT_TH = {"vsd": [0.3], "mssd": [0.2], "mspd": [10.0], "cus": [0.5], "rete": [5.0, 5.0], "re": [5.0], "te": [5.0], "proj": [5.0], "ad": [0.1], "add": [0.1],
              "adi": [0.1]}                                  # eval_calc_scores.py:39-51
NORMALIZED_BY_DIAMETER = ("ad", "add", "adi", "mssd")       # eval_calc_scores.py:54
NORMALIZED_BY_IM_WIDTH = ("mspd",)                          # eval_calc_scores.py:57
SISO_PARAMS = dict(error_type="vsd", n_top=1, visib_gt_min=0.1, correct_th=[0.3], vsd_delta=15, vsd_taus=[20.0], vsd_normalized_by_diameter=False)   # scripts/eval_siso.py:26-46


def error_signature(error_type, n_top, vsd_delta=None, vsd_tau=None):
    """misc.get_error_signature (misc.py:334-350): the folder name of one error calculation."""
    sign = "error=" + error_type + "_ntop=" + str(n_top)
    if error_type == "vsd":
        tau = "inf" if vsd_tau == float("inf") else "{:.3f}".format(vsd_tau)
        sign += "_delta={:.3f}_tau={}".format(vsd_delta, tau)
    return sign


def score_signature(correct_th, visib_gt_min):
    """misc.get_score_signature (misc.py:353-361)."""
    return "th=" + "-".join(["{:.3f}".format(t) for t in correct_th]) + "_min-visib={:.3f}".format(visib_gt_min)


def match_poses_elements(errs, error_ths, max_ests_count=0, gt_valid=None):
    """pose_matching.match_poses (pose_matching.py:9-90) for an error of any number of elements: by descending score, each estimate takes the valid,
    unmatched ground truth that beats the best so far in ALL elements, the thresholds being the first best.  ``errs``: ``[{"est_id", "score", "errors":
    {gt_id: [e, ...]}}]``.  Returns ``[{"est_id", "gt_id", "score", "error", "error_norm"}]``.  The one place the greedy rule is written."""
    errs_sorted = sorted(errs, key=lambda e: e["score"], reverse=True)
    if max_ests_count > 0:
        errs_sorted = errs_sorted[:max_ests_count]
    n_el = len(error_ths)
    matches, taken = [], []
    for e in errs_sorted:
        best_gt, best = -1, list(error_ths)
        for gt_id, error in e["errors"].items():
            if (not gt_valid or gt_valid[gt_id]) and gt_id not in taken and all(error[i] < best[i] for i in range(n_el)):
                best_gt, best = gt_id, error
        if best_gt >= 0:
            taken.append(best_gt)
            matches.append({"est_id": e["est_id"], "gt_id": best_gt, "score": e["score"], "error": best,
                            "error_norm": [best[i] / float(error_ths[i]) for i in range(n_el)]})
    return matches


def localization_scores(scene_ids, obj_ids, matches, n_top):
    """score.calc_localization_scores (score.py:62-157) without the printing: the dictionary eval_calc_scores.py saves as scores_*.json."""
    insts = {}
    for m in matches:
        if m["valid"]:
            key = (m["obj_id"], m["scene_id"], m["im_id"])
            insts[key] = insts.get(key, 0) + 1
    tars, obj_tars, scene_tars = 0, {i: 0 for i in obj_ids}, {i: 0 for i in scene_ids}
    for (o, s, _), c in insts.items():
        count = min(n_top, c) if n_top > 0 else c              # score.py:93-96: SiSo counts one target however many instances an image shows
        tars += count
        obj_tars[o] += count
        scene_tars[s] += count
    tps, obj_tps, scene_tps = 0, {i: 0 for i in obj_ids}, {i: 0 for i in scene_ids}
    for m in matches:
        if m["valid"] and m["est_id"] != -1:
            tps += 1
            obj_tps[m["obj_id"]] += 1
            scene_tps[m["scene_id"]] += 1
    recall = lambda tp, n: tp / float(n) if n else 0.0
    obj_recalls = {i: recall(obj_tps[i], obj_tars[i]) for i in obj_ids}
    scene_recalls = {i: float(recall(scene_tps[i], scene_tars[i])) for i in scene_ids}
    return {"recall": float(recall(tps, tars)), "obj_recalls": obj_recalls, "mean_obj_recall": float(np.mean(list(obj_recalls.values()))),
            "scene_recalls": scene_recalls, "mean_scene_recall": float(np.mean(list(scene_recalls.values()))),
            "gt_count": len(matches), "targets_count": int(tars), "tp_count": int(tps)}


class LocalizationMeter(_Meter):
    """eval_calc_errors.py:192-388 and eval_calc_scores.py:184-269 for ONE error type, in process: collects pose estimates and returns the dictionary of
    score.calc_localization_scores.  It shares with Bop19Meter the collection of estimates, the reading of a dataset tree, the pair walk with its top-n
    cut, the two shortcut gates, the VSD runs and the greedy matching rule; its own are the choice of one error type and the scripts' records and scores.

    ``errors``: a BopErrors, or anything with ``.models_info`` and the calls the error type needs -- ``.vsd`` (vsd), ``.errors`` (mssd, mspd),
    ``.point_errors`` (ad, add, adi, proj), ``.mask_errors`` (cus); re / te / rete are formed here.  ``targets``, ``scene_gt``, ``scene_gt_info``: as for
    Bop19Meter.  Parameters, with the scripts' names:
        error_type      one of ERROR_TYPES;
        n_top           estimates scored per (image, object), by descending score: k, 0 = all, -1 = the target's inst_count;
        visib_gt_min    >= 0: a ground truth is valid when its object is a target of the image and its visib_fract >= this (eval_calc_scores.py:217-223);
                        -1: per object the inst_count most visible ones (:224-238);
        correct_th      one threshold per error element (rete has two: a match needs ALL elements below); default CORRECT_TH[error_type];
        vsd_delta, vsd_taus, vsd_normalized_by_diameter      as for eval_calc_errors.py; results are per tau (``tau_index``);
        symmetric_obj_ids     the objects for which ``ad`` is adi (add for the others);
        im_width        for the normalisation of mspd;  im_hw = (H, W) for the renders of cus;  depth_loader(scene_id, im_id) for vsd;
        scene_ids, obj_ids    the scenes of the split and the objects of the dataset the scores are reported over (default: those of the targets / of
                        ``errors.models_info``).
    The script's two shortcuts are applied: vsd / cus of a pair whose sphere projections do not overlap is 1.0, ad / add / adi / mssd of a pair whose
    centres lie a diameter or more apart is inf, both without a device call."""

    def __init__(self, errors, targets, scene_gt, scene_gt_info, error_type="vsd", n_top=1, visib_gt_min=-1, correct_th=None, vsd_delta=15,
                 vsd_taus=(20.0,), vsd_normalized_by_diameter=False, symmetric_obj_ids=(), im_width=640, im_hw=None, depth_loader=None, scene_ids=None,
                 obj_ids=None):
        if error_type not in ERROR_TYPES:
            raise ValueError(f"LocalizationMeter: unknown error type {error_type!r}; known: {ERROR_TYPES}")
        super().__init__(errors, targets, scene_gt, scene_gt_info)
        self.error_type, self.n_top, self.visib_gt_min = error_type, int(n_top), float(visib_gt_min)
        self.correct_th = [float(t) for t in (CORRECT_TH[error_type] if correct_th is None else correct_th)]
        n_el = 2 if error_type == "rete" else 1
        if len(self.correct_th) != n_el:
            raise ValueError(f"LocalizationMeter: {error_type} has {n_el} error element(s), correct_th has {len(self.correct_th)}")
        self.vsd_delta, self.vsd_taus, self.vsd_normalized_by_diameter = vsd_delta, [float(t) for t in vsd_taus], bool(vsd_normalized_by_diameter)
        self.symmetric_obj_ids = {int(o) for o in symmetric_obj_ids}
        self.im_width, self.im_hw, self.depth_loader = float(im_width), im_hw, depth_loader
        if error_type == "vsd" and depth_loader is None:
            raise ValueError("LocalizationMeter: vsd needs a depth_loader(scene_id, im_id)")
        if error_type == "cus" and im_hw is None:
            raise ValueError("LocalizationMeter: cus needs im_hw = (H, W)")
        self.scene_ids = sorted(self.targets) if scene_ids is None else [int(s) for s in scene_ids]
        self.obj_ids = sorted(int(o) for o in errors.models_info) if obj_ids is None else [int(o) for o in obj_ids]
        self._records = None

    def add(self, scene_id, im_id, obj_id, score, T_est, K):
        super().add(scene_id, im_id, obj_id, score, T_est, K)
        self._records = None

    # -- eval_calc_errors.py ---------------------------------------------------------------------------------
    def _device_errors(self, pairs):
        """Error lists of the pairs that passed the shortcuts: ``pairs`` = [(scene, im, obj, T_est, T_gt, K)]."""
        et = self.error_type
        if not pairs:
            return []
        if et == "vsd":
            return vsd_runs(self.errors, self.depth_loader, pairs, delta=self.vsd_delta, taus=self.vsd_taus, normalized=self.vsd_normalized_by_diameter)
        objs, Te, Tg, K = _stacked(pairs)
        if et in ("mssd", "mspd"):
            mssd, mspd = self.errors.errors(objs, Te, Tg, K)
            return [[e] for e in (mssd if et == "mssd" else mspd).tolist()]
        if et in ("add", "adi", "proj"):
            return [[e] for e in self.errors.point_errors(objs, Te, Tg, K, which=(et,))[et].tolist()]
        if et == "ad":                                                      # eval_calc_errors.py:340-346
            out = [None] * len(pairs)
            for name, pick in (("adi", True), ("add", False)):
                ii = [i for i, o in enumerate(objs) if (o in self.symmetric_obj_ids) == pick]
                if ii:
                    e = self.errors.point_errors([objs[i] for i in ii], Te[ii], Tg[ii], K[ii], which=(name,))[name].tolist()
                    for i, v in zip(ii, e):
                        out[i] = [v]
            return out
        if et == "cus":
            return [[e] for e in self.errors.mask_errors(objs, Te, Tg, K, self.im_hw)["cus"].tolist()]
        out = []
        for te_, tg_ in zip(Te, Tg):
            re_, tr_ = float(rotation_error(te_[:, :3], tg_[:, :3])), float(translation_error(te_[:, 3], tg_[:, 3]))
            out.append([re_, tr_] if et == "rete" else [re_] if et == "re" else [tr_])
        return out

    def error_records(self):
        """``{scene_id: [{"im_id", "obj_id", "est_id", "score", "errors": {gt_id: [e, ...]}}]}`` in the script's order: what eval_calc_errors.py holds in
        ``scene_errs`` before it saves (vsd: one element per tau).  Computed once per set of estimates."""
        if self._records is not None:
            return self._records
        et, records, pairs, where = self.error_type, {s: [] for s in self.targets}, [], []
        for s, im, o, est_id, est, gts in self._walk(self.n_top):
            row = {"im_id": im, "obj_id": o, "est_id": est_id, "score": est["score"], "errors": {}}
            records[s].append(row)
            for gt_id, Tg in gts:
                if et in ("vsd", "cus") and not projections_overlap(self.errors.models_info[o]["diameter"], est["T"], Tg):
                    row["errors"][gt_id] = [1.0] * (len(self.vsd_taus) if et == "vsd" else 1)
                elif et in ("ad", "add", "adi", "mssd") and not centres_within(self.errors.models_info[o]["diameter"], est["T"], Tg):
                    row["errors"][gt_id] = [float("inf")]
                else:
                    row["errors"][gt_id] = None                 # keeps the ground truths in their order
                    pairs.append((s, im, o, est["T"], Tg, est["K"]))
                    where.append((row, gt_id))
        for (row, gt_id), e in zip(where, self._device_errors(pairs)):
            row["errors"][gt_id] = e
        self._records = records
        return records

    def error_sign(self, tau_index=0):
        return error_signature(self.error_type, self.n_top, vsd_delta=self.vsd_delta, vsd_tau=self.vsd_taus[tau_index] if self.error_type == "vsd" else None)

    def score_sign(self):
        return score_signature(self.correct_th, self.visib_gt_min)

    def errors_json(self, scene_id, tau_index=0):
        """The list eval_calc_errors.py saves as ``errors_<scene_id>.json`` (for vsd: the file of tau ``tau_index``)."""
        pick = (lambda e: [e[tau_index]]) if self.error_type == "vsd" else (lambda e: list(e))
        return [{"im_id": r["im_id"], "obj_id": r["obj_id"], "est_id": r["est_id"], "score": r["score"], "errors": {g: pick(e) for g, e in r["errors"].items()}}
                for r in self.error_records()[scene_id]]

    # -- eval_calc_scores.py ---------------------------------------------------------------------------------
    def valid_gts(self, scene_id, im_id):
        gts, infos, im_targets = self.scene_gt[scene_id][im_id], self.scene_gt_info[scene_id][im_id], self.targets[scene_id][im_id]
        if self.visib_gt_min >= 0:
            return [gt["obj_id"] in im_targets and infos[g]["visib_fract"] >= self.visib_gt_min for g, gt in enumerate(gts)]
        return valid_gt_mask([gt["obj_id"] for gt in gts], [i["visib_fract"] for i in infos], im_targets)

    def matches(self, tau_index=0):
        """The list eval_calc_scores.py saves as ``matches_*.json``: one record per ground truth of the target images (pose_matching.match_poses_scene)."""
        out = []
        factor = 640.0 / self.im_width
        for s, ims in self.targets.items():
            by_im = {}
            for r in self.errors_json(s, tau_index):
                if self.error_type in NORMALIZED_BY_DIAMETER:
                    diameter = float(self.errors.models_info[r["obj_id"]]["diameter"])
                    r["errors"] = {g: [e / diameter for e in es] for g, es in r["errors"].items()}
                if self.error_type in NORMALIZED_BY_IM_WIDTH:
                    r["errors"] = {g: [factor * e for e in es] for g, es in r["errors"].items()}
                by_im.setdefault(r["im_id"], {}).setdefault(r["obj_id"], []).append(r)
            for im in ims:
                gts, valid = self.scene_gt[s][im], self.valid_gts(s, im)
                im_matches = [{"scene_id": s, "im_id": im, "obj_id": gt["obj_id"], "gt_id": g, "est_id": -1, "score": -1, "error": -1, "error_norm": -1,
                               "valid": valid[g]} for g, gt in enumerate(gts)]
                for o in {gt["obj_id"] for gt in gts}:
                    for m in match_poses_elements(by_im.get(im, {}).get(o, []), self.correct_th, self.n_top, valid):
                        im_matches[m["gt_id"]].update(est_id=m["est_id"], score=m["score"], error=m["error"], error_norm=m["error_norm"])
                out += im_matches
        return out

    def result(self, tau_index=0):
        """Exactly the dictionary of score.calc_localization_scores: ``recall``, ``obj_recalls``, ``mean_obj_recall``, ``scene_recalls``,
        ``mean_scene_recall``, ``gt_count``, ``targets_count``, ``tp_count``."""
        return localization_scores(self.scene_ids, self.obj_ids, self.matches(tau_index), self.n_top)

    def parameters(self, tau_index=0):
        p = {"error_type": self.error_type, "n_top": self.n_top, "visib_gt_min": self.visib_gt_min, "correct_th": list(self.correct_th)}
        if self.error_type == "vsd":
            p.update(vsd_delta=self.vsd_delta, vsd_tau=self.vsd_taus[tau_index], vsd_normalized_by_diameter=self.vsd_normalized_by_diameter)
        return p
