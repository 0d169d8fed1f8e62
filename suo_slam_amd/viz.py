"""A view's three-panel visualisation (collect_results(no_viz=False)), painted on the device.

What lib/object_slam.py:226-274 and lib/utils/utils.py:182-354 (draw_points, bbox_color, make_kp_viz) do per view -- left: the frame with the input boxes and the
prior heat of the symmetric objects blended in; centre: the detected keypoints, with their covariance ellipses under ``viz_cov``; right: every mesh painted at
its estimated pose -- split in two:

    build_primitives(shape, K, obj_ids, detection, poses, draw_cov)    the reference's own expressions in numpy, verbatim, up to the LIST of primitives
    Visualizer(mesh_db, H, W).render(frame, prims)                     -> HIP, csrc/viz.hip (suo_viz_view): uint8 [H,3W,3]

include/suo_hip.h states how each primitive is rasterised (cv2 is absent: those rules are oracle-unpinned) and DESIGN.md 6 the two deviations: putText labels
are not drawn, and ``do_viz_extra`` (the per-object crops of the paper's figures) is not built.  The dtype flow is the reference's: keypoint centres go through
a float32 array before Python's round, and a covariance is propagated in fp64, stored as float32 and decomposed by np.linalg.eig in that type."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib

NUM_KP = 41
KP_RAD = 8                                        # make_kp_viz's rad
PRIOR_HALF = 45                                   # draw_gaussian_2d: tmpSize = ceil(3 sigma), sigma = 15
LIM = 1 << 30                                     # integer coordinates are clipped to +-2^30 before they become int32: no canvas reaches that far
MAX_KP, MAX_OBJ = 656, 64                         # SUO_VIZ_MAX_KP, SUO_VIZ_MAX_OBJ

_tables = None


def colour_tables():
    """(kp_colors() int [41,3], bbox_color's table int [30,3]), BGR: the reference's two tables, kept as data in the library (suo_viz_colours)."""
    global _tables
    if _tables is None:
        kp, bb = np.zeros((NUM_KP, 3), np.uint8), np.zeros((30, 3), np.uint8)
        _lib.check(_lib.lib().suo_viz_colours(kp.ctypes.data, bb.ctypes.data), "suo_viz_colours")
        _tables = (kp.astype(np.int64), bb.astype(np.int64))
    return _tables


def bbox_color(obj_id):
    """utils.bbox_color (:248-251): cols[obj_id - 1] with Python's indexing (obj_id 0, the row of an undetected object, takes the last entry)."""
    cols = colour_tables()[1]
    if int(obj_id) > len(cols):
        raise ValueError(f"bbox_color: obj_id {obj_id} is beyond the table's {len(cols)} entries")
    return cols[int(obj_id) - 1].tolist()


def pack(bgr):
    return int(bgr[0]) | int(bgr[1]) << 8 | int(bgr[2]) << 16


def _clip(v):
    return int(min(max(int(v), -LIM), LIM))


def build_primitives(shape, K, obj_ids, detection, poses, draw_cov):
    """The primitives of one view.  ``shape``: (H, W); ``K``: the view's camera matrix; ``obj_ids``: the objects in the order collect_results walks them;
    ``detection``: {obj_id: detection} of the view; ``poses``: {obj_id: T_OtoC 4x4} of the objects with a map pose, in that order; ``draw_cov``: ellipses
    (``viz_cov and not no_network_cov``).  Returns the dict tests/viz_ref.py documents, plus "box_obj" (the boxes' obj_id column)."""
    vh, vw = int(shape[0]), int(shape[1])
    obj_ids = list(obj_ids)
    n = len(obj_ids)
    kp_cols = colour_tables()[0]
    # object_slam.py:203-255
    kp_pred = np.zeros((n, NUM_KP, 2), dtype=np.float32)
    kp_cov = np.zeros((n, NUM_KP, 2, 2), dtype=np.float32) if draw_cov else None
    kp_mask = np.zeros((n, NUM_KP), dtype=bool)
    bboxes = np.zeros((n, 5), dtype=int)
    stamps = []
    for i, obj_id in enumerate(obj_ids):
        if obj_id not in detection:
            continue
        det_obj = detection[obj_id]
        kp_mask_i = np.asarray(det_obj["kp_mask"], dtype=bool)
        H = (np.asarray(K) @ np.linalg.inv(det_obj["K"])).T
        kp_pred[i][kp_mask_i] = det_obj["uv_pred"] @ H[:2, :2] + H[2:3, :2]
        kp_mask[i] = kp_mask_i
        bboxes[i][0] = obj_id
        bboxes[i][1:] = (np.asarray(det_obj["bbox"]) + 0.5).astype(int)
        if draw_cov:
            assert det_obj.get("cov_pred") is not None
            kp_cov[i][kp_mask_i] = H[:2, :2].T[None, None, ...] @ det_obj["cov_pred"] @ H[None, None, :2, :2]
        if det_obj["prior_uv"] is not None:
            prior_uv_full = det_obj["prior_uv"] @ H[:2, :2] + H[2:3, :2]
            x1, y1, x2, y2 = (int(v) for v in bboxes[i][1:])
            wx0, wx1, _ = slice(x1, x2).indices(vw)          # what [y1:y2, x1:x2] selects (:253-255)
            wy0, wy1, _ = slice(y1, y2).indices(vh)
            mask = det_obj["model_kp_mask"]
            for k in range(prior_uv_full.shape[0]):          # utils.make_prior_kp_input (:398-411), ndc=False; draw_gaussian_2d (:364-385)
                if mask[k] and np.all(np.isfinite(prior_uv_full[k, :2])):
                    u, v = prior_uv_full[k, :2]
                    if abs(u) >= LIM or abs(v) >= LIM:
                        continue                             # (its window misses every canvas)
                    pt = (int(round(u)), int(round(v)))
                    stamps.append((k, pt[0] - PRIOR_HALF, pt[1] - PRIOR_HALF, wx0, max(wx1, wx0), wy0, max(wy1, wy0), obj_id))
    # make_kp_viz(bbox_pred=bboxes): utils.py:314-320, one rectangle per row -- the zero row of an undetected object included
    box = [(_clip(x1), _clip(y1), _clip(x2), _clip(y2), pack(bbox_color(o))) for o, x1, y1, x2, y2 in bboxes]
    # make_kp_viz(kp_pred, kp_mask, cov, ndc=False) -> draw_points: utils.py:332-337, :208-242
    kp, kp_angle = [], []
    for i in range(n):
        uv = kp_pred[i][kp_mask[i]]
        cov_i = kp_cov[i][kp_mask[i]] if draw_cov else None
        cols = kp_cols[kp_mask[i]]
        for j in range(len(cols)):
            x, y = uv[j, :2]
            if not (np.isfinite(x) and np.isfinite(y)):
                continue                                     # (the reference's int(round(nan)) raises; a picture is not worth a crash)
            x = int(round(x))
            y = int(round(y))
            if x < 0 or y < 0 or x >= vw or y >= vh:
                continue
            col = cols[j].tolist()
            rec, ang = [x, y, int(round(1.3 * KP_RAD)), int(round(KP_RAD)), pack(col), 0, 0, 0], 0.0
            if cov_i is not None:
                lamb, v = np.linalg.eig(cov_i[j])
                angle = np.arctan2(v[1, 0], v[0, 0])
                s = 1.0 / 3
                axes_length = (int(round(s * 2 * np.sqrt(5.991 * lamb[0]))), int(round(s * 2 * np.sqrt(5.991 * lamb[1]))))
                rec[5:], ang = [1, axes_length[0], axes_length[1]], float(180 * angle / np.pi)
            kp.append(rec)
            kp_angle.append(ang)
    # make_kp_viz(poses=...): utils.py:275-311
    poses_sorted = sorted(list(poses.items()), key=lambda p: -p[1][2, 3])
    overlay = [(o, pack(bbox_color(o)), np.asarray(T, np.float64)[:3, :4].copy(), np.asarray(K, np.float64).reshape(3, 3).copy()) for o, T in poses_sorted]
    return {"box": np.array(box, np.int64).reshape(-1, 5), "box_obj": bboxes[:, 0].copy(), "stamp": np.array(stamps, np.int64).reshape(-1, 8),
            "kp": np.array(kp, np.int64).reshape(-1, 8), "kp_angle": np.array(kp_angle, np.float64), "overlay": overlay}


def view_primitives(slam, view_id):
    """build_primitives of one view of an ObjectSLAM, from the state collect_results reads (object_slam.py:188-220)."""
    T_GtoC = np.asarray(slam.cam_poses[view_id], np.float64)
    if T_GtoC.shape[0] == 3:
        T_GtoC = np.concatenate((T_GtoC, np.eye(4)[3:4, :]), axis=0)
    detection = slam.detections[view_id]
    obj_ids = set(list(slam.obj_poses.keys()) + list(detection.keys()))
    poses = {}
    for obj_id in obj_ids:
        if obj_id in slam.obj_poses:
            T_OtoG = np.asarray(slam.obj_poses[obj_id], np.float64)
            if T_OtoG.shape[0] == 3:
                T_OtoG = np.concatenate((T_OtoG, np.eye(4)[3:4, :]), axis=0)
            poses[obj_id] = T_GtoC @ T_OtoG
    return build_primitives(slam.images[view_id].shape[:2], slam.cam_K[view_id], obj_ids, detection, poses, bool(slam.viz_cov and not slam.no_network_cov))


def _points_numpy(p):
    if hasattr(p, "detach"):
        p = p.detach().cpu().numpy()
    return np.ascontiguousarray(p, np.float32).reshape(-1, 3)


class Visualizer:
    """Owns a suo_viz handle for H x W frames and a mesh database of the objects of ``mesh_db`` that carry "points" ({obj_id: {"points": [P,3]}})."""

    def __init__(self, mesh_db, H, W):
        self.lib = _lib.lib()
        _lib.require_gpu()
        self.H, self.W = int(H), int(W)
        self._h = self._db = None
        ids = [o for o in mesh_db if "points" in mesh_db[o]]
        self._index = {o: i for i, o in enumerate(ids)}
        if ids:
            clouds = [_points_numpy(mesh_db[o]["points"]) for o in ids]
            n_pts = np.array([len(c) for c in clouds], np.int32)
            allpts = np.ascontiguousarray(np.concatenate(clouds), np.float32)
            h = C.c_void_p()
            _lib.check(self.lib.suo_mesh_db_create(len(clouds), n_pts.ctypes.data, allpts.ctypes.data, C.byref(h)), "suo_mesh_db_create")
            self._db = h
        h = C.c_void_p()
        _lib.check(self.lib.suo_viz_create(self.H, self.W, C.byref(h)), "suo_viz_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self.lib.suo_viz_destroy(self._h)
            self._h = None
        if getattr(self, "_db", None):
            self.lib.suo_mesh_db_destroy(self._db)
            self._db = None

    __del__ = close

    def descriptor(self, prims):
        """(VizViewDesc without its frame, the arrays it points into) of build_primitives' dict.  ValueError for an overlay object without points."""
        i32 = lambda a, w: np.ascontiguousarray(np.asarray(a, np.int64).reshape(-1, w), np.int32)        # noqa: E731
        box, stamp, kp = i32(prims["box"], 5), i32(np.clip(prims["stamp"], -LIM, LIM), 8), i32(prims["kp"], 8)
        # cv2.ellipse takes degrees; the rule's cos / sin are those of phi = degrees * pi / 180, formed here in fp64 (the device only multiplies and adds)
        phi = [float(a) * math.pi / 180 for a in prims["kp_angle"]]
        cs = np.array([[math.cos(p), math.sin(p)] for p in phi], np.float64).reshape(-1, 2)
        ov = prims["overlay"]
        missing = [o for o, *_ in ov if o not in self._index]
        if missing:
            raise ValueError(f"Visualizer: objects {missing} have a pose but no points in the mesh database")
        model = np.array([self._index[o] for o, *_ in ov], np.int32)
        colour = np.array([c for _, c, _, _ in ov], np.int32)
        T = np.ascontiguousarray(np.array([t for _, _, t, _ in ov], np.float64).reshape(-1, 12))
        K = np.ascontiguousarray(np.array([k for _, _, _, k in ov], np.float64).reshape(-1, 9))
        keep = (box, stamp, kp, cs, model, colour, T, K)
        d = _lib.VizViewDesc(None, len(box), box.ctypes.data, len(stamp), stamp.ctypes.data, len(kp), kp.ctypes.data, cs.ctypes.data,
                             len(model), model.ctypes.data, colour.ctypes.data, T.ctypes.data, K.ctypes.data)
        return d, keep

    def render_device(self, frame, prims):
        """The canvas as a torch uint8 [H,3W,3] tensor on the device, enqueued on torch's current stream (no host synchronisation).  ``frame``: uint8 [H,W,3]
        BGR, a numpy array or a tensor on the device.  The library stages a call's primitives in a ring of 8 pinned slots: wait for the stream before a ninth
        view of this handle is enqueued behind eight unfinished ones (render() waits every time)."""
        import torch
        if not torch.is_tensor(frame):
            frame = torch.from_numpy(np.ascontiguousarray(frame, np.uint8))
        frame = frame.to("cuda").contiguous()
        if frame.dtype != torch.uint8 or tuple(frame.shape) != (self.H, self.W, 3):
            raise ValueError(f"Visualizer: frame {tuple(frame.shape)} {frame.dtype} is not uint8 [{self.H},{self.W},3]")
        d, keep = self.descriptor(prims)
        d.frame = frame.data_ptr()
        out = torch.empty((self.H, 3 * self.W, 3), dtype=torch.uint8, device=frame.device)
        _lib.check(self.lib.suo_viz_view(self._h, C.byref(d), self._db, out.data_ptr(), _lib.current_stream_ptr()), "suo_viz_view")
        return out

    def render(self, frame, prims):
        return self.render_device(frame, prims).cpu().numpy()
