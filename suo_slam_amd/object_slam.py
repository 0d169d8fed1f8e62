"""Host-side mirror of the reference's ``ObjectSLAM`` driver (/root/reference/lib/object_slam.py:51-1167)
for the hot path: same public methods, argument order and state dictionaries (``detections``,
``cam_poses``, ``obj_poses``), so an ``evaluate.py``-shaped harness can call it unchanged:

    ObjectSLAM(chkpt_path, mesh_db, ...)                 object_slam.py:52-57
    reset()                                              :125-153
    process_view(view_id, img, K, obj_ids, bboxes, model_kps, model_kps_masks, kp_masks, uv_gt, cam_pose)  :327-451
    collect_results(last_only, no_viz, final)            :175-274 (no_viz=False: the three-panel picture, suo_slam_amd/viz.py -> csrc/viz.hip)
    optimize(curr_only)                                  :703-930
    pnp(points_3d, points_2d, camera_matrix)             :25-41

What differs is where the work runs: the network, the keypoint masks, PnP for all objects of the frame
and every LM round execute in libsuo_hip.so (HIP, gfx950); this file only keeps the reference's
bookkeeping: the map state, the rules (thresholds, acceptance / removal / re-initialisation) and the host route
of a pass (_run_kp_model), which restates the reference's data flow.  The routes that keep a view's keypoints on
the device between the network and the poses are the base class, view_chain.DeviceRoutes.  There is no CPU fallback.
"""
from __future__ import annotations

from collections import defaultdict
from time import time

import numpy as np

from . import ba as _ba
from . import lambdatwist as _lt
from . import slam_score as _sc
from .geometry import fix_K_for_bbox_ndc, fix_K_for_bbox_ndc_many, invert_SE3, normalize_uv, to4x4
from .view_chain import CHI2_2DOF_95, DeviceRoutes, _on_stream, prior_arrays
from .weights import NUM_KP


class AverageMeter:
    """lib/utils/eval_meter.py:47-63."""

    def __init__(self):
        self.sum = 0.0
        self.count = 0

    def update(self, val, n=1):
        self.sum += float(val) * n
        self.count += n

    def average(self):
        return self.sum / self.count if self.count > 0 else 0.0


def pnp(points_3d, points_2d, camera_matrix):
    """object_slam.py:25-41: PnP pose [3,4] + all-true inlier mask, or None (needs >= 4 points; the
    identity pose is the native failure code)."""
    assert points_3d.shape[0] == points_2d.shape[0], "points 3D and points 2D must have same number of rows"
    assert camera_matrix.shape == (3, 3), "Camera matrix must be of shape (3,3)"
    n = points_3d.shape[0]
    if n < 4:
        return None
    res = _lt.pnp(np.asarray(points_3d, np.float64), normalize_uv(np.asarray(points_2d, np.float64), camera_matrix))
    if np.allclose(res, np.eye(4)):
        return None
    return res[:3, :], np.ones(n, dtype=bool)


# ---- prior heat-maps (lib/utils/utils.py:356-411) ------------------------------------------------
def _gaussian_patch(size=91):
    """gaussian_2d(): a unit impulse blurred by cv2.GaussianBlur(ksize=size, sigma=0) and divided by its
    max.  OpenCV derives sigma = 0.3*((size-1)*0.5-1)+0.8 (= 14.0 for 91) and reflects at the border
    (BORDER_REFLECT_101), which doubles the outermost ring of the impulse response."""
    sigma = 0.3 * ((size - 1) * 0.5 - 1) + 0.8
    i = np.arange(size, dtype=np.float64) - (size - 1) / 2
    k = np.exp(-(i * i) / (2 * sigma * sigma))
    k /= k.sum()
    k[0] *= 2
    k[-1] *= 2
    g = np.outer(k, k)
    return (g / g.max()).astype(np.float32)


_PATCH = None


def draw_gaussian_2d(img, pt, sigma=15):
    """utils.py:364-385: paste (assign) the 91x91 patch around pt=(x,y); window [pt-45, pt+45)."""
    global _PATCH
    tmp = int(np.ceil(3 * sigma))
    ul = [int(np.floor(pt[0] - tmp)), int(np.floor(pt[1] - tmp))]
    br = [int(np.floor(pt[0] + tmp)), int(np.floor(pt[1] + tmp))]
    H, W = img.shape
    if ul[0] > W or ul[1] > H or br[0] < 1 or br[1] < 1:
        return img
    if _PATCH is None or _PATCH.shape[0] != 2 * tmp + 1:
        _PATCH = _gaussian_patch(2 * tmp + 1)
    gx = [max(0, -ul[0]), min(br[0], W) - max(0, ul[0]) + max(0, -ul[0])]
    gy = [max(0, -ul[1]), min(br[1], H) - max(0, ul[1]) + max(0, -ul[1])]
    ix = [max(0, ul[0]), min(br[0], W)]
    iy = [max(0, ul[1]), min(br[1], H)]
    img[iy[0]:iy[1], ix[0]:ix[1]] = _PATCH[gy[0]:gy[1], gx[0]:gx[1]]
    return img


def make_prior_kp_input(kp_uv, kp_uv_mask, img_shape, ndc=True):
    """utils.py:398-411: one Gaussian stamp per valid keypoint channel."""
    n = kp_uv.shape[0]
    vh, vw = img_shape
    x = np.zeros((n, vh, vw), dtype=np.float32)
    for i in range(n):
        if kp_uv_mask[i] and np.all(np.isfinite(kp_uv[i, :2])):
            u, v = float(kp_uv[i, 0]), float(kp_uv[i, 1])
            if ndc:
                u = (min(max(u, -1), 1) * vw / 2 + vw / 2) - 0.5
                v = vh - 0.5 - (min(max(v, -1), 1) * vh / 2 + vh / 2)
            draw_gaussian_2d(x[i], (int(round(u)), int(round(v))))
    return x


def _det_cache(d):
    """Padded copies of a detection's immutable arrays (keypoints, predictions, covariances, intrinsics), built once
    per detection: the scoring rules below run O(objects^2 + 15 objects) times per SLAM view and the graph assembly
    once per keypoint, which as per-detection numpy calls dominated a view's host time."""
    c = d.get("_cache")
    if c is not None and c["src"][0] is d["uv_pred"] and c["src"][1] is d["cov_pred"] and c["src"][2] is d["model_kp"] and c["src"][3] is d["K"]:
        return c
    n = int(d["uv_pred"].shape[0])
    nk = max(NUM_KP, n)
    pts = np.zeros((nk, 3))
    uv = np.zeros((nk, 2))
    pts[:n] = d["model_kp"]
    uv[:n] = d["uv_pred"]
    cov = None
    if d["cov_pred"] is not None:
        cov = np.zeros((nk, 2, 2))
        cov[:, 0, 0] = cov[:, 1, 1] = 1.0
        cov[:n] = np.asarray(d["cov_pred"], dtype=np.float64)
    c = {"src": (d["uv_pred"], d["cov_pred"], d["model_kp"], d["K"]), "n": n, "pts": pts, "uv": uv, "cov": cov,
         "K": np.asarray(d["K"], dtype=np.float64)}
    d["_cache"] = c
    return c


def _det_edges(d):
    """Per-keypoint graph-edge data of a detection (object_slam.py:795-821): information matrices [n,3] as
    (xx, xy, yy) and the pinhole parameters (fx, fy, cx, cy)."""
    c = _det_cache(d)
    if "info" not in c:
        Kd = c["K"]
        # (np.allclose's rule -- |a - b| <= 1e-8 + 1e-5 |b| -- on five scalars: the numpy call costs 15 us per detection on the view's critical path)
        assert (abs(Kd[0, 1]) <= 1e-8 and abs(Kd[1, 0]) <= 1e-8 and abs(Kd[2, 0]) <= 1e-8 and abs(Kd[2, 1]) <= 1e-8 and abs(Kd[2, 2] - 1.0) <= 1e-8 + 1e-5), \
            f"K matrix has off-diagonals!\n\n{Kd}"
        n = c["n"]
        if d["cov_pred"] is not None and n > 0:
            # np.linalg.inv(cov_uv[k]) in the covariance's OWN dtype (float32 from the network, :825-828), then g2o's doubles;
            # the kernels keep Omega as (xx, xy, yy): its symmetric part is all that error^T Omega error sees
            Om = np.linalg.inv(np.asarray(d["cov_pred"]).reshape(n, 2, 2)).astype(np.float64)
            info = np.stack([Om[:, 0, 0], 0.5 * (Om[:, 0, 1] + Om[:, 1, 0]), Om[:, 1, 1]], axis=1)
        else:
            info = np.tile(np.array([1.0, 0.0, 1.0]), (n, 1))
        c["info"] = info
        c["camk"] = np.array([Kd[0, 0], Kd[1, 1], Kd[0, 2], Kd[1, 2]])
    return c


class _EdgeRefs:
    """(view, object, keypoint) of every graph edge, kept as per-detection segments [(view, object, first edge, n)]."""

    def __init__(self, segs, n_edges):
        self.segs, self.n_edges = segs, n_edges

    def __len__(self):
        return self.n_edges

    def __iter__(self):
        for v, o, _, n in self.segs:
            for k in range(n):
                yield (v, o, k)


class ObjectSLAM(DeviceRoutes):
    def __init__(self, chkpt_path, mesh_db, no_network_cov=False, no_prior_det=False, pred_res=(256, 256),
                 debug_gt_kp=False, sfm_mode=False, single_view_mode=False, viz_cov=False, do_viz_extra=False,
                 global_opt_every=10, kp_var_thresh=0.2, bbox_thresh=0.9, bbox_inflate=0.0, manual_kp_std=0.005,
                 opt_init_with_outliers=False, give_all_prior=False, state_dict=None, max_crops=16, seed=0, verbose=False,
                 device_chain=True, run_network_in_debug=False, debug_gt_on_device=False):
        """Same keyword surface as the reference.  ``chkpt_path`` is a torch checkpoint whose ``['model']`` is the
        PkpNet state_dict (object_slam.py:92-97); ``state_dict`` may be given directly instead."""
        self.mesh_db = mesh_db
        self.no_network_cov = no_network_cov or debug_gt_kp
        self.no_prior_det = no_prior_det
        self.pred_res = list(pred_res)
        self.debug_gt_kp = debug_gt_kp
        self.sfm_mode = sfm_mode
        self.single_view_mode = single_view_mode
        self.slam_mode = not (sfm_mode or single_view_mode)
        self.global_opt_every = global_opt_every
        self.kp_var_thresh = kp_var_thresh
        self.bbox_thresh = bbox_thresh
        self.bbox_inflate = bbox_inflate
        self.manual_kp_std = manual_kp_std
        self.opt_init_with_outliers = opt_init_with_outliers
        self.give_all_prior = give_all_prior
        self.verbose = verbose
        self.viz_cov = bool(viz_cov)           # collect_results(no_viz=False): covariance ellipses on the centre panel (suo_slam_amd/viz.py)
        self.do_viz_extra = bool(do_viz_extra)  # the paper figures' per-object crops: not built, collect_results(no_viz=False) raises NotImplementedError
        self._visualizer = None                # viz.Visualizer of the current frame size, made by the first collect_results(no_viz=False)
        # single-view frames: masks -> compaction -> PnP -> acceptance -> graph -> LM as ONE device chain behind the network
        # (suo_slam_amd/frame_geom.py); False = the host route that restates the reference's data flow (three read-backs, Python lists)
        self.device_chain = bool(device_chain)
        super().__init__()                     # what this object keeps on the GPU between views (view_chain.DeviceRoutes)
        self._score_store = None               # the scene's detections on the device, made by slam_score.chi2_counts at its first call; cleared with the map
        self._rng = np.random.default_rng(seed)
        self._pnp_seed = int(seed)
        self.reset()
        self.model = None
        self.model_epoch = -1
        # benchmark aid: in --debug_gt_kp mode ALSO run the network (both passes, device-rendered priors, masks, read-back) on the
        # frame's pixels and discard what it says in favour of the ground-truth keypoints -- random weights give meaningless
        # keypoints, a SLAM sequence needs meaningful ones, and the view's time must include the network
        self.run_network_in_debug = bool(run_network_in_debug and debug_gt_kp and state_dict is not None)
        # ... and, with debug_gt_on_device, make that substitution WHERE THE NETWORK'S OUTPUT LIES: the ground-truth keypoints (+ the same noise draws) overwrite the
        # device tensors in float32 -- the type the network emits -- and the view continues on the product route (_run_kp_model_chain), not on the host restatement
        self.debug_gt_on_device = bool(debug_gt_on_device and self.run_network_in_debug and device_chain)
        if not debug_gt_kp or self.run_network_in_debug:
            from .pkpnet import PkpNet
            if state_dict is None:
                import torch
                ck = torch.load(chkpt_path, map_location="cpu")
                state_dict = ck["model"]
                self.model_epoch = ck.get("epoch", -1)
            self.model = PkpNet(calc_cov=True, state_dict=state_dict, max_crops=max_crops)
            import torch
            self._gpu_stream = torch.cuda.Stream(device=self.model.device)
            # frames carry a varying number of detections: capture the graph of every crop count now, not inside a timed view
            self.model.prepare(with_priors=(False,) if (single_view_mode or no_prior_det) else (False, True))
        self.fp16_range_reissues = 0          # network calls re-issued on the bf16x3 form because an activation left fp16's range (reported by Evaluator.run / bench.py)
        self.avg_std_meter = AverageMeter()
        self.track_time_meter = AverageMeter()
        self.opt_time_meter = AverageMeter()
        self.all_time_num_views = 0

    def _log(self, *a):
        if self.verbose:
            print(*a)

    def reset(self):
        self.detections = {}
        self.cam_poses = {}
        self.view_ids = []
        self.cam_K = {}
        self.images = {}
        self.obj_poses = {}
        self.obj_num_dets = defaultdict(int)
        self.obj_num_det_kps = defaultdict(int)
        self.remove_penalty = defaultdict(int)
        self.needs_opt = False
        if self._score_store is not None:
            self._score_store.clear()

    def num_views_processed(self):
        return len(self.cam_poses)

    def obj_num_inliers(self, obj_id):
        n = 0
        for det in self.detections.values():
            n += int(np.count_nonzero(det.get(obj_id, {}).get("inliers", np.array([]))))
        return n

    def remove_obj(self, obj_id):
        self.obj_poses.pop(obj_id)

    def get_tracking_strtime(self, tt0=np.nan, tt1=np.nan):
        avg = self.track_time_meter.average()
        return f"TIMING: Tracking time: {1000 * (tt1 - tt0):.3f} ms ({1000 * avg:.3f} avg) ({'inf' if avg < 1e-12 else 1 / avg} Hz)"

    def get_global_opt_strtime(self, t0=np.nan, t1=np.nan):
        avg = self.opt_time_meter.average()
        return f"TIMING: Global opt time: {1000 * (t1 - t0)} ms ({1000 * avg} avg) ({'inf' if avg < 1e-12 else 1 / avg} Hz)"

    # ---------------------------------------------------------------------------------------------
    def collect_results(self, last_only=False, no_viz=True, final=False, covariances=False):
        """object_slam.py:175-225: T_OtoC = T_GtoC @ T_OtoG per view; score = 1 + total inliers.  covariances=True: every pose entry also carries "cov_OtoC", the
        6x6 covariance of that T_OtoC (pose_covariances(relative=True)), None where T_OtoC is None.  no_viz=False (:226-274): every view also carries "viz", the
        three-panel picture uint8 [H,3W,3] BGR painted on the device (suo_slam_amd/viz.py; ellipses under viz_cov and not no_network_cov).  The default stays
        no_viz=True, unlike the reference's, and the dict is then exactly what it was."""
        if not no_viz and self.do_viz_extra:
            raise NotImplementedError("do_viz_extra (the per-object crops of the paper's figures, object_slam.py:276-325) is not built: DESIGN.md 6")
        if self.slam_mode and self.needs_opt and final:
            t0 = time()
            self.optimize()
            self.opt_time_meter.update(time() - t0)
        results = {}
        n_inl = {}                     # per object, the same for every view: counted once (the reference recounts per view, :199-214)
        assert len(self.view_ids) == len(self.cam_poses)
        views = [self.view_ids[-1]] if last_only else self.view_ids
        rel = self.pose_covariances(view_ids=views, relative=True)["rel"] if covariances else None
        for view_id in views:
            T_GtoC = to4x4(self.cam_poses[view_id])
            detection = self.detections[view_id]
            results[view_id] = {"poses": {}}
            for obj_id in set(list(self.obj_poses.keys()) + list(detection.keys())):
                T_OtoC = None
                if obj_id in self.obj_poses:
                    T_OtoC = T_GtoC @ to4x4(self.obj_poses[obj_id])
                if obj_id not in n_inl:
                    n_inl[obj_id] = self.obj_num_inliers(obj_id)
                results[view_id]["poses"][obj_id] = {"T_OtoC": T_OtoC, "score": 1 + n_inl[obj_id]}
                if covariances:
                    results[view_id]["poses"][obj_id]["cov_OtoC"] = None if T_OtoC is None else rel[(view_id, obj_id)]
            if not no_viz:
                results[view_id]["viz"] = self._viz_view(view_id)
        return results

    def _viz_view(self, view_id):
        """The view's picture: the primitives are the reference's host arithmetic (viz.view_primitives), the painting one stream-ordered device call."""
        from . import viz
        img = self.images[view_id]
        if self._visualizer is None or (self._visualizer.H, self._visualizer.W) != tuple(img.shape[:2]):
            if self._visualizer is not None:
                self._visualizer.close()
            self._visualizer = viz.Visualizer(self.mesh_db, img.shape[0], img.shape[1])
        frame = self._frame_dev if self._frame_key == (id(img), getattr(img, "shape", None)) else None      # the frame _frame_on_device uploaded, when it is this view's
        if frame is None or not hasattr(frame, "is_cuda") or not frame.is_cuda or tuple(frame.shape) != tuple(img.shape) or str(frame.dtype) != "torch.uint8":
            frame = img
        return self._visualizer.render(frame, viz.view_primitives(self, view_id))

    # ---------------------------------------------------------------------------------------------
    @_on_stream
    def process_view(self, view_id, img, K, obj_ids, bboxes, model_kps, model_kps_masks, kp_masks, uv_gt=None, cam_pose=None):
        """object_slam.py:327-451."""
        assert view_id not in self.cam_poses, f"Repeat view_id {view_id}"
        if self.views_in_flight():                          # (their results carry PnP sampler keys that continue from _pnp_seed: a view in between would reuse them)
            raise RuntimeError("process_view: batches of submit_views_single are still in flight -- collect them first")
        import torch
        self._frame_key = self._frame_dev = None            # (the frame is uploaded once per view: _frame_on_device)
        if self.model is not None:
            torch.cuda.synchronize()
        tt0 = time()
        obj_ids = np.asarray(obj_ids)
        bboxes = np.array(bboxes, dtype=np.float64)
        model_kps = np.asarray(model_kps)
        model_kps_masks = np.asarray(model_kps_masks, dtype=bool)
        kp_masks = np.asarray(kp_masks, dtype=bool)
        self.cam_K[view_id] = K
        self.images[view_id] = img
        self.all_time_num_views += 1
        if not self.no_prior_det:
            is_sym = np.array([bool(self.mesh_db[o]["is_symmetric"]) for o in obj_ids], dtype=bool)
        else:
            is_sym = np.zeros(len(obj_ids), dtype=bool)
        if cam_pose is not None:
            self.cam_poses[view_id] = cam_pose
            self.view_ids.append(view_id)
            is_sym = np.ones(len(obj_ids), dtype=bool)
        if self.give_all_prior:
            is_sym = np.ones(len(obj_ids), dtype=bool)
        if self.single_view_mode:
            is_sym = np.zeros(len(obj_ids), dtype=bool)
        is_non_sym = ~is_sym
        n_sym, n_non_sym = int(is_sym.sum()), int(is_non_sym.sum())
        if cam_pose is None and not self.single_view_mode and len(self.view_ids) > 0 and n_non_sym == 0:
            self._backup_estimate_camera_pose(view_id, obj_ids, bboxes)
        self.needs_opt = True
        bboxes[:, [0, 1]] *= 1.0 - self.bbox_inflate
        bboxes[:, [2, 3]] *= 1.0 + self.bbox_inflate
        # (debug_gt_kp replaces the network's keypoints by the ground truth, :1129-1131: that substitution lives on the host route)
        if (self.single_view_mode and self.device_chain and self.model is not None and not self.debug_gt_kp and cam_pose is None and len(self.view_ids) == 0
                and not self.cam_poses and not self.obj_poses and 0 < len(obj_ids) <= 16):
            self._process_view_single_device(view_id, img, K, obj_ids, bboxes, model_kps, model_kps_masks)
            torch.cuda.synchronize()
            tt1 = time()
            if self.all_time_num_views > 5:
                self.track_time_meter.update(tt1 - tt0)        # network + PnP + refinement: one chain, not separable from the host
            self.needs_opt = False
            return

        def sub(mask):
            return (obj_ids[mask], bboxes[mask], model_kps[mask], model_kps_masks[mask], kp_masks[mask],
                    uv_gt[mask] if uv_gt is not None else None)
        chained = False
        if self._slam_view_takes_the_vote_chain(view_id, cam_pose, n_non_sym, n_sym):
            chained = self._process_view_slam_chain(view_id, img, K, sub(is_non_sym), sub(is_sym))
        elif n_non_sym > 0:
            self._process_objects(False, view_id, img, K, *sub(is_non_sym))
        if view_id not in self.cam_poses:
            if len(self.view_ids) == 0:
                self.view_ids.append(view_id)
                self.cam_poses[view_id] = np.eye(4)[:3, :]
            else:
                self._backup_estimate_camera_pose(view_id, obj_ids, bboxes)
        if n_sym > 0 and not chained and ((view_id in self.cam_poses) or self.no_prior_det):
            self._process_objects(True, view_id, img, K, *sub(is_sym))
        if not self.single_view_mode:
            self._maybe_reinit_objects(view_id, len(self.view_ids) if self.sfm_mode else 15)
            self.optimize(curr_only=True)
        if self.model is not None:
            torch.cuda.synchronize()
        tt1 = time()
        if self.all_time_num_views > 5:            # warm-up views are not timed (:425)
            self.track_time_meter.update(tt1 - tt0)
        if self.sfm_mode or self.single_view_mode or (len(self.view_ids) > 1 and len(self.view_ids) % self.global_opt_every == 0):
            t0 = time()
            self.optimize()
            self.opt_time_meter.update(time() - t0)
            self.needs_opt = False

    def _cull_after_optimize(self, graph_objs, curr_only, view_curr):
        """object_slam.py:904-930: objects whose centre fell behind 0.5 diameter in the current view, then objects with too few inliers."""
        if not curr_only:
            for o in graph_objs:
                if view_curr in self.cam_poses:
                    p = self.cam_poses[view_curr][:3, :3] @ self.obj_poses[o][:3, 3] + self.cam_poses[view_curr][:3, 3]
                    if p[2] < 0.5 * self.mesh_db[o]["diameter"]:
                        self.remove_obj(o)
        n_inl = defaultdict(int)                                 # obj_num_inliers of every object in one pass over the detections
        for det in self.detections.values():
            for o, d in det.items():
                n_inl[o] += int(np.count_nonzero(d["inliers"]))
        for o in list(self.obj_poses.keys()):
            need = 3 if self.obj_num_dets[o] < 3 else 6
            if n_inl[o] < need:
                self.remove_obj(o)

    # ---------------------------------------------------------------------------------------------
    def _process_objects(self, is_sym, view_id, img, K, obj_ids, bboxes, model_kps, model_kps_masks, kp_masks, uv_gt=None):
        """object_slam.py:464-593."""
        if len(obj_ids) == 0:
            return
        prior_dets = prior_det_uv = None
        if is_sym and (not self.no_prior_det) and (view_id in self.cam_poses):
            prior_dets, prior_det_uv = {}, {}
            T_GtoC = to4x4(self.cam_poses[view_id])
            for k, obj_id in enumerate(obj_ids):
                if obj_id not in self.obj_poses:
                    continue
                m = model_kps_masks[k]
                T_OtoC = T_GtoC @ to4x4(self.obj_poses[obj_id])
                kps_in_C = model_kps[k][m] @ T_OtoC[:3, :3].T + T_OtoC[:3, 3]
                uvd = kps_in_C @ fix_K_for_bbox_ndc(K, bboxes[k]).T
                if np.all(uvd[:, 2] > 0):
                    full = np.zeros((m.shape[0], 2), dtype=np.float32)
                    full[m] = uvd[:, :2] / uvd[:, 2:3]
                    prior_det_uv[obj_id] = full
                    prior_dets[obj_id] = (full, m.astype(np.uint8))        # rendered on the device (pkpnet.PkpNet.forward)
        kp_det = self._run_kp_model(view_id, img, K, obj_ids, bboxes, model_kps, model_kps_masks, kp_masks, uv_gt, prior_dets)
        self._install_kp_detections(view_id, obj_ids, bboxes, model_kps_masks, kp_det, prior_det_uv)

    _VOTE_ON_HOST = object()

    def _install_kp_detections(self, view_id, obj_ids, bboxes, model_kps_masks, kp_det, prior_det_uv, cam_vote=_VOTE_ON_HOST):
        """Second half of __process_objects (object_slam.py:527-593): the detections of a pass into the state, the view's camera pose from the hypothesis vote when it
        has none yet, new objects into the map.  cam_vote: the vote's outcome when it was taken on the device (csrc/slam_vote.hip: the pose or None), else the host votes."""
        if not self.no_network_cov:
            for det in kp_det:
                if det["cov_pred"] is not None and det["cov_pred"].size > 0:
                    std = np.sqrt(det["cov_pred"][..., [0, 1], [0, 1]])
                    self.avg_std_meter.update(std.mean(), std.size)
        detection = {}
        for k, obj_id in enumerate(obj_ids):
            detection[obj_id] = {"bbox": bboxes[k], "model_kp_mask": model_kps_masks[k],
                                 "prior_uv": prior_det_uv.get(obj_id) if prior_det_uv is not None else None}
            detection[obj_id].update(kp_det[k])
            if self.num_views_processed() == 0:
                assert obj_id not in self.obj_poses, f"Object {obj_id} is in detections twice! obj_id must be an instance label."
                if detection[obj_id]["pose"] is not None:
                    T_OtoC = detection[obj_id]["pose"]
                    self.obj_poses[obj_id] = (invert_SE3(to4x4(self.cam_poses[view_id])) @ T_OtoC) if view_id in self.cam_poses else T_OtoC
        if view_id in self.detections:
            for obj_id in obj_ids:
                assert obj_id not in self.detections[view_id], "Object has already been processed for this view"
                self.detections[view_id][obj_id] = detection[obj_id]
        else:
            self.detections[view_id] = detection
        if view_id not in self.cam_poses:
            if self.num_views_processed() == 0:
                self.cam_poses[view_id] = np.eye(4)[:3, :]
            else:
                cam_pose = self._estimate_camera_pose(view_id) if cam_vote is self._VOTE_ON_HOST else cam_vote
                if cam_pose is None:
                    return
                self.cam_poses[view_id] = cam_pose
            self.view_ids.append(view_id)
        for obj_id in obj_ids:
            if obj_id not in self.obj_poses and detection[obj_id]["pose"] is not None:
                self.obj_poses[obj_id] = invert_SE3(to4x4(self.cam_poses[view_id])) @ detection[obj_id]["pose"]

    # ---------------------------------------------------------------------------------------------
    def _run_kp_model(self, view_id, img, K, obj_ids, bboxes, model_kps, model_kps_masks, kp_masks_gt=None, uv_gt=None, prior_dets=None):
        """object_slam.py:1077-1167.  Network + masks on the GPU, then ONE batched PnP launch for all
        objects of the frame (the reference loops lambdatwist.pnp per object)."""
        L = len(obj_ids)
        K_bbox = fix_K_for_bbox_ndc_many(K, bboxes).astype(np.float32)            # float32 container as in the reference (:1082)
        if self.device_chain and self.model is not None and (not self.debug_gt_kp or self.debug_gt_on_device):
            return self._run_kp_model_chain(img, K_bbox, obj_ids, bboxes, model_kps, model_kps_masks, kp_masks_gt, uv_gt, prior_dets)
        cov_uv = None
        if not self.debug_gt_kp or self.run_network_in_debug:
            import torch
            from .pkpnet import keypoint_masks
            prior_uv, prior_mask = prior_arrays(obj_ids, prior_dets) if prior_dets else (None, None)
            if self.no_network_cov:
                bt, vt = self.bbox_thresh, 1e30
            else:
                bt, vt = self.bbox_thresh, self.kp_var_thresh
            for _attempt in range(2):
                pred = self.model(self._frame_on_device(img), [torch.as_tensor(np.asarray(bboxes, np.float32))], None,
                                  prior_uv=prior_uv, prior_mask=prior_mask, check=False)
                masks_dev = keypoint_masks(pred["uv"], pred["cov"], pred["kp_mask"], model_kps_masks, bt, vt)
                # (three small read-backs, as the reference does, :1100-1111: packing them with torch.cat first costs more host time in
                #  torch's dispatcher -- 4 extra ops, +0.2 ms per call on the GPU boxes -- than the two stream waits it saves)
                exp_uv = pred["uv"].cpu().numpy()
                kp_masks = masks_dev.cpu().numpy().astype(bool)
                if not self.no_network_cov or self.run_network_in_debug:
                    cov_uv = pred["cov"].cpu().numpy()
                if not self.model.call_range_exceeded(pred.call):     # (fp16 form only: the read-backs above synchronised; on True the network is on bf16x3 now)
                    break
                self.fp16_range_reissues += 1
        if self.debug_gt_kp:
            assert kp_masks_gt is not None and uv_gt is not None
            kp_masks = np.asarray(kp_masks_gt, dtype=bool)
            cov_uv = None
        per_obj = []
        for k in range(L):
            m = kp_masks[k]
            if not self.debug_gt_kp:
                uv_pred = exp_uv[k][m].astype(np.float64)
            else:
                uv_pred = uv_gt[k][m].astype(np.float64)
                uv_pred = uv_pred + self._rng.normal(scale=0.01, size=uv_pred.shape)       # :1129-1131
            per_obj.append((uv_pred, cov_uv[k][m] if cov_uv is not None else None, model_kps[k][m].astype(np.float64),
                            K_bbox[k].astype(np.float64)))
        # batched PnP: objects with < 4 points are failures by definition (:31)
        idx = [k for k in range(L) if per_obj[k][0].shape[0] >= 4]
        poses = {}
        if idx:
            # normalize_uv per object (:34-36) with the L inverses taken in one stacked call (the same LAPACK routine per matrix)
            KinvT = np.linalg.inv(K_bbox.astype(np.float64)).transpose(0, 2, 1)
            T, status = _lt.pnp_batch([per_obj[k][2] for k in idx], [per_obj[k][0] @ KinvT[k][:2, :2] + KinvT[k][2:3, :2] for k in idx],
                                      0.001, seed=self._pnp_seed)
            self._pnp_seed += len(idx)
            for j, k in enumerate(idx):
                if not np.allclose(T[j], np.eye(4)):
                    poses[k] = T[j]
        ret = []
        for k, obj_id in enumerate(obj_ids):
            uv_pred, cov_pred, kp_model, K_kp = per_obj[k]
            inliers = np.ones(uv_pred.shape[0], dtype=bool)
            pose = None
            if k in poses and poses[k][2, 3] > 0.5 * self.mesh_db[obj_id]["diameter"] and inliers.sum() >= 4:      # :1147-1148
                pose = poses[k]
            self.obj_num_dets[obj_id] += 1
            self.obj_num_det_kps[obj_id] += uv_pred.shape[0]
            ret.append({"pose": pose, "inliers": inliers, "kp_mask": kp_masks[k], "model_kp": kp_model, "uv_gt": uv_gt,
                        "uv_pred": uv_pred, "cov_pred": cov_pred, "K": K_kp,
                        "score": 0.0 if inliers.size == 0 else float(inliers.astype(np.float32).mean())})
        return ret

    # ---------------------------------------------------------------------------------------------
    def _estimate_camera_pose(self, view_id, min_num_inliers=4):
        """object_slam.py:975-1072: hypotheses T_GtoC = T_OtoC(pnp) @ T_GtoO per object, scored by chi2 inliers."""
        curr = self.detections[view_id]
        obj_ids = [o for o in curr if curr[o].get("pose") is not None and o in self.obj_poses]
        self.last_cam_hypotheses = None
        if not obj_ids:
            return None
        hyps = [curr[i]["pose"] @ invert_SE3(to4x4(self.obj_poses[i])) for i in obj_ids]
        scored = [j for j in obj_ids if np.count_nonzero(curr[j]["inliers"]) > 0]
        counts = np.zeros(len(hyps), dtype=np.int64)
        if scored:
            T_obj = np.stack([to4x4(self.obj_poses[j]) for j in scored]).astype(np.float32).astype(np.float64)   # float32 container (:1004)
            # all |hypotheses| x |objects| scorings in one launch (csrc/slam_score.hip); the products as one stacked matmul (numpy runs the
            # same 4x4 kernel per pair as the reference's per-pair `@`)
            Ts = (np.stack(hyps)[:, None] @ T_obj[None]).reshape(-1, 4, 4)
            counts = _sc.chi2_counts(self, Ts, [curr[j] for _ in hyps for j in scored], True, self.manual_kp_std,
                                     CHI2_2DOF_95).reshape(len(hyps), len(scored)).sum(axis=1)
        best, best_n = None, -1
        for T_GtoC, n in zip(hyps, counts):
            if n >= min_num_inliers and n > best_n:
                best, best_n = T_GtoC, int(n)
        self.last_cam_hypotheses = {"obj_ids": obj_ids, "counts": [int(n) for n in counts], "best_num_inliers": best_n}
        return best

    def _maybe_reinit_objects(self, view_id, check_n_views=15):
        """object_slam.py:595-697: re-initialise an object from its current PnP pose when that explains
        >= 3 and more than 3x as many keypoints (over the last views) as the map pose."""
        if self.num_views_processed() < 2 or view_id not in self.cam_poses:
            return {}
        check_n_views = min(len(self.view_ids), check_n_views)
        curr = self.detections[view_id]
        obj_ids = [o for o in self.obj_poses if curr.get(o, {}).get("pose") is not None]
        if not obj_ids:
            return {}
        T_CtoG = invert_SE3(to4x4(self.cam_poses[view_id]))
        views = [self.view_ids[-(i + 1)] for i in range(check_n_views)]
        T_cam32 = np.stack([to4x4(self.cam_poses[v]) for v in views]).astype(np.float32)              # float32 containers (:619,:631)
        T_cam = T_cam32.astype(np.float64)
        T_pnp = {o: T_CtoG @ curr[o]["pose"] for o in obj_ids}
        T_pnp_all = np.stack([T_pnp[o] for o in obj_ids])
        T_est32 = np.stack([to4x4(self.obj_poses[o]) for o in obj_ids]).astype(np.float32)
        # every (object, recent view) pair under both poses in one launch (csrc/slam_score.hip); objects are independent of each other.
        # The reference's products keep numpy's promotion: float32 camera @ float64 PnP pose -> float64, but
        # float32 camera @ float32 map pose -> a float32 product (:634-637); as stacked matmuls (the same 4x4 kernel per pair)
        pairs = [(k, i) for k, o in enumerate(obj_ids) for i, v in enumerate(views) if o in self.detections[v]]
        dets = [self.detections[views[i]][obj_ids[k]] for k, i in pairs]
        owner = np.array([k for k, _ in pairs], dtype=np.int64)
        vi = np.array([i for _, i in pairs], dtype=np.int64)
        Ts = np.concatenate([T_cam[vi] @ T_pnp_all[owner], (T_cam32[vi] @ T_est32[owner]).astype(np.float64)])
        counts = _sc.chi2_counts(self, Ts, dets + dets, False, self.manual_kp_std, CHI2_2DOF_95)
        n_pnp = np.bincount(owner, weights=counts[:len(pairs)], minlength=len(obj_ids)).astype(np.int64)
        n_est = np.bincount(owner, weights=counts[len(pairs):], minlength=len(obj_ids)).astype(np.int64)
        report = {}
        for k, o in enumerate(obj_ids):
            reinit = bool(n_pnp[k] >= 3 and n_pnp[k] > 3 * n_est[k])
            report[o] = {"pnp": int(n_pnp[k]), "estim": int(n_est[k]), "reinit": reinit}
            if reinit:
                self.obj_poses[o] = T_pnp[o]
        return report                                  # (the reference returns nothing; the counts are for tests / logging)

    def _backup_estimate_camera_pose(self, view_id, obj_ids_, bboxes):
        """object_slam.py:933-973: bbox-centroid PnP, else constant velocity, else copy the last pose."""
        assert len(self.view_ids) > 0 and view_id not in self.view_ids and view_id not in self.cam_poses
        cents, centers = [], []
        for i, o in enumerate(obj_ids_):
            if o in self.obj_poses:
                cents.append(0.5 * (bboxes[i, :2] + bboxes[i, 2:]))
                centers.append(self.obj_poses[o][:3, 3])
        ret = pnp(np.stack(centers), np.stack(cents), self.cam_K[view_id]) if cents else None
        if ret is not None:
            self.cam_poses[view_id] = ret[0]
        elif len(self.view_ids) > 1:
            T1, T2 = to4x4(self.cam_poses[self.view_ids[-2]]), to4x4(self.cam_poses[self.view_ids[-1]])
            self.cam_poses[view_id] = (T2 @ invert_SE3(T1)) @ T2
        else:
            self.cam_poses[view_id] = self.cam_poses[self.view_ids[-1]]
        self.view_ids.append(view_id)

    # ---------------------------------------------------------------------------------------------
    def build_problem(self, curr_only=False, view=None, exclude_views=()):
        """Graph construction of optimize() (object_slam.py:713-839) as a flat SoA for suo_optimize.
        Returns (problem, bookkeeping) or None when the reference would return early.
        view: the view whose curr_only graph is built (default: the last one).  exclude_views: views whose cameras and detections the global graph leaves out
        (map_covariance); the gauge is then the first camera that remains.  The defaults give the graphs optimize() runs."""
        if len(self.view_ids) == 0:
            return None
        num_cam_edges, num_obj_edges = defaultdict(int), defaultdict(int)
        obj_ids = list(self.obj_poses.keys())
        view_curr = self.view_ids[-1] if view is None else view
        if curr_only:
            if view_curr not in self.cam_poses or view_curr not in self.detections:
                return None
            dets = {view_curr: self.detections[view_curr]}
        elif exclude_views:
            dets = {v: d for v, d in self.detections.items() if v not in exclude_views}
        else:
            dets = self.detections
        for v, det in dets.items():
            if v in self.cam_poses:
                for o, d in det.items():
                    if o in obj_ids:
                        n = int(np.count_nonzero(d["inliers"]))
                        num_cam_edges[v] += n
                        num_obj_edges[o] += n
        if curr_only and num_cam_edges[view_curr] < 3:
            return None
        obj_index = {o: j for j, o in enumerate(o for o in obj_ids if num_obj_edges[o] > 0)}
        cam_views = [view_curr] if curr_only else [v for v in self.cam_poses.keys() if v not in exclude_views]
        cam_index, cam_fixed = {}, []
        for i, v in enumerate(cam_views):
            if num_cam_edges[v] > 0:
                cam_index[v] = len(cam_index)
                cam_fixed.append(0 if curr_only else int(i == 0))          # gauge: enumeration index 0 only (:774, R11)
        if not cam_index or not obj_index:
            return None
        # one segment of edges per detection, in the reference's enumeration order (views, objects, keypoints); the
        # per-keypoint data comes from the detection's cache instead of a Python loop over keypoints
        segs, seg_cam, seg_obj, seg_n, e_k, e_p, e_uv, e_info, e_inl = [], [], [], [], [], [], [], [], []
        E = 0
        for v, det in dets.items():
            if v not in cam_index:
                continue
            for o, d in det.items():
                if o in obj_index:
                    c = _det_edges(d)
                    n = c["n"]
                    segs.append((v, o, E, n))
                    seg_cam.append(cam_index[v]); seg_obj.append(obj_index[o]); seg_n.append(n)
                    e_k.append(c["camk"]); e_p.append(c["pts"][:n]); e_uv.append(c["uv"][:n]); e_info.append(c["info"])
                    e_inl.append(np.asarray(d["inliers"], dtype=np.uint8))
                    E += n
        seg_n = np.array(seg_n, dtype=np.int64)
        if self.sfm_mode or (self.slam_mode and not curr_only):
            its = (10, 10, 40, 40)
        else:
            its = (10, 10, 10, 10)
        prob = _ba.Problem(np.stack([to4x4(self.cam_poses[v])[:3] for v in cam_index]), np.array(cam_fixed, np.uint8),
                           np.stack([to4x4(self.obj_poses[o])[:3] for o in obj_index]),
                           np.full(len(obj_index), 1 if curr_only else 0, np.uint8),
                           np.repeat(np.array(seg_cam, np.int32), seg_n), np.repeat(np.array(seg_obj, np.int32), seg_n),
                           np.repeat(np.array(e_k, np.float64).reshape(-1, 4), seg_n, axis=0),
                           np.concatenate(e_p).reshape(E, 3), np.concatenate(e_uv).reshape(E, 2),
                           np.concatenate(e_info).reshape(E, 3), np.concatenate(e_inl), its=its,
                           init_with_outliers=bool(self.opt_init_with_outliers and curr_only))
        return prob, (cam_index, obj_index, _EdgeRefs(segs, E), curr_only, view_curr)

    def apply_problem(self, prob, book):
        """Read-back + culling of optimize() (object_slam.py:898-930)."""
        cam_index, obj_index, e_ref, curr_only, view_curr = book
        inl = np.asarray(prob.inlier).astype(bool)
        for v, o, first, n in e_ref.segs:
            self.detections[v][o]["inliers"][:] = inl[first:first + n]
        cam_T = prob.cam_T.reshape(-1, 3, 4)
        obj_T = prob.obj_T.reshape(-1, 3, 4)
        for v, i in cam_index.items():
            self.cam_poses[v] = cam_T[i].copy()
        if not curr_only:
            for o, j in obj_index.items():
                self.obj_poses[o] = obj_T[j].copy()
        self._cull_after_optimize(list(obj_index.keys()), curr_only, view_curr)

    @_on_stream
    def pose_covariances(self, view_ids=None, relative=False, trajectory=False, scaled=False):
        """6x6 marginal covariances of the current map: {"cams": {view_id: 6x6}, "objs": {obj_id: 6x6}} for every key of cam_poses (or those in view_ids) and
        obj_poses, from the global graph of build_problem() at the stored poses and inlier flags (ba.pose_covariances: rows / columns [omega, upsilon] of the
        left update; zeros for the gauge camera, NaNs for a vertex no counted measurement reaches).  These blocks are relative to the gauge camera.
        relative=True adds "rel": {(view_id, obj_id): 6x6} for every selected view and every object of the map: the covariance of the T_OtoC = T_GtoC T_OtoG that
        collect_results reports, which does not depend on the gauge.  trajectory=True adds "rel_cams": {(view_a, view_b): 6x6} for consecutive selected views in
        cam_poses order: the covariance of T_b T_a^-1, the motion between the two views (NaN where a view is not in the graph).  One device call
        (ba.pose_covariances_graph: any number of objects up to its cap; the bits of ba.pose_covariances / ba.pose_covariances_pairs wherever those answer).
        scaled=True multiplies every returned block by the chi2 scale s0^2 of the same graph (residual_statistics()["summary"]["s0_sq"]) and adds
        "variance_factor": NaN, and with it every block, when the graph has no redundancy (dof <= 0) or does not build.  Without it the blocks are the
        covariance under the stated information matrices.  Changes nothing in the map."""
        nan = np.full((6, 6), np.nan)
        cams = {v: nan.copy() for v in self.cam_poses if view_ids is None or v in view_ids}
        objs = {o: nan.copy() for o in self.obj_poses}
        built = self.build_problem(False)
        if built is not None:
            prob, (cam_index, obj_index, _, _, _) = built
            keys = [(v, o) for v in cams if v in cam_index for o in obj_index] if relative else []
            pairs = [(cam_index[v], len(cam_index) + obj_index[o]) for v, o in keys]
            views = list(cams)
            steps = [(a, b) for a, b in zip(views[:-1], views[1:]) if a in cam_index and b in cam_index] if trajectory else []
            pairs += [(cam_index[a], cam_index[b]) for a, b in steps]
            cam_cov, obj_cov, _, rel_cov, _ = _ba.pose_covariances_graph_batch([prob], [np.array(pairs, np.int32).reshape(-1, 2)])[0]
            for v, i in cam_index.items():
                if v in cams:
                    cams[v] = cam_cov[i].copy()
            for o, j in obj_index.items():
                objs[o] = obj_cov[j].copy()
        out = {"cams": cams, "objs": objs}
        if relative:
            out["rel"] = {(v, o): nan.copy() for v in cams for o in objs}
            if built is not None:
                for k, S6 in zip(keys, rel_cov):
                    out["rel"][k] = S6.copy()
        if trajectory:
            views = list(cams)
            out["rel_cams"] = {k: nan.copy() for k in zip(views[:-1], views[1:])}
            if built is not None:
                for k, S6 in zip(steps, rel_cov[len(keys):]):
                    out["rel_cams"][k] = S6.copy()
        if scaled:
            s0_sq = float(_ba.residual_statistics_batch([prob])[0]["summary"][5]) if built is not None else float("nan")
            for blocks in out.values():
                for k in blocks:
                    blocks[k] = blocks[k] * s0_sq
            out["variance_factor"] = s0_sq
        return out

    @_on_stream
    def map_covariance(self, exclude_views=()):
        """(obj_ids, Sigma_OO): the joint covariance [6 n, 6 n] of every object of obj_poses, in that order, from the global graph of build_problem() without the
        cameras and detections of exclude_views, at the stored poses and inlier flags -- the objects' blocks and every (object, object) cross block of
        ba.pose_covariances_graph, assembled dense (rows / columns [omega, upsilon] of the left update, relative to the gauge camera).  The rows and columns of an
        object that graph does not reach are NaN: tracking_covariance() treats it as not in the map.  Changes nothing in the map."""
        obj_ids = list(self.obj_poses.keys())
        Sigma = np.full((6 * len(obj_ids), 6 * len(obj_ids)), np.nan)
        built = self.build_problem(False, exclude_views=tuple(exclude_views))
        if built is not None:
            prob, (cam_index, obj_index, _, _, _) = built
            nc, objs = len(cam_index), list(obj_index)
            pairs = [(nc + obj_index[a], nc + obj_index[b]) for i, a in enumerate(objs) for b in objs[i + 1:]]
            _, obj_cov, cross, _, _ = _ba.pose_covariances_graph_batch([prob], [np.array(pairs, np.int32).reshape(-1, 2)])[0]
            at = {o: 6 * i for i, o in enumerate(obj_ids)}
            for o, j in obj_index.items():
                Sigma[at[o]:at[o] + 6, at[o]:at[o] + 6] = obj_cov[j]
            for (ja, jb), X in zip(pairs, cross):
                a, b = at[objs[ja - nc]], at[objs[jb - nc]]
                Sigma[a:a + 6, b:b + 6] = X
                Sigma[b:b + 6, a:a + 6] = X.T
        return obj_ids, Sigma

    @_on_stream
    def tracking_covariance(self, view_id=None, map_cov=None):
        """The covariance of a tracked camera with the map's uncertainty carried in (ba.tracking_covariances; include/suo_hip.h: suo_tracking_covariances), from the
        curr_only graph of view_id (default: the last view) at the stored poses and inlier flags:
          "cam"            6x6, Hcc^-1 + G Sigma_OO G^T: the covariance of the camera as the tracker estimates it, against objects it holds at their map poses
          "cam_fixed_map"  6x6, Hcc^-1: what pose tracking against a perfectly known map would give (ba.pose_covariances of the same graph)
          "cross"          {obj_id: 6x6} Sigma_co, rows the camera; "rel" {obj_id: 6x6} the covariance of T_OtoC = T_GtoC T_OtoG, for every object of that graph
          "status"         [NaN cameras, objects of the graph that are not in the map]
        map_cov is the pair map_covariance() returns.  ASSUMPTION: it must not contain this view's measurements -- the formula takes the map's errors and the view's
        keypoint noise as independent.  None computes map_covariance(exclude_views=(view_id,)), which rebuilds the global graph; the intended use is to call
        map_covariance() once after a global adjustment and to pass it for the views that follow until the next one.  An object the map covariance does not hold
        (NaN block, or missing from its obj_ids: e.g. first initialised from this very view) is left out: its keypoints are not counted and its blocks are NaN.
        Every block is NaN when the view has no curr_only graph.  Changes nothing in the map."""
        view = self.view_ids[-1] if view_id is None and self.view_ids else view_id
        nan = np.full((6, 6), np.nan)
        out = {"cam": nan.copy(), "cam_fixed_map": nan.copy(), "cross": {}, "rel": {}, "status": [1, 0]}
        built = self.build_problem(True, view=view) if self.view_ids else None
        if built is None:
            return out
        prob, (_, obj_index, _, _, _) = built
        obj_ids, Sigma = self.map_covariance(exclude_views=(view,)) if map_cov is None else map_cov
        objs = list(obj_index)
        sub = np.full((6 * len(objs), 6 * len(objs)), np.nan)
        rows = {o: 6 * i for i, o in enumerate(obj_ids)}
        have = [j for j, o in enumerate(objs) if o in rows]
        if have:
            src = np.concatenate([np.arange(rows[objs[j]], rows[objs[j]] + 6) for j in have])
            dst = np.concatenate([np.arange(6 * j, 6 * j + 6) for j in have])
            sub[np.ix_(dst, dst)] = np.asarray(Sigma)[np.ix_(src, src)]
        r = _ba.tracking_covariances_batch([prob], [sub])[0]
        out["cam"], out["cam_fixed_map"] = r["cam_cov"][0].copy(), r["fixed_map_cov"][0].copy()
        out["cross"] = {o: r["cross"][0, j].copy() for o, j in obj_index.items()}
        out["rel"] = {o: r["rel"][0, j].copy() for o, j in obj_index.items()}
        out["status"] = [int(x) for x in r["status"]]
        return out

    @_on_stream
    def residual_statistics(self, view_ids=None):
        """How well the measurements of the current map agree with its poses, from the global graph of build_problem() at the stored poses and inlier flags
        (ba.residual_statistics; include/suo_hip.h: suo_residual_statistics):
          "summary"  {"m": counted keypoints, "n": rows of the Hessian, "chi2": their sum of v^T Omega v, "leverage": their sum of leverages (= n), "dof": 2 m - n,
                      "s0_sq": chi2 / dof, the factor pose_covariances(scaled=True) applies; NaN without redundancy, "status": the entry's four counts}
          "cams"     {view_id: (count, chi2, redundancy)} over the view's counted keypoints, for every key of cam_poses (or those in view_ids); "objs" {obj_id: ...}
                     likewise for every key of obj_poses.  chi2 / redundancy is the vertex's variance component; (0, 0.0, 0.0) for a vertex outside the graph.
          "edges"    {(view_id, obj_id): {"chi2", "leverage", "t"}}, one array entry per keypoint of the detection in its stored order (apply_problem's book-keeping):
                     t is the studentised statistic, chi2(2) under the model whether the keypoint is counted or not; NaN where it cannot be checked.
        Changes nothing in the map."""
        cams = {v: (0, 0.0, 0.0) for v in self.cam_poses if view_ids is None or v in view_ids}
        objs = {o: (0, 0.0, 0.0) for o in self.obj_poses}
        nan = float("nan")
        summary = {"m": 0, "n": 0, "chi2": 0.0, "leverage": 0.0, "dof": 0, "s0_sq": nan, "status": [0, 0, 0, 0]}
        edges = {}
        built = self.build_problem(False)
        if built is not None:
            prob, (cam_index, obj_index, e_ref, _, _) = built
            r = _ba.residual_statistics_batch([prob])[0]
            s = r["summary"]
            summary = {"m": int(s[0]), "n": int(s[1]), "chi2": float(s[2]), "leverage": float(s[3]), "dof": int(s[4]), "s0_sq": float(s[5]),
                       "status": [int(x) for x in r["status"]]}
            triple = lambda row: (int(row[0]), float(row[1]), float(row[2]))
            for v, i in cam_index.items():
                if v in cams:
                    cams[v] = triple(r["cam_stat"][i])
            for o, j in obj_index.items():
                objs[o] = triple(r["obj_stat"][j])
            for v, o, first, n in e_ref.segs:
                if v in cams:
                    edges[(v, o)] = {"chi2": r["edge_chi2"][first:first + n].copy(), "leverage": r["edge_lev"][first:first + n].copy(),
                                     "t": r["edge_t"][first:first + n].copy()}
        return {"summary": summary, "cams": cams, "objs": objs, "edges": edges}

    @_on_stream
    def optimize(self, curr_only=False):
        """object_slam.py:703-930 with the g2o graph replaced by one suo_optimize call."""
        built = self.build_problem(curr_only)
        if built is None:
            return
        prob, book = built
        _ba.optimize_batch([prob])
        self.apply_problem(prob, book)
