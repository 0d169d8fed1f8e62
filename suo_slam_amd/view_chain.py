"""The device routes of ``ObjectSLAM``: every way a view's keypoints reach the PnP poses WITHOUT leaving the device between the network and the geometry
chain (suo_slam_amd/frame_geom.py, csrc/frame_geom.hip), where the host route (object_slam.py: _run_kp_model) restates the reference's data flow.

    ChainPass        one network pass of a SLAM view: ``prepare`` (the constructor: pure numpy, no GPU, no torch) decides what goes to the device and where
                     it lies in the staged block; ``stage`` / ``launch`` (= ``enqueue``) put it on the current stream and never wait
    vote_block       the host block of csrc/slam_vote.hip for the two passes of a tracking view
    DeviceRoutes     base class of ObjectSLAM: the single-view chain (one frame, or batches in flight), a SLAM pass on the chain (_run_kp_model_chain) and
                     both passes of a tracking view as one chain (_process_view_slam_chain); the device state an ObjectSLAM owns is declared in its __init__

The rules (thresholds, acceptance, removal, re-initialisation), the map state and the host route stay in object_slam.py.  There is no CPU fallback.
"""
from __future__ import annotations

import functools
import os
from time import time

import numpy as np

from .frame_geom import kbbox_terms
from .geometry import fix_K_for_bbox_ndc, fix_K_for_bbox_ndc_many
from .weights import NUM_KP

CHI2_2DOF_95 = 5.991
# the vote's host block (include/suo_hip.h: SUO_SLAM_VOTE_BLOCK doubles): a_in_map [16] | a_T [16][12] | a_K [16][9] | b_in_map [16] | b_T [16][12] | b_K [16][9]
_A_IN, _A_T, _A_K, _B_IN, _B_T, _B_K, SUO_SLAM_VOTE_BLOCK = 0, 16, 208, 352, 368, 560, 704


def _on_stream(fn):
    """Run a method's device work on the object's own (non-NULL) stream.  torch's default stream is the legacy NULL stream, on which libsuo_hip's network
    entries BLOCK (include/suo_hip.h: "NULL = internal stream + blocking"): measured 13.3 ms of host time per 128-crop call that an asynchronous call returns
    from in 0.3 ms.  Everything a method enqueues -- uploads, network, masks, geometry chain, read-backs -- goes to the one stream, so it stays ordered."""
    @functools.wraps(fn)
    def wrapped(self, *a, **kw):
        st = getattr(self, "_gpu_stream", None)
        if st is None:
            return fn(self, *a, **kw)
        import torch
        with torch.cuda.stream(st):
            return fn(self, *a, **kw)
    return wrapped


def vote_block(K, ids_a, K_bbox_a, ids_b, bboxes_b, obj_poses):
    """The vote's host block: map flags and poses of both passes' objects, pass A's intrinsics in their float32 container (what its detections carry, :1082),
    pass B's as the double fix_K_for_bbox_ndc (as the reference projects the priors with it, :505)."""
    blk = np.zeros(SUO_SLAM_VOTE_BLOCK)
    for ids, in_map, T, Kk, Ks in ((ids_a, _A_IN, _A_T, _A_K, [Kb.astype(np.float64) for Kb in K_bbox_a]),
                                   (ids_b, _B_IN, _B_T, _B_K, [fix_K_for_bbox_ndc(K, bb) for bb in bboxes_b])):
        for k, o in enumerate(ids):
            if o in obj_poses:
                blk[in_map + k] = 1.0
                blk[T + 12 * k:T + 12 * k + 12] = np.asarray(obj_poses[o], dtype=np.float64)[:3, :4].reshape(-1)
            blk[Kk + 9 * k:Kk + 9 * k + 9] = Ks[k].reshape(-1)
    return blk


def prior_arrays(obj_ids, prior_dets):
    """prior_dets = {obj_id: (uv [41,2], mask [41])} as the network's inputs: prior_uv float32 [L,41,2] NDC, prior_mask uint8 [L,41] (zeros where an object has
    none).  The reference stamps the heat-maps on the host (make_prior_kp_input) and uploads [L,41,256,256]; here the projected keypoints go to the device and
    the stamps are rendered while the crop is staged."""
    prior_uv = np.zeros((len(obj_ids), NUM_KP, 2), dtype=np.float32)
    prior_mask = np.zeros((len(obj_ids), NUM_KP), dtype=np.uint8)
    for k, obj_id in enumerate(obj_ids):
        if obj_id in prior_dets:
            prior_uv[k], prior_mask[k] = prior_dets[obj_id]
    return prior_uv, prior_mask


class ChainPass:
    """One network pass of a SLAM view whose keypoints stay on the device: network -> masks (or the ground-truth substitution) -> compaction -> PnP ->
    acceptance (FrameGeometry.launch with do_lm = False).

    The constructor is the PREPARE half, pure numpy: the per-crop host inputs of the chain (K_bbox, kinv, camk, min_depth, vt), the noise draws of the
    ground-truth keypoints, and ``host_arrays`` -- every small host array of the pass, which go to the device in ONE pinned block and ONE stream-ordered copy
    kernel, enqueued BEFORE the network: a pageable .to(device) per array blocks the host until it has run -- in front of the network that is tens of
    microseconds each on the critical path, behind it a wait for the network.  ``pos`` says which position of the list holds what; nobody else has to know.

    objs = (obj_ids, bboxes, model_kps, model_kps_masks, kp_masks_gt, uv_gt).  K_bbox: the float32 container when the caller has it already.
    prior_dets: {obj_id: (uv [41,2], mask [41])}, the projected keypoints the network renders its prior heat-maps from.  block: the vote's host block."""

    def __init__(self, K, objs, mesh_db, rng, no_network_cov, debug_gt_kp, bbox_thresh, kp_var_thresh, K_bbox=None, prior_dets=None, block=None):
        obj_ids, bboxes, model_kps, model_kps_masks, kp_masks_gt, uv_gt = objs
        self.L = L = len(obj_ids)
        self.K_bbox = fix_K_for_bbox_ndc_many(K, bboxes).astype(np.float32) if K_bbox is None else K_bbox      # float32 container (:1082)
        self.kinv, self.camk = kbbox_terms(self.K_bbox)
        self.min_depth = np.array([0.5 * mesh_db[o]["diameter"] for o in obj_ids], dtype=np.float64)
        self.use_cov, self.bbox_thresh, self.vt = not no_network_cov, bbox_thresh, 1e30 if no_network_cov else kp_var_thresh
        named = [("kps", np.ascontiguousarray(model_kps, dtype=np.float32)), ("boxes", np.ascontiguousarray(bboxes, dtype=np.float32)),
                 ("class_mask", np.ascontiguousarray(model_kps_masks, dtype=np.uint8))]
        if block is not None:
            named.append(("block", block))
        if debug_gt_kp:                                       # (debug_gt_on_device: the same draws, in the same order, as the host route's :1129-1131)
            gt_mask = np.ascontiguousarray(kp_masks_gt, dtype=np.uint8)
            gt_uv = np.zeros((L, NUM_KP, 2), dtype=np.float32)
            for k in range(L):
                m = gt_mask[k].astype(bool)
                u = uv_gt[k][m].astype(np.float64)
                gt_uv[k][m] = (u + rng.normal(scale=0.01, size=u.shape)).astype(np.float32)
            named += [("gt_mask", gt_mask), ("gt_uv", gt_uv)]
        if prior_dets:
            named += zip(("prior_uv", "prior_mask"), prior_arrays(obj_ids, prior_dets))
        self.pos = {name: i for i, (name, _) in enumerate(named)}
        self.host_arrays = [a for _, a in named]

    def stage(self, model):
        """The pass's host arrays on the device (one stage_block call), by name."""
        st = model.stage_block(self.host_arrays)
        dev = {name: st[i] for name, i in self.pos.items()}
        self.kps_dev, self.boxes_dev, self.class_mask_dev, self.block_dev = dev["kps"], dev["boxes"], dev["class_mask"], dev.get("block")
        self._gt_dev = (dev["gt_uv"], dev["gt_mask"]) if "gt_uv" in dev else None
        self._prior_dev = (dev.get("prior_uv"), dev.get("prior_mask"))

    def launch(self, model, fg, frame, seed, seed_dev=None, prior_uv=None, prior_mask=None, out_slot=None):
        """Network + masks + PnP chain of the staged pass on the current stream.  prior_uv / prior_mask: device tensors that replace the pass's own priors."""
        from .pkpnet import keypoint_masks
        if prior_uv is None:
            prior_uv, prior_mask = self._prior_dev
        self.pred = pred = model(frame, [self.boxes_dev], None, prior_uv=prior_uv, prior_mask=prior_mask, check=False, out_slot=out_slot)
        if self._gt_dev is not None:                          # the ground truth overwrites the network's keypoints where they lie, in float32: the type it emits
            self.uv_dev, self.masks_dev = self._gt_dev
        else:
            self.uv_dev, self.masks_dev = pred["uv"], keypoint_masks(pred["uv"], pred["cov"], pred["kp_mask"], self.class_mask_dev, self.bbox_thresh, self.vt)
        fg.launch([0, self.L], self.uv_dev, pred["cov"], self.masks_dev, self.kps_dev, self.kinv, self.camk, self.min_depth, seed=seed, seed_dev=seed_dev,
                  use_cov=self.use_cov, do_lm=False)

    def enqueue(self, model, fg, frame, seed, **kw):
        self.stage(model)
        self.launch(model, fg, frame, seed, **kw)


def _geometry(fg, L):
    """The one-frame geometry context fg, or a new one when there is none yet or it is too small for L crops."""
    from .frame_geom import FrameGeometry
    return fg if fg is not None and fg.max_crops >= L else FrameGeometry(max(16, L), 1)


class DeviceRoutes:
    """The device routes of ObjectSLAM and the device state they keep between views.  Reads the flags, the map state and the rules of the ObjectSLAM it is
    the base of (object_slam.py)."""

    def __init__(self):
        self._gpu_stream = None       # the stream all device work of this object runs on (_on_stream); made with the network
        # geometry contexts (FrameGeometry: one launch in flight each), created at first use and regrown when a frame has more crops
        self._fg = None               # single-view frames, a SLAM pass, pass A of a tracking view
        self._fg2 = None              # pass B of a tracking view: enqueued while pass A's block is still to be read
        self._fg_ring = {"ctx": [None, None], "next": 0}      # batches of single views: two in flight
        # the PnP sampler's running key on the device (batches in flight continue from each other's counts without a read-back): the launch samples with
        # _seed_base + _seed_run[0]; _seed_expect is what the collected batches added to it, so _seed_base + _seed_expect == _pnp_seed unless another route ran
        self._seed_run = None
        self._seed_base = 0
        self._seed_expect = 0
        # batches of submit_views_single in flight, oldest first, and when the last one was collected
        self._tickets = []
        self._last_collect = 0.0
        # pinned read-back buffers of the vote (its 32 doubles, the priors it projected, an event), made with the first tracking view
        self._vote_pin = None
        # the frame of the current view on the device (_frame_on_device): uploaded once per view
        self._frame_key = self._frame_dev = None

    def _chain_pass(self, K, objs, **kw):
        return ChainPass(K, objs, self.mesh_db, self._rng, self.no_network_cov, self.debug_gt_kp, self.bbox_thresh, self.kp_var_thresh, **kw)

    # ---- single-view frames ---------------------------------------------------------------------
    def _launch_single_views(self, fg, frame_first, pred, class_mask, model_kps, K_bbox, obj_ids, **seed):
        """What follows the network on a single-view frame (or a batch of them): keypoint masks, then PnP -> acceptance -> graph -> LM as one chain.
        model_kps: float32, on the host (uploaded here, behind the masks) or on the device already."""
        import torch
        from .pkpnet import keypoint_masks
        kinv, camk = kbbox_terms(K_bbox)
        min_depth = np.array([0.5 * self.mesh_db[o]["diameter"] for o in obj_ids], dtype=np.float64)
        vt = 1e30 if self.no_network_cov else self.kp_var_thresh
        its = (10, 10, 40, 40) if self.sfm_mode else (10, 10, 10, 10)                                    # (:843-846)
        masks_dev = keypoint_masks(pred["uv"], pred["cov"], pred["kp_mask"], class_mask, self.bbox_thresh, vt)
        kps_dev = torch.as_tensor(model_kps).to(pred["uv"].device)
        fg.launch(frame_first, pred["uv"], pred["cov"], masks_dev, kps_dev, kinv, camk, min_depth, use_cov=not self.no_network_cov, do_lm=True, its=its, **seed)

    def _process_view_single_device(self, view_id, img, K, obj_ids, bboxes, model_kps, model_kps_masks):
        """A single-view frame (evaluate.py --nviews 1: __process_objects(False, ...) :464-593, __run_kp_model :1077-1167, then
        optimize() :703-930 with the camera fixed at identity) with everything between the network and the poses on the device
        (csrc/frame_geom.hip): one launch chain, one read-back.  Leaves the same state behind as the host route."""
        import torch
        L = len(obj_ids)
        K_bbox = fix_K_for_bbox_ndc_many(K, bboxes).astype(np.float32)                                   # float32 container (:1082)
        fg = self._fg = _geometry(self._fg, L)
        for _attempt in range(2):
            pred = self.model(np.ascontiguousarray(img), [torch.as_tensor(np.asarray(bboxes, np.float32))], None, check=False)
            self._launch_single_views(fg, [0, L], pred, model_kps_masks, np.ascontiguousarray(model_kps, dtype=np.float32), K_bbox, obj_ids, seed=self._pnp_seed)
            r = fg.fetch(copy=True)
            if not self.model.call_range_exceeded(pred.call):  # (fp16 form only: an activation of this call left its range -> the network is on bf16x3 now, once more)
                break
            self.fp16_range_reissues += 1
        self._pnp_seed += int(np.count_nonzero(r["n_kp"] >= 4))
        self._ingest_single_view(view_id, obj_ids, bboxes, model_kps, model_kps_masks, K_bbox, r, 0, 0)

    def _ingest_single_view(self, view_id, obj_ids, bboxes, model_kps, model_kps_masks, K_bbox, r, lo, frame):
        """State of a single-view frame from the device chain's read-back (crops [lo, lo + L) of launch result r, frame index `frame`)."""
        kp_det = self._kp_det_from_chain(r, obj_ids, model_kps, K_bbox, None, lo=lo, lm_inliers=True)
        detection = {}
        for k, obj_id in enumerate(obj_ids):
            det = kp_det[k]
            if det["cov_pred"] is not None and det["cov_pred"].size > 0:
                std = np.sqrt(det["cov_pred"][..., [0, 1], [0, 1]])
                self.avg_std_meter.update(std.mean(), std.size)
            assert obj_id not in self.obj_poses and obj_id not in detection, f"Object {obj_id} is in detections twice! obj_id must be an instance label."
            detection[obj_id] = {"bbox": bboxes[k], "model_kp_mask": model_kps_masks[k], "prior_uv": None, **det}
            if det["pose"] is not None:
                self.obj_poses[obj_id] = r["T_opt"][lo + k].copy()
        self.detections[view_id] = detection
        self.cam_poses[view_id] = np.eye(4)[:3, :]
        self.view_ids.append(view_id)
        self.last_lm_stats = r["lm_stats"][frame].copy()
        t0 = time()
        self._cull_after_optimize([o for k, o in enumerate(obj_ids) if r["accepted"][lo + k]], False, view_id)
        self.opt_time_meter.update(time() - t0)

    def single_views_take_the_device_chain(self, views):
        """True when process_views_single can run `views` as ONE device call (else it processes them one by one)."""
        if not (self.single_view_mode and self.device_chain and self.model is not None and not self.debug_gt_kp and len(views) > 1):
            return False
        shape = np.asarray(views[0][1]).shape
        if sum(len(v[3]) for v in views) > self.model.max_crops:      # more crops than the network was built for: view by view (ObjectSLAM(max_crops=...) lifts it)
            return False
        return all(0 < len(v[3]) <= 16 and np.asarray(v[1]).shape == shape and np.asarray(v[1]).dtype == np.uint8 for v in views)

    @_on_stream
    def process_views_single(self, views):
        """Single-view evaluation (evaluate.py --nviews 1: reset / process_view / collect_results per reference view, evaluate.py:338-395) of SEVERAL
        independent views in one device call: `views` = [(view_id, img, K, obj_ids, bboxes, model_kps, model_kps_masks, kp_masks), ...].
        Returns [collect_results() of view 0, of view 1, ...] -- what the per-view loop returns: everything downstream of the network is bit for bit
        the per-view loop's on the same network outputs (one geometry launch; the PnP sampler's keys continue from frame to frame as the per-view
        loop advances its seed, csrc/pnp.hip); the shared network call picks its kernels by launch size, so its keypoints agree with the
        per-view calls' to the network's tolerance (1e-5 of the reference either way).  tests/test_gpu_evaluator.py holds both.
        = submit_views_single + collect_views_single; a caller with more batches to come submits the next one BEFORE collecting this one
        (Evaluator.run does), so that the host's share of a batch -- bookkeeping of the results, preparation of the next -- runs under the device's.
        Refuses to run with batches of an earlier submit_views_single still in flight: collect_views_single hands back the OLDEST batch, which would be zipped
        against these views."""
        if self.views_in_flight():
            raise RuntimeError("process_views_single: %d batch(es) submitted earlier are still in flight -- collect_views_single() / drain_views_single() them first"
                               % self.views_in_flight())
        if not self.single_views_take_the_device_chain(views):
            self.drain_views_single()
            out = []
            for v in views:
                self.reset()
                self.process_view(*v[:8])
                out.append(self.collect_results(no_viz=True))
            return out
        self.submit_views_single(views)
        return self.collect_views_single()

    def views_in_flight(self):
        return len(self._tickets)

    @_on_stream
    def drain_views_single(self):
        """Collect (and drop) whatever submit_views_single left in flight."""
        while self.views_in_flight():
            self.collect_views_single()

    def _enqueue_views(self, prep, ff, t0):
        """Network + masks + geometry chain of one prepared batch (submitted at t0) on the current stream, and its ticket; nothing here waits for the device."""
        import torch
        from .frame_geom import FrameGeometry
        Ltot, B = ff[-1], len(prep)
        ring = self._fg_ring
        k = ring["next"]
        ring["next"] = (k + 1) % 2
        fg = ring["ctx"][k]
        if fg is None or fg.max_crops < Ltot or fg.max_frames < B:
            fg = ring["ctx"][k] = FrameGeometry(max(256, Ltot), max(32, B))
        if self._seed_run is None:
            self._seed_run = torch.zeros(1, dtype=torch.int64, device=self.model.device)      # the sampler's running key, device-resident
            self._seed_base = self._pnp_seed
        mm_all = np.concatenate([p[6] for p in prep]).astype(np.uint8)
        kps_all = np.ascontiguousarray(np.concatenate([p[5] for p in prep]), dtype=np.float32)
        pred = self.model.forward_frames([np.ascontiguousarray(p[1]) for p in prep], [np.asarray(p[4], np.float32) for p in prep], check=False,
                                         extra=[mm_all, kps_all])
        mm_dev, kps_dev = pred["extra"]
        self._launch_single_views(fg, ff, pred, mm_dev, kps_dev, np.concatenate([p[7] for p in prep]), [o for p in prep for o in p[3]],
                                  seed=self._seed_base, seed_dev=self._seed_run)
        # ("call": the network call whose validity decides the batch's, PkpNet.call_range_exceeded)
        self._tickets.append({"prep": prep, "ff": ff, "fg": fg, "pred": pred, "call": self.model.last_call(), "t0": t0})

    @_on_stream
    def submit_views_single(self, views):
        """First half of process_views_single: prepare the batch and enqueue its device work.  Up to two batches may be in flight."""
        assert self.single_views_take_the_device_chain(views), "submit_views_single: this batch does not take the device chain (process_views_single decides)"
        assert self.views_in_flight() < 2, "two batches are already in flight: collect one first"
        if not self.views_in_flight() and self._seed_run is not None and self._seed_expect + self._seed_base != self._pnp_seed:
            # nothing in flight: the host's seed is complete -- rebase the device-resident key on it (another route has advanced it meanwhile)
            self._seed_run.zero_()
            self._seed_base, self._seed_expect = self._pnp_seed, 0
        prep, ff = [], [0]
        for view_id, img, K, obj_ids, bboxes, model_kps, model_kps_masks, _ in views:
            obj_ids = np.asarray(obj_ids)
            bboxes = np.array(bboxes, dtype=np.float64)
            bboxes[:, [0, 1]] *= 1.0 - self.bbox_inflate                                               # (process_view, :368-369)
            bboxes[:, [2, 3]] *= 1.0 + self.bbox_inflate
            K_bbox = fix_K_for_bbox_ndc_many(K, bboxes).astype(np.float32)
            prep.append((view_id, img, K, obj_ids, bboxes, np.asarray(model_kps), np.asarray(model_kps_masks, dtype=bool), K_bbox))
            ff.append(ff[-1] + len(obj_ids))
        assert ff[-1] <= self.model.max_crops, f"{ff[-1]} crops in one call, the network was built for {self.model.max_crops} (ObjectSLAM(max_crops=...))"
        self._enqueue_views(prep, ff, time())

    @_on_stream
    def collect_views_single(self):
        """Second half: wait for the OLDEST batch in flight, install its state view by view and return [collect_results() per view]."""
        tk = self._tickets[0]
        r = tk["fg"].fetch(copy=True)
        if self.model.call_range_exceeded(tk["call"]):
            # fp16 form only: this batch's own call left the range (a batch still in flight behind it cannot mark it) -- its results are invalid, and so are those
            # of every batch enqueued after it: their PnP keys continue from its counts on the running key.  The network is on bf16x3 now: re-issue them all in
            # order from the host's seed, which only ever counted valid batches.  Batches collected before it were valid and stay.
            redo = self._tickets
            self._tickets = []
            self.fp16_range_reissues += len(redo)
            import torch
            torch.cuda.synchronize()                          # (the batches behind it drain before their contexts and the key are reused)
            self._seed_run.zero_()
            self._seed_base, self._seed_expect = self._pnp_seed, 0
            for t in redo:
                self._enqueue_views(t["prep"], t["ff"], t["t0"])
            tk = self._tickets[0]
            r = tk["fg"].fetch(copy=True)
        self._tickets.pop(0)
        prep, ff = tk["prep"], tk["ff"]
        n_solv = int(np.count_nonzero(r["n_kp"] >= 4))
        self._pnp_seed += n_solv
        self._seed_expect += n_solv
        now = time()
        per_view = (now - max(tk["t0"], self._last_collect)) / len(prep)              # batches overlap: the time this batch added to the stream of results
        self._last_collect = now
        out = []
        for f, (view_id, img, K, obj_ids, bboxes, model_kps, model_kps_masks, K_bbox) in enumerate(prep):
            self.reset()
            self.cam_K[view_id] = K
            self.images[view_id] = img
            self.all_time_num_views += 1
            self._ingest_single_view(view_id, obj_ids, bboxes, model_kps, model_kps_masks, K_bbox, r, ff[f], f)
            if self.all_time_num_views > 5:
                self.track_time_meter.update(per_view)
            self.needs_opt = False
            out.append(self.collect_results(no_viz=True))
        return out

    # ---- SLAM views -----------------------------------------------------------------------------
    def _frame_on_device(self, img):
        """The frame of the current view on the device: uploaded once (pinned staging + copy kernel, pkpnet.PkpNet._to_device) and handed to
        BOTH network passes of a SLAM view (the reference uploads the full frame per pass, lib/object_slam.py:1092-1098)."""
        import torch
        key = (id(img), getattr(img, "shape", None))
        if self._frame_key != key or self._frame_dev is None:
            host = np.ascontiguousarray(img)
            self._frame_dev = self.model._to_device(torch.from_numpy(host)) if isinstance(host, np.ndarray) and host.dtype == np.uint8 else host
            self._frame_key = key
        return self._frame_dev

    def _run_kp_model_chain(self, img, K_bbox, obj_ids, bboxes, model_kps, model_kps_masks, kp_masks_gt, uv_gt, prior_dets):
        """__run_kp_model (object_slam.py:1077-1167) of a SLAM pass with everything between the network and the PnP poses on the device: network -> masks ->
        compaction -> normalisation -> batched PnP -> acceptance as ONE stream-ordered chain (suo_frame_geom_launch with do_lm = 0: the camera hypotheses of
        :975-1072 continue on the host) and ONE read-back, where the host route makes three read-backs, compacts in Python and ships the points back for the PnP
        launch.  Same kernels on the same numbers: PnP poses and statuses are those of the host route bit for bit (tests/test_gpu_frame_geom.py)."""
        cp = self._chain_pass(None, (obj_ids, bboxes, model_kps, model_kps_masks, kp_masks_gt, uv_gt), K_bbox=K_bbox, prior_dets=prior_dets)
        fg = self._fg = _geometry(self._fg, cp.L)
        for _attempt in range(2):
            cp.enqueue(self.model, fg, self._frame_on_device(img), self._pnp_seed)
            r = fg.fetch(copy=True)
            if not self.model.call_range_exceeded(cp.pred.call):  # (fp16 form only: the fetch synchronised; on True the network is on bf16x3 now, once more)
                break
            self.fp16_range_reissues += 1
        self._pnp_seed += int(np.count_nonzero(r["n_kp"] >= 4))
        return self._kp_det_from_chain(r, obj_ids, model_kps, K_bbox, uv_gt)

    def _kp_det_from_chain(self, r, obj_ids, model_kps, K_bbox, uv_gt, lo=0, lm_inliers=False):
        """What __run_kp_model returns per object (:1150-1165), from crops [lo, lo + L) of a chain read-back.  Everything kept is COPIED out of r (fetch(copy=False)
        hands out views into the pinned block).  lm_inliers: the inlier flags the chain's LM left (do_lm), else all true as PnP's are (:40)."""
        ret = []
        for k, obj_id in enumerate(obj_ids):
            c = lo + k
            m = r["mask"][c]
            n = int(r["n_kp"][c])
            self.obj_num_dets[obj_id] += 1
            self.obj_num_det_kps[obj_id] += n
            ret.append({"pose": r["T_pnp"][c].copy() if r["accepted"][c] else None, "inliers": r["inlier"][c, :n].copy() if lm_inliers else np.ones(n, dtype=bool),
                        "kp_mask": m, "model_kp": model_kps[k][m].astype(np.float64), "uv_gt": uv_gt, "uv_pred": r["uv"][c][m].astype(np.float64),
                        "cov_pred": None if self.no_network_cov else r["cov"][c][m], "K": K_bbox[k].astype(np.float64), "score": 0.0 if n == 0 else 1.0})
        return ret

    def _slam_view_takes_the_vote_chain(self, view_id, cam_pose, n_non_sym, n_sym):
        """Both passes of a SLAM view as ONE device chain (pass A -> PnP -> hypothesis vote -> prior projection -> pass B): a tracking view of a running map with
        objects of both kinds, on the routes that keep their keypoints on the device.  SUO_SLAM_VOTE_CHAIN=0: the host votes between the passes (A/B)."""
        return (self.device_chain and self.model is not None and (not self.debug_gt_kp or self.debug_gt_on_device) and not self.single_view_mode and cam_pose is None
                and not self.no_prior_det and 0 < n_non_sym <= 16 and 0 < n_sym <= 16 and self.num_views_processed() > 0 and view_id not in self.cam_poses
                and os.environ.get("SUO_SLAM_VOTE_CHAIN", "1") not in ("", "0"))

    def _process_view_slam_chain(self, view_id, img, K, A, B):
        """A SLAM view's two network passes with NOTHING on the host between them (round 6; lib/object_slam.py:464-593 twice, :975-1072 between): pass A (the
        non-symmetric objects) -> masks -> compaction -> PnP -> acceptance (csrc/frame_geom.hip) -> camera-hypothesis vote + projection of the symmetric objects' prior
        keypoints (csrc/slam_vote.hip) -> pass B with device-rendered priors -> its PnP, enqueued back to back; the host reads pass A's block and the vote while pass B
        runs and does pass A's bookkeeping under it.  A / B = (obj_ids, bboxes, model_kps, model_kps_masks, kp_masks, uv_gt) of the two passes.  Leaves the state the
        two _process_objects calls leave; when no hypothesis reaches four inliers (:1067) it returns False with pass A installed, and the caller continues as the
        reference does (__backup_estimate_camera_pose, then pass B again with that pose)."""
        import ctypes as C
        import torch
        from . import _lib
        lib = _lib.lib()
        ids_a, bb_a, kps_a, mm_a = A[:4]
        ids_b, bb_b, kps_b, mm_b = B[:4]
        La, Lb = len(ids_a), len(ids_b)
        fg_a = self._fg = _geometry(self._fg, max(La, Lb))
        fg_b = self._fg2 = _geometry(self._fg2, max(La, Lb))
        P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        # pass A's host arrays now; pass B's and the vote's block are prepared AFTER pass A is enqueued, under its GPU time
        pa = self._chain_pass(K, A)
        rng_after_a = self._rng.bit_generator.state if self.debug_gt_kp else None      # (a pass B that has to be issued again draws its noise again: from here)
        pb = None
        for _attempt in range(2):
            frame = self._frame_on_device(img)
            dev = self.model.device
            seed_run = torch.zeros(1, dtype=torch.int64, device=dev)
            # ---- pass A
            pa.enqueue(self.model, fg_a, frame, self._pnp_seed, seed_dev=seed_run, out_slot="slam A")
            ra_dev = fg_a.device_result()
            if pb is None:
                pb = self._chain_pass(K, B, block=vote_block(K, ids_a, pa.K_bbox, ids_b, bb_b, self.obj_poses))
            pb.stage(self.model)
            puv = torch.empty((Lb, NUM_KP, 2), dtype=torch.float32, device=dev)
            pmk = torch.empty((Lb, NUM_KP), dtype=torch.uint8, device=dev)
            vout = torch.empty(32, dtype=torch.float64, device=dev)
            # ---- vote + priors, on the stream, behind pass A's PnP (the masks as the chain used them: without the keypoints it dropped for a singular covariance)
            _lib.check(lib.suo_slam_vote(La, ra_dev.T_pnp, ra_dev.accepted, ra_dev.n_kp, P(pa.uv_dev), P(pa.pred["cov"]), ra_dev.mask, P(pa.kps_dev),
                                         P(pb.block_dev), Lb, P(pb.kps_dev), P(pb.class_mask_dev), int(not self.no_network_cov), float(self.manual_kp_std) ** 2,
                                         CHI2_2DOF_95, 4, P(puv), P(pmk), P(vout), C.c_void_p(_lib.current_stream_ptr())), "suo_slam_vote")
            if self._vote_pin is None:
                self._vote_pin = (torch.empty(32, dtype=torch.float64).pin_memory(), torch.empty((16, NUM_KP, 2), dtype=torch.float32).pin_memory(),
                                  torch.empty((16, NUM_KP), dtype=torch.uint8).pin_memory(), torch.cuda.Event())
            v_pin, puv_pin, pmk_pin, v_ev = self._vote_pin
            v_pin.copy_(vout, non_blocking=True)
            puv_pin[:Lb].copy_(puv, non_blocking=True)
            pmk_pin[:Lb].copy_(pmk, non_blocking=True)
            v_ev.record()
            # ---- pass B: priors rendered on the device from what the vote kernel wrote; nothing above has waited
            pb.launch(self.model, fg_b, frame, self._pnp_seed, seed_dev=seed_run, prior_uv=puv, prior_mask=pmk, out_slot="slam B")
            # ---- the host, under pass B: pass A's block and the vote
            ra = fg_a.fetch(copy=False)                       # (views into the pinned block: everything the state keeps is copied out per object below)
            v_ev.synchronize()
            vote = v_pin.numpy().copy()
            prior_uv_h, prior_mask_h = puv_pin[:Lb].numpy().copy(), pmk_pin[:Lb].numpy().copy()
            if not self.model.call_range_exceeded(pa.pred.call):   # (pass A's own call: pass B, still running, cannot mark it)
                break
            # (fp16 form only) pass A left the range: its results -- and the priors pass B is running on -- are invalid.  Let pass B drain, then both again on bf16x3
            fg_b.fetch(copy=False)
            self.fp16_range_reissues += 2
        assert vote[31] == 0.0, "NaN in information matrix"
        n_solv_a = int(np.count_nonzero(ra["n_kp"] >= 4))
        best = int(vote[12])
        hyp_ids = [o for k, o in enumerate(ids_a) if vote[15 + k] >= 0]
        # ---- pass A into the state, with the device's vote -- while pass B runs
        self._pnp_seed += n_solv_a
        det_a = self._kp_det_from_chain(ra, ids_a, kps_a, pa.K_bbox, A[5])
        cam = None
        if best >= 0:
            cam = np.eye(4)
            cam[:3, :4] = vote[:12].reshape(3, 4)
        self.last_cam_hypotheses = ({"obj_ids": hyp_ids, "counts": [int(vote[15 + k]) for k in range(La) if vote[15 + k] >= 0], "best_num_inliers": int(vote[14])}
                                    if hyp_ids else None)
        self._install_kp_detections(view_id, ids_a, bb_a, mm_a, det_a, None, cam_vote=cam)
        rb = fg_b.fetch(copy=False)
        b_invalid = self.model.call_range_exceeded(pb.pred.call)   # (fp16 form only: pass B left the range, pass A did not -- its results stand)
        if b_invalid:
            self.fp16_range_reissues += 1
        if cam is None or b_invalid:
            # no hypothesis reached four inliers: the reference falls back to the bbox-centroid pose and THEN runs pass B -- with priors this chain did not have.
            # Pass B's speculative results are dropped (its PnP consumed sampler keys past the host's seed, which never counted them) and the caller issues the
            # pass again, one at a time; the noise draws of its ground-truth keypoints are taken back so that it draws them again.
            if rng_after_a is not None:
                self._rng.bit_generator.state = rng_after_a
            return False
        # ---- pass B into the state
        self._pnp_seed += int(np.count_nonzero(rb["n_kp"] >= 4))
        det_b = self._kp_det_from_chain(rb, ids_b, kps_b, pb.K_bbox, B[5])
        prior_det_uv = {o: prior_uv_h[k] for k, o in enumerate(ids_b) if prior_mask_h[k].any()}
        self._install_kp_detections(view_id, ids_b, bb_b, mm_b, det_b, prior_det_uv)
        return True
