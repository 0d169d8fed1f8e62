"""Consistency of the reported uncertainties: are the errors of the refined poses, and of the predicted keypoints, distributed as their covariances say?

    pose_nees(bop_errors, obj_ids, T_est, T_gt, cov)     NEES = xi^T Sigma^-1 xi of xi = log(T_est T_ref^-1), T_ref = T_gt S_s* with the symmetry of the MSSD
                                                         minimum                                       -> HIP, csrc/eval_nees.hip (suo_pose_nees)
    keypoint_nees(bop_errors, dets, T_ref)               chi2 = e^T C^-1 e of e = uv - pi(K, T_ref x)  -> HIP, csrc/eval_nees.hip (suo_keypoint_nees)
    ConsistencyMeter(bop_errors).add_poses / add_keypoints / result()

Both are reached as ``BopErrors.pose_nees`` / ``BopErrors.keypoint_nees`` (bop_eval.py): the class owns the mesh database and its symmetry sets.  The keypoint half
restates what the reference plots in plot_cov.py:138-145 (the share of keypoints inside the 99 % bound of chi2 with two degrees of freedom); the pose half has no
counterpart there.  The definitions, the tie rule and the NaN rules are those of include/suo_hip.h.  The chi2 scale is not applied anywhere.  No CPU fallback."""
from __future__ import annotations

import numpy as np

from . import _lib
from .bop_eval import pack_poses, stage_pairs

# Quantiles of the chi2 distribution (0.95, 0.99): six degrees of freedom for a pose (standard tables: 12.5916, 16.8119), two for a keypoint (-2 ln 0.05 = 5.9915;
# -2 ln 0.01 = 9.2103, kept as the reference's own literal 9.210, plot_cov.py:145).
CHI2_6_95, CHI2_6_99 = 12.5916, 16.8119
CHI2_2_95, CHI2_2_99 = 5.9915, 9.210


def pose_nees(errors, obj_ids, T_est, T_gt, cov):
    """n (object, estimated pose, ground-truth pose, 6x6 covariance) items; poses [n,3|4,4], cov [n,6,6] with rows / columns [omega, upsilon] of the left update
    (ba.pose_covariances, collect_results(covariances=True)["cov_OtoC"]), all lengths in the unit of the mesh database.
    Returns ``{"nees" [n], "xi" [n,6], "sym_index" [n] (-1: a non-finite pose), "T_ref" [n,3,4], "n_nan"}``."""
    n, idx, _, Te, Tg = stage_pairs(errors._index, obj_ids, None, T_est, T_gt)
    nees, xi, sym, T_ref = np.zeros(n), np.zeros((n, 6)), np.zeros(n, np.int32), np.zeros((n, 3, 4))
    status = np.zeros(1, np.int32)
    if n:
        cv = np.ascontiguousarray(np.asarray(cov, np.float64).reshape(n, 36))
        _lib.check(errors.lib.suo_pose_nees(errors._h, n, idx.ctypes.data, Te.ctypes.data, Tg.ctypes.data, cv.ctypes.data, nees.ctypes.data, xi.ctypes.data,
                                            sym.ctypes.data, T_ref.ctypes.data, status.ctypes.data), "suo_pose_nees")
    return {"nees": nees, "xi": xi, "sym_index": sym, "T_ref": T_ref, "n_nan": int(status[0])}


def keypoint_nees(errors, dets, T_ref):
    """chi2 of the keypoints of ObjectSLAM detection dicts (keys "model_kp" [k,3], "uv_pred" [k,2], "cov_pred" [k,2,2] or None, "K" [3,3]: the host route and
    view_chain.py both fill them) at the poses T_ref [n,3|4,4].  A detection with ``cov_pred is None`` is skipped and counted.
    Returns ``{"chi2": [array [k] or None per detection], "err": [array [k,2] or None], "n_skipped"}``."""
    n = len(dets)
    T = pack_poses(T_ref, n)
    use = [i for i, d in enumerate(dets) if d.get("cov_pred") is not None]
    chi2, err = [None] * n, [None] * n
    if use:
        n_pts = np.array([int(np.asarray(dets[i]["uv_pred"]).reshape(-1, 2).shape[0]) for i in use], np.int32)
        cat = lambda key, w: np.ascontiguousarray(np.concatenate([np.asarray(dets[i][key], np.float64).reshape(-1, w) for i in use], 0))
        kp, uv, cv = cat("model_kp", 3), cat("uv_pred", 2), cat("cov_pred", 4)
        assert kp.shape[0] == uv.shape[0] == cv.shape[0] == int(n_pts.sum()), "a detection's keypoints, predictions and covariances must have one length"
        K = np.ascontiguousarray(np.stack([np.asarray(dets[i]["K"], np.float64).reshape(9) for i in use]))
        Tu = np.ascontiguousarray(T[use])
        out, e = np.zeros(int(n_pts.sum())), np.zeros((int(n_pts.sum()), 2))
        _lib.check(errors.lib.suo_keypoint_nees(errors._h, len(use), n_pts.ctypes.data, kp.ctypes.data, uv.ctypes.data, cv.ctypes.data, K.ctypes.data,
                                                Tu.ctypes.data, out.ctypes.data, e.ctypes.data), "suo_keypoint_nees")
        at = 0
        for i, k in zip(use, n_pts.tolist()):
            chi2[i], err[i] = out[at:at + k], e[at:at + k]
            at += k
    return {"chi2": chi2, "err": err, "n_skipped": n - len(use)}


def _stats(values, b95, b99, name):
    v = np.asarray(values, np.float64)
    ok = v[~np.isnan(v)]
    return {"n": int(v.size), "n_nan": int(v.size - ok.size), f"mean_{name}": float(ok.mean()) if ok.size else float("nan"),
            "frac_95": float(np.mean(ok <= b95)) if ok.size else float("nan"), "frac_99": float(np.mean(ok <= b99)) if ok.size else float("nan")}


class ConsistencyMeter:
    """Collects NEES of poses and chi2 of keypoints.  ``errors``: a bop_eval.BopErrors.  A consistent estimator gives a mean NEES of 6 with 95 % / 99 % of the
    poses below CHI2_6_95 / CHI2_6_99, and a mean keypoint chi2 of 2 with 95 % / 99 % below CHI2_2_95 / CHI2_2_99.  NaN results (include/suo_hip.h) are counted
    in ``n_nan`` and left out of the means and shares.  Models whose models_info entry has ``symmetries_continuous`` are left out of the pose aggregate and
    counted in ``n_skipped_continuous``: the rotation about their axis is unobservable, and the toolkit's discretised set does not contain the identity
    (bop_eval.symmetry_transformations).  Their T_ref is still computed, for the keypoints."""

    def __init__(self, errors):
        self.errors = errors
        self._nees = {}                      # obj_id -> [nees]
        self._chi2 = []
        self.n_skipped_continuous = 0
        self.n_skipped_detections = 0

    def _continuous(self, obj_id):
        return bool(self.errors.models_info.get(int(obj_id), {}).get("symmetries_continuous"))

    def add_poses(self, obj_ids, T_est, T_gt, cov):
        """Returns BopErrors.pose_nees' dict for ALL the items (T_ref is what add_keypoints wants)."""
        res = self.errors.pose_nees(obj_ids, T_est, T_gt, cov)
        for o, v in zip(obj_ids, res["nees"].tolist()):
            if self._continuous(o):
                self.n_skipped_continuous += 1
            else:
                self._nees.setdefault(int(o), []).append(v)
        return res

    def add_keypoints(self, dets, T_ref):
        res = self.errors.keypoint_nees(dets, T_ref)
        self.n_skipped_detections += res["n_skipped"]
        self._chi2.extend(c for c in res["chi2"] if c is not None)
        return res

    def result(self):
        """``{"pose": {"n", "n_nan", "mean_nees", "frac_95", "frac_99", "per_object": {obj_id: {the same five}}, "n_skipped_continuous"},
        "keypoint": {"n", "n_nan", "n_skipped" (detections without a covariance), "mean_chi2", "frac_95", "frac_99"}}``."""
        every = [v for o in sorted(self._nees) for v in self._nees[o]]
        pose = _stats(every, CHI2_6_95, CHI2_6_99, "nees")
        pose["per_object"] = {o: _stats(self._nees[o], CHI2_6_95, CHI2_6_99, "nees") for o in sorted(self._nees)}
        pose["n_skipped_continuous"] = int(self.n_skipped_continuous)
        kp = _stats(np.concatenate(self._chi2) if self._chi2 else np.zeros(0), CHI2_2_95, CHI2_2_99, "chi2")
        kp["n_skipped"] = int(self.n_skipped_detections)
        return {"pose": pose, "keypoint": kp}
