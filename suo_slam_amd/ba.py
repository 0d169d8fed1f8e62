"""Flat-SoA front end of the HIP pose-refinement / bundle-adjustment kernel (csrc/lm.hip), the
replacement for the g2o graph that ObjectSLAM.optimize builds (/root/reference/lib/object_slam.py:703-903)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

CHI2_THR = 5.991                       # lib/object_slam.py:680,860
HUBER_DELTA = float(np.sqrt(5.991))    # lib/object_slam.py:831


class Problem:
    """One optimize() call.  Arrays are copied; results are read back from .cam_T/.obj_T/.inlier/.chi2/.stats."""

    def __init__(self, cam_T, cam_fixed, obj_T, obj_fixed, edge_cam, edge_obj, edge_camk, edge_p, edge_uv, edge_info,
                 edge_inlier, its=(10, 10, 40, 40), init_with_outliers=False, chi2_thr=CHI2_THR, huber_delta=HUBER_DELTA):
        self.cam_T = np.ascontiguousarray(np.asarray(cam_T, np.float64)[..., :3, :4]).reshape(-1, 12).copy()
        self.obj_T = np.ascontiguousarray(np.asarray(obj_T, np.float64)[..., :3, :4]).reshape(-1, 12).copy()
        self.cam_fixed = np.ascontiguousarray(cam_fixed, np.uint8).copy()
        self.obj_fixed = np.ascontiguousarray(obj_fixed, np.uint8).copy()
        self.edge_cam = np.ascontiguousarray(edge_cam, np.int32).copy()
        self.edge_obj = np.ascontiguousarray(edge_obj, np.int32).copy()
        E = len(self.edge_cam)
        self.edge_camk = np.ascontiguousarray(edge_camk, np.float64).reshape(E, 4).copy()
        self.edge_p = np.ascontiguousarray(edge_p, np.float64).reshape(E, 3).copy()
        self.edge_uv = np.ascontiguousarray(edge_uv, np.float64).reshape(E, 2).copy()
        info = np.asarray(edge_info, np.float64)
        if info.ndim == 3:
            info = np.stack([info[:, 0, 0], info[:, 0, 1], info[:, 1, 1]], -1)
        self.edge_info = np.ascontiguousarray(info).reshape(E, 3).copy()
        self.inlier = np.ascontiguousarray(edge_inlier, np.uint8).copy()
        self.chi2 = np.zeros(max(E, 1))
        self.its = tuple(int(i) for i in its)
        self.init_with_outliers = bool(init_with_outliers)
        self.chi2_thr = float(chi2_thr)
        self.huber_delta = float(huber_delta)
        self.stats = np.zeros(4, np.int32)

    def _fill(self, s):
        s.n_cam, s.n_obj, s.n_edge = len(self.cam_T), len(self.obj_T), len(self.edge_cam)
        for name in ("cam_T", "cam_fixed", "obj_T", "obj_fixed", "edge_cam", "edge_obj", "edge_camk", "edge_p", "edge_uv", "edge_info"):
            setattr(s, name, getattr(self, name).ctypes.data)
        s.edge_inlier = self.inlier.ctypes.data
        s.edge_chi2 = self.chi2.ctypes.data
        for i, v in enumerate(self.its):
            s.its[i] = v
        s.n_rounds = len(self.its)
        s.init_with_outliers = int(self.init_with_outliers)
        s.chi2_thr = self.chi2_thr
        s.huber_delta = self.huber_delta


def optimize_batch(problems):
    """Run many independent problems (e.g. one per frame) in one launch; results land in each Problem."""
    if not problems:
        return problems
    lib = _lib.lib()
    _lib.require_gpu()
    arr = (_lib.BaProblem * len(problems))()
    for s, p in zip(arr, problems):
        p._fill(s)
    _lib.check(lib.suo_optimize_batch(C.cast(arr, C.c_void_p), len(problems)), "suo_optimize_batch")
    for s, p in zip(arr, problems):
        p.stats[:] = list(s.stats)
        p.chi2 = p.chi2[:len(p.edge_cam)]
    return problems


def optimize(*args, **kw):
    p = Problem(*args, **kw)
    optimize_batch([p])
    return p.cam_T.reshape(-1, 3, 4), p.obj_T.reshape(-1, 3, 4), p.inlier, p.chi2, p.stats


def _call_batch(entry, problems, bufs, *flat, lead=()):
    """One call of a covariance batch entry of the C ABI: (BaProblem array, n, *lead, one pointer column per buffer of bufs[i], *flat).  bufs[i]: problem i's
    arrays, one per column, in the entry's order; lead / flat: arrays with one row per problem.  Everything stays alive until the call has returned."""
    _lib.require_gpu()
    n = len(problems)
    arr = (_lib.BaProblem * n)()
    for s, p in zip(arr, problems):
        p._fill(s)
    cols = [(C.c_void_p * n)(*[b.ctypes.data for b in col]) for col in zip(*bufs)]
    _lib.check(getattr(_lib.lib(), entry)(C.cast(arr, C.c_void_p), n, *[a.ctypes.data for a in lead], *[C.cast(c, C.c_void_p) for c in cols],
                                   *[a.ctypes.data for a in flat]), entry)


def pose_covariances_batch(problems):
    """6x6 marginal covariances of every camera and object pose of each Problem at the state it holds (cam_T, obj_T, inlier): the diagonal blocks of the inverse
    Gauss-Newton Hessian, rows and columns [omega, upsilon] of the left update exp(delta) T (include/suo_hip.h: suo_pose_covariances).  One call for the whole
    list; per problem (cam_cov [C,6,6], obj_cov [O,6,6], status [2] = NaN camera blocks, NaN object blocks).  The problems are not modified."""
    if not problems:
        return []
    status = np.zeros((len(problems), 2), np.int32)
    bufs = [(np.zeros((len(p.cam_T), 6, 6)), np.zeros((len(p.obj_T), 6, 6))) for p in problems]
    _call_batch("suo_pose_covariances_batch", problems, bufs, status)
    return [b + (st,) for b, st in zip(bufs, status)]


def pose_covariances(*args, **kw):
    """The arguments of optimize(); returns (cam_cov [C,6,6], obj_cov [O,6,6], status [2]) at the poses and inlier flags given."""
    return pose_covariances_batch([Problem(*args, **kw)])[0]


def pose_covariances_pairs_batch(problems, pairs):
    """pose_covariances_batch plus, per problem, the cross block and the relative-pose covariance of the vertex pairs in pairs[i] ([P,2] ints; camera c is c,
    object o is n_cam + o; (camera, object) in either order or (object, object)): cross [P,6,6] = Sigma_ab, rows vertex a; rel [P,6,6] = the covariance of
    T_OtoC = T_c T_o, or of T_AtoB = T_b^-1 T_a (include/suo_hip.h: suo_pose_covariances_pairs).  Per problem (cam_cov, obj_cov, cross, rel, status [3] = NaN
    camera blocks, NaN object blocks, NaN pairs).  One call for the whole list; the problems are not modified."""
    return _pairs_batch(problems, pairs, "suo_pose_covariances_pairs_batch")


def _pairs_batch(problems, pairs, entry):
    """the shared body of pose_covariances_pairs_batch and pose_covariances_graph_batch: `entry` is the C function, both have one signature"""
    if not problems:
        return []
    if len(pairs) != len(problems):
        raise ValueError(f"{entry[4:]}: one pair list per problem")
    _lib.require_gpu()                                      # (before the argument checks below, as ever)
    status = np.zeros((len(problems), 3), np.int32)
    bufs = []                                               # pair_a, pair_b, cam_cov, obj_cov, cross, rel
    for p, pr in zip(problems, pairs):
        pr = np.asarray(pr, np.int32).reshape(-1, 2)
        bufs.append((np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1]), np.zeros((len(p.cam_T), 6, 6)), np.zeros((len(p.obj_T), 6, 6)),
                     np.zeros((len(pr), 6, 6)), np.zeros((len(pr), 6, 6))))
    _call_batch(entry, problems, bufs, status, lead=(np.array([len(b[0]) for b in bufs], np.int32),))
    return [b[2:] + (st,) for b, st in zip(bufs, status)]


def pose_covariances_pairs(*args, pairs, **kw):
    """The arguments of optimize() plus pairs [P,2]; returns (cam_cov [C,6,6], obj_cov [O,6,6], cross [P,6,6], rel [P,6,6], status [3])."""
    return pose_covariances_pairs_batch([Problem(*args, **kw)], [pairs])[0]


def pose_covariances_graph_batch(problems, pairs):
    """pose_covariances_pairs_batch without its two limits (include/suo_hip.h: suo_pose_covariances_graph): free cameras next to up to 64 free objects, and
    (camera a, camera b) pairs -- cross = Sigma_ab, rel = the covariance of T_b T_a^-1, the motion between the two views.  The same return values; bit-identical
    to pose_covariances_pairs_batch wherever that answers and no (camera, camera) pair is asked for."""
    return _pairs_batch(problems, pairs, "suo_pose_covariances_graph_batch")


def pose_covariances_graph(*args, pairs, **kw):
    """The arguments of optimize() plus pairs [P,2]; returns (cam_cov [C,6,6], obj_cov [O,6,6], cross [P,6,6], rel [P,6,6], status [3])."""
    return pose_covariances_graph_batch([Problem(*args, **kw)], [pairs])[0]


TRACK_KEYS = ("cam_cov", "fixed_map_cov", "cross", "rel")


def tracking_covariances_batch(problems, map_covs):
    """The covariance of every tracked camera of each Problem with the map's uncertainty carried in (include/suo_hip.h: suo_tracking_covariances).  Every object
    of a Problem is fixed (the curr_only graph); map_covs[i] [6 O, 6 O] is the covariance of its stacked object perturbations, e.g. assembled from
    pose_covariances_graph -- only the upper triangle is read, and an object whose block starts with NaN is not in the map.  Per problem a dict: cam_cov [C,6,6] =
    Hcc^-1 + G Sigma G^T, fixed_map_cov [C,6,6] = Hcc^-1 (pose_covariances' camera blocks, bit for bit, when every object is in the map), cross [C,O,6,6] = Sigma_co
    (rows the camera), rel [C,O,6,6] = the covariance of T_c T_o, status [2] = NaN cameras, objects not in the map.  One call for the whole list; the problems are
    not modified."""
    if not problems:
        return []
    if len(map_covs) != len(problems):
        raise ValueError("tracking_covariances_batch: one map covariance per problem")
    _lib.require_gpu()                                      # (before the shape check below, as ever)
    status = np.zeros((len(problems), 2), np.int32)
    bufs = []                                               # map_cov, cam_cov, fixed_map_cov, cross, rel
    for i, (p, m) in enumerate(zip(problems, map_covs)):
        nc, no = len(p.cam_T), len(p.obj_T)
        m = np.ascontiguousarray(m, np.float64)
        if m.shape != (6 * no, 6 * no):
            raise ValueError(f"tracking_covariances_batch: problem {i}: map covariance of shape {m.shape}, expected {(6 * no, 6 * no)}")
        bufs.append((m, np.zeros((nc, 6, 6)), np.zeros((nc, 6, 6)), np.zeros((nc, no, 6, 6)), np.zeros((nc, no, 6, 6))))
    _call_batch("suo_tracking_covariances_batch", problems, bufs, status)
    return [dict(zip(TRACK_KEYS, b[1:]), status=st) for b, st in zip(bufs, status)]


def tracking_covariances(*args, map_cov, **kw):
    """The arguments of optimize() plus map_cov [6 O, 6 O]; returns the dict of tracking_covariances_batch at the poses and inlier flags given."""
    return tracking_covariances_batch([Problem(*args, **kw)], [map_cov])[0]


RESID_KEYS = ("cam_cov", "obj_cov", "edge_chi2", "edge_pcov", "edge_lev", "edge_t", "cam_stat", "obj_stat")


def residual_statistics_batch(problems):
    """Per-edge leverages, studentised residuals and the chi2 scale of each Problem at the state it holds (include/suo_hip.h: suo_residual_statistics), one call
    for the whole list.  Per problem a dict: cam_cov [C,6,6] / obj_cov [O,6,6] (those of pose_covariances_graph, bit for bit), and for EVERY edge, in the caller's
    order, edge_chi2 [E] = v^T Omega v, edge_pcov [E,3] = J Sigma J^T as (xx, xy, yy), edge_lev [E] = tr(P Omega), edge_t [E] = v^T (Omega^-1 -/+ P)^-1 v (minus for a
    counted edge; NaN where the edge has no redundancy or touches a NaN vertex); cam_stat [C,3] / obj_stat [O,3] = (count, sum chi2, sum 2 - lev) over the vertex's
    counted edges; summary [6] = m, n, sum chi2, sum lev, dof = 2 m - n, s0^2 = sum chi2 / dof (NaN when dof <= 0); status [4] = NaN camera blocks, NaN object
    blocks, NaN edges, edges without redundancy.  The problems are not modified."""
    if not problems:
        return []
    summary = np.zeros((len(problems), 6))
    status = np.zeros((len(problems), 4), np.int32)
    bufs = []
    for p in problems:
        nc, no, E = len(p.cam_T), len(p.obj_T), len(p.edge_cam)
        bufs.append((np.zeros((nc, 6, 6)), np.zeros((no, 6, 6)), np.zeros(E), np.zeros((E, 3)), np.zeros(E), np.zeros(E), np.zeros((nc, 3)), np.zeros((no, 3))))
    _call_batch("suo_residual_statistics_batch", problems, bufs, summary, status)
    return [dict(zip(RESID_KEYS, b), summary=sm, status=st) for b, sm, st in zip(bufs, summary, status)]


def residual_statistics(*args, **kw):
    """The arguments of optimize(); returns the dict of residual_statistics_batch at the poses and inlier flags given."""
    return residual_statistics_batch([Problem(*args, **kw)])[0]
