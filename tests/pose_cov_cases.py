"""Synthetic graphs for the pose-covariance tests (tests/test_gpu_pose_cov.py, tests/test_pose_cov_ref.py), synthetic.make_frame-style in METRES: objects of
4-10 cm extent at 0.5-1.5 m depth, NDC keypoints with noise 0.004 and a random 2x2 covariance per keypoint whose inverse is the edge's information.  The poses
are the ground truth moved by a small left update: the state a refinement would leave (the covariance is defined at any state).  Every graph is cached with
its reference (tests/pose_cov_ref.py), computed once and never modified: tests take copies."""
import functools

import numpy as np

from tests import pose_cov_ref as R

NOISE = 0.004


def _rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _graph(rng, cam_gt, cam_fixed, n_obj, sees, kp=(6, 12), obj_fixed=None):
    """cam_gt [C,4,4] world -> camera; sees(c, o) -> bool; kp: keypoints per (camera, object) pair, drawn from [lo, hi]."""
    C = len(cam_gt)
    obj_gt, pts = [], []
    for o in range(n_obj):
        T = np.eye(4)
        T[:3, :3] = _rot(rng)
        z = rng.uniform(0.5, 1.5)
        T[:3, 3] = [rng.uniform(-0.2, 0.2) * z, rng.uniform(-0.15, 0.15) * z, z]
        obj_gt.append(T)
        pts.append(rng.uniform(-1, 1, (41, 3)) * rng.uniform(0.04, 0.1, 3))
    e_cam, e_obj, e_k, e_p, e_uv, e_info = [], [], [], [], [], []
    for c in range(C):
        for o in range(n_obj):
            if not sees(c, o):
                continue
            n = int(rng.integers(kp[0], kp[1] + 1))
            # K_bbox-like intrinsics of the crop, in NDC: the object fills most of [-1, 1]
            pc = (cam_gt[c] @ obj_gt[o] @ np.c_[pts[o], np.ones(41)].T).T[:, :3]
            xy = pc[:, :2] / pc[:, 2:3]
            half = 0.6 * (xy.max(0) - xy.min(0))
            mid = 0.5 * (xy.max(0) + xy.min(0))
            k = np.array([1 / half[0], 1 / half[1], -mid[0] / half[0], -mid[1] / half[1]])
            for j in rng.choice(41, n, replace=False):
                uv = np.array([k[0] * xy[j, 0] + k[2], k[1] * xy[j, 1] + k[3]]) + rng.normal(0, NOISE, 2)
                A = rng.normal(0, 0.3, (2, 2)) + np.eye(2)
                Om = np.linalg.inv(A @ A.T * NOISE * NOISE)
                e_cam.append(c); e_obj.append(o); e_k.append(k); e_p.append(pts[o][j]); e_uv.append(uv); e_info.append([Om[0, 0], Om[0, 1], Om[1, 1]])
    cam_fixed = np.asarray(cam_fixed, np.uint8)
    obj_fixed = np.zeros(n_obj, np.uint8) if obj_fixed is None else np.asarray(obj_fixed, np.uint8)
    move = lambda T, fixed: T if fixed else R.exp_se3(np.r_[rng.normal(0, 2e-3, 3), rng.normal(0, 1e-3, 3)]) @ T
    return {"cam_T": np.stack([move(T, f)[:3] for T, f in zip(cam_gt, cam_fixed)]), "cam_fixed": cam_fixed,
            "obj_T": np.stack([move(T, f)[:3] for T, f in zip(obj_gt, obj_fixed)]), "obj_fixed": obj_fixed,
            "edge_cam": np.array(e_cam, np.int32), "edge_obj": np.array(e_obj, np.int32), "edge_camk": np.array(e_k), "edge_p": np.array(e_p),
            "edge_uv": np.array(e_uv), "edge_info": np.array(e_info), "edge_inlier": np.ones(len(e_cam), np.uint8)}


def _arc(rng, n_cam):
    cams = []
    for c in range(n_cam):
        s = c / max(n_cam - 1, 1) - 0.5 if n_cam > 1 else 0.0
        ang = 0.5 * s
        T = np.eye(4)
        if c > 0 or n_cam == 1:
            T[:3, :3] = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
            T[:3, 3] = [-0.3 * s, rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02)]
        cams.append(T)
    return cams


def frame(seed, n_obj, kp=(6, 12)):
    """single-view frame: one fixed camera at identity, n_obj free objects"""
    rng = np.random.default_rng(seed)
    return _graph(rng, [np.eye(4)], [1], n_obj, lambda c, o: True, kp)


def cam_only(seed):
    """curr_only graph: one free camera, 2 fixed objects, 8 edges"""
    rng = np.random.default_rng(seed)
    return _graph(rng, _arc(rng, 1), [0], 2, lambda c, o: True, (4, 4), obj_fixed=[1, 1])


def coupled(seed, n_cam, n_obj, miss=0.0, kp=(6, 10)):
    """n_cam cameras on an arc, the first fixed (the gauge), n_obj free objects; every object is seen by camera 0 and missed by the others with probability miss"""
    rng = np.random.default_rng(seed)
    seen = rng.random((n_cam, n_obj)) >= miss
    seen[0] = True
    return _graph(rng, _arc(rng, n_cam), [1] + [0] * (n_cam - 1), n_obj, lambda c, o: bool(seen[c, o]), kp)


CASES = {
    "1x1_4edges": lambda: frame(1, 1, (4, 4)),
    "1x8": lambda: frame(2, 8),
    "1x9": lambda: frame(3, 9),
    "1x16": lambda: frame(4, 16),
    "1x17": lambda: frame(5, 17),
    "1x33": lambda: frame(6, 33, (5, 8)),
    "batch_3": lambda: frame(7, 3),
    "batch_16": lambda: frame(8, 16),
    "batch_1": lambda: frame(9, 1),
    "cam_only": lambda: cam_only(10),
    "3x2": lambda: coupled(11, 3, 2),
    "5x16": lambda: coupled(12, 5, 16, miss=0.3, kp=(5, 7)),
    "2x17": lambda: coupled(13, 2, 17, kp=(4, 4)),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    g = CASES[name]()
    return g, (R.covariances(g) if name != "2x17" else None)


def case(name):
    """(graph, reference): the graph a deep copy, the reference shared and read-only (None for the graph that must be refused)"""
    g, ref = _case(name)
    return {k: v.copy() for k, v in g.items()}, ref


ARGS = ("cam_T", "cam_fixed", "obj_T", "obj_fixed", "edge_cam", "edge_obj", "edge_camk", "edge_p", "edge_uv", "edge_info", "edge_inlier")


def args(g):
    return [g[k] for k in ARGS]
