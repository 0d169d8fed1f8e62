"""Bundle-adjustment graphs placed on the dispatch boundaries of suo_optimize_batch (csrc/ba_api.hip), each with the kernel route the dispatcher
must pick for every problem of it.  tests/test_lm_routes.py holds the table against suo_debug_lm_routes on the CPU; tests/test_gpu_lm_routes.py runs
every case on the GPU against the C oracle.

Every graph carries anisotropic information: per edge Sigma = R(theta) diag(s1^2, s2^2) R(theta)^T with theta uniform and s1 / s2 up to 10, the pixel
noise drawn from Sigma and info = inv(Sigma) stored as (xx, xy, yy), so xy takes both signs and xx != yy.  5-15 % of the measurements are outliers:
half of them a few Huber deltas out (Mahalanobis 3-8, where the Huber weight is between 0.3 and 0.8), half gross (anywhere in the image)."""
from __future__ import annotations

import os
import re
import zlib

import numpy as np

from suo_slam_amd import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("cam_T", "cam_fixed", "obj_T", "obj_fixed", "edge_cam", "edge_obj", "edge_camk", "edge_p", "edge_uv", "edge_info", "edge_inlier")
K_PIX = np.array([600.0, 600.0, 320.0, 240.0])
LM_LDS_CAP = 150 * 1024          # csrc/lm.hip: LM_LDS_BYTES
LM_STAGE_EDGES = 384             # csrc/lm.hip: the Jacobian stage above this many edges


def route_codes():
    """{name: code} of the SUO_LM_ROUTE_* macros of include/suo_hip.h."""
    hdr = open(os.path.join(ROOT, "include", "suo_hip.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+SUO_LM_ROUTE_([A-Z0-9_]+)\s+(\d+)", hdr)}


TUNING_ONLY_ROUTES: set = set()  # every route of include/suo_hip.h is in the product library


# ---- graph builders ---------------------------------------------------------------------------------------------------------------------------------


def _cameras(rng, n_cam):
    cam = np.zeros((n_cam, 3, 4))
    for c in range(n_cam):
        s = c / max(n_cam - 1, 1) - 0.5
        ang = 0.5 * s
        cam[c, :, :3] = [[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]
        cam[c, :, 3] = [-300 * s, rng.uniform(-20, 20), rng.uniform(-20, 20)]
    return cam


def _objects(rng, n_obj):
    obj = np.zeros((n_obj, 3, 4))
    for o in range(n_obj):
        obj[o, :, :3] = S.random_rotation(rng)
        obj[o, :, 3] = [rng.uniform(-200, 200), rng.uniform(-120, 120), rng.uniform(800, 1100)]
    return obj


def anisotropic_noise(rng, n, s_min=0.4, ratio=10.0):
    """(noise [n,2], info [n,3] = (xx, xy, yy) of inv(Sigma)) for Sigma = R(theta) diag(s1^2, s2^2) R(theta)^T, s1 / s2 in [1, ratio] either way."""
    th = rng.uniform(0, np.pi, n)
    s1 = s_min * np.exp(rng.uniform(0, np.log(ratio), n))
    s2 = s_min * np.exp(rng.uniform(0, np.log(ratio), n))
    c, s = np.cos(th), np.sin(th)
    R = np.stack([np.stack([c, -s], -1), np.stack([s, c], -1)], -2)                  # [n,2,2]
    z = rng.standard_normal((n, 2)) * np.stack([s1, s2], -1)
    noise = np.einsum("nij,nj->ni", R, z)
    Sig = R @ (np.stack([s1 ** 2, s2 ** 2], -1)[:, :, None] * np.transpose(R, (0, 2, 1)))
    Inf = np.linalg.inv(Sig)
    info = np.stack([Inf[:, 0, 0], 0.5 * (Inf[:, 0, 1] + Inf[:, 1, 0]), Inf[:, 1, 1]], -1)
    return noise, info, Sig


def graph(rng, counts, cam_fixed, obj_fixed, outlier_frac=None, gross_objects=(), perturb=(5e-4, 0.3)):
    """A pose graph with counts[c, o] edges between camera c and object o (each edge its own model point), anisotropic information, outliers as in
    the module doc; every free vertex starts perturbed from the truth by perturb = (rot [rad], trans [mm]).  gross_objects: objects ALL of whose measurements are
    gross outliers.  The truth rides along under "cam_gt" / "obj_gt" (not in KEYS: no solver sees it)."""
    counts = np.asarray(counts, int)
    n_cam, n_obj = counts.shape
    cam_gt, obj_gt = _cameras(rng, n_cam), _objects(rng, n_obj)
    e_cam, e_obj, e_p, e_uv, e_info = [], [], [], [], []
    for c in range(n_cam):
        for o in range(n_obj):
            k = int(counts[c, o])
            if k == 0:
                continue
            pts = rng.uniform(-60, 60, (k, 3))
            pw = pts @ obj_gt[o, :, :3].T + obj_gt[o, :, 3]
            pc = pw @ cam_gt[c, :, :3].T + cam_gt[c, :, 3]
            uv = np.c_[K_PIX[0] * pc[:, 0] / pc[:, 2] + K_PIX[2], K_PIX[1] * pc[:, 1] / pc[:, 2] + K_PIX[3]]
            noise, info, Sig = anisotropic_noise(rng, k)
            uv = uv + noise
            e_cam += [c] * k
            e_obj += [o] * k
            e_p.append(pts)
            e_uv.append(uv)
            e_info.append(info)
            if o in gross_objects:
                uv[:] = rng.uniform((0, 0), (640, 480), (k, 2))
                continue
            frac = rng.uniform(0.05, 0.15) if outlier_frac is None else outlier_frac
            bad = np.flatnonzero(rng.random(k) < frac)
            for j, i in enumerate(bad):
                if j % 2 == 0:            # a few deltas out, along a random direction of the whitened residual
                    d = rng.uniform(3.0, 8.0)
                    u = rng.standard_normal(2)
                    u /= np.linalg.norm(u)
                    uv[i] += np.linalg.cholesky(Sig[i]) @ (d * u)
                else:                     # gross
                    uv[i] = rng.uniform((0, 0), (640, 480))
    E = len(e_cam)
    cam_fixed = np.asarray(cam_fixed, np.uint8)
    obj_fixed = np.asarray(obj_fixed, np.uint8)
    rot, trans = perturb
    cam_T = np.stack([T if cam_fixed[c] else S._perturb_pose(T, rng, rot, trans) for c, T in enumerate(cam_gt)])
    obj_T = np.stack([T if obj_fixed[o] else S._perturb_pose(T, rng, rot, trans) for o, T in enumerate(obj_gt)])
    return {"cam_T": cam_T, "cam_fixed": cam_fixed, "obj_T": obj_T, "obj_fixed": obj_fixed,
            "edge_cam": np.array(e_cam, np.int32), "edge_obj": np.array(e_obj, np.int32), "edge_camk": np.tile(K_PIX, (E, 1)),
            "edge_p": np.concatenate(e_p), "edge_uv": np.concatenate(e_uv), "edge_info": np.concatenate(e_info), "edge_inlier": np.ones(E, np.uint8),
            "cam_gt": cam_gt, "obj_gt": obj_gt}


def spread(rng, total, n_cam, n_obj, miss=0.15):
    """counts [n_cam, n_obj] summing to exactly `total`, about evenly over the (camera, object) pairs a `miss` fraction of which is not seen (every object
    stays seen by two cameras at least, every camera sees something)."""
    seen = rng.random((n_cam, n_obj)) >= miss
    for o in range(n_obj):
        if seen[:, o].sum() < min(2, n_cam):
            seen[rng.choice(n_cam, min(2, n_cam), replace=False), o] = True
    for c in range(n_cam):
        if not seen[c].any():
            seen[c, rng.integers(n_obj)] = True
    idx = np.argwhere(seen)
    base, extra = divmod(total, len(idx))
    counts = np.zeros((n_cam, n_obj), int)
    counts[tuple(idx.T)] = base
    for i in rng.choice(len(idx), extra, replace=False):
        counts[tuple(idx[i])] += 1
    return counts


def frame(rng, per_obj, perturb=(3e-4, 0.2)):
    """Single-view frame: one fixed camera, objects free, per_obj[o] edges each."""
    return graph(rng, np.array([per_obj]), [1], np.zeros(len(per_obj)), perturb=perturb)


def tracking(rng, per_obj, n_fixed_cams=0, perturb=(2e-4, 0.1)):
    """Camera tracking (ObjectSLAM.optimize(curr_only=True)): ONE free camera, every object fixed; n_fixed_cams more (fixed) cameras with their own edges."""
    counts = np.array([per_obj] * (1 + n_fixed_cams))
    cam_fixed = [0] + [1] * n_fixed_cams
    return graph(rng, counts, cam_fixed, np.ones(len(per_obj)), perturb=perturb)


def global_graph(rng, total, n_cam, n_obj, miss=0.15, perturb=(5e-4, 0.3)):
    """The global adjustment: camera 0 fixed (the gauge), every other camera and every object free."""
    cf = np.zeros(n_cam)
    cf[0] = 1
    return graph(rng, spread(rng, total, n_cam, n_obj, miss), cf, np.zeros(n_obj), perturb=perturb)


def with_weak_camera(rng, P, n_kp):
    """P plus one more free camera that sees one object through n_kp keypoints only: its 6x6 block H_cc has rank 2 n_kp before lambda."""
    o = int(np.bincount(P["edge_obj"]).argmax())
    T_o, T_c = P["obj_T"][o], _cameras(rng, 3)[1]             # (measured from the object's starting pose, the camera perturbed from where it saw it)
    pts = rng.uniform(-60, 60, (n_kp, 3))
    pc = (pts @ T_o[:, :3].T + T_o[:, 3]) @ T_c[:, :3].T + T_c[:, 3]
    uv = np.c_[K_PIX[0] * pc[:, 0] / pc[:, 2] + K_PIX[2], K_PIX[1] * pc[:, 1] / pc[:, 2] + K_PIX[3]]
    noise, info, _ = anisotropic_noise(rng, n_kp)
    Q = {k: np.array(v) for k, v in P.items()}
    Q["cam_T"] = np.concatenate([P["cam_T"], S._perturb_pose(T_c, rng, 5e-4, 0.3)[None]])
    Q["cam_fixed"] = np.r_[P["cam_fixed"], 0].astype(np.uint8)
    Q["edge_cam"] = np.r_[P["edge_cam"], [len(P["cam_T"])] * n_kp].astype(np.int32)
    Q["edge_obj"] = np.r_[P["edge_obj"], [o] * n_kp].astype(np.int32)
    Q["edge_camk"] = np.concatenate([P["edge_camk"], np.tile(K_PIX, (n_kp, 1))])
    Q["edge_p"] = np.concatenate([P["edge_p"], pts])
    Q["edge_uv"] = np.concatenate([P["edge_uv"], uv + noise])
    Q["edge_info"] = np.concatenate([P["edge_info"], info])
    Q["edge_inlier"] = np.ones(len(Q["edge_cam"]), np.uint8)
    return Q


# ---- the table ----------------------------------------------------------------------------------------------------------------------------------------

TRACKING_ITS = (10, 10, 10, 10)        # lib/object_slam.py:846 (curr_only)


class Case:
    def __init__(self, name, build, routes, its=None, tracking=False):
        self.name, self._build, self.routes, self.its, self.tracking = name, build, list(routes), its, tracking

    def problems(self):
        """The case's graphs, rebuilt from its fixed seed (the same arrays on every call)."""
        return self._build(np.random.default_rng(zlib.crc32(self.name.encode())))


def _c(name, routes, its=None, tracking=False):
    def deco(fn):
        CASES.append(Case(name, fn, routes, its, tracking))
        return fn
    return deco


CASES: list = []

# FRAME2's per-object cap: 32 edges per lane, 8 lanes up to 8 objects, 4 lanes with 9-16 (ba_api.hip: frame2_takes)
_c("frame2_cap8_256", ["FRAME2"])(lambda r: [frame(r, [256, 60, 40])])
_c("frame2_cap8_257", ["FRAME8"])(lambda r: [frame(r, [257, 60, 40])])
_c("frame2_cap16_128", ["FRAME2"])(lambda r: [frame(r, [128] + [30] * 8)])
_c("frame2_cap16_129_lm", ["LM"])(lambda r: [frame(r, [129] + [30] * 8)])                # 369 edges
_c("frame2_cap16_129_lm_big", ["LM_BIG"])(lambda r: [frame(r, [129] + [50] * 8)])        # 529 edges
# FRAME2's edge budget (LF2_MAX_EDGES = 656)
_c("frame2_656", ["FRAME2"])(lambda r: [frame(r, [41] * 16)])
_c("frame2_657", ["LM_BIG"])(lambda r: [frame(r, [41] * 15 + [42])])
# 16 / 17 objects in a fixed-camera frame
_c("frame_16_objects", ["FRAME2"])(lambda r: [frame(r, [20] * 16)])
_c("frame_17_objects_lm", ["LM"])(lambda r: [frame(r, [20] * 17)])                      # 340 edges
_c("frame_17_objects_lm_big", ["LM_BIG"])(lambda r: [frame(r, [35] * 17)])              # 595 edges
# camera tracking: CAM2 up to LC2_MAX_EDGES = 1024 edges with the camera alone in its graph
_c("tracking_1024", ["CAM2"], TRACKING_ITS, True)(lambda r: [tracking(r, [128] * 8)])
_c("tracking_1025", ["CAM"], TRACKING_ITS, True)(lambda r: [tracking(r, [129] + [128] * 7)])
_c("tracking_second_fixed_camera", ["CAM"], TRACKING_ITS, True)(lambda r: [tracking(r, [20] * 6, n_fixed_cams=1)])
# the default iteration budget on lm_cam_kernel: trials are rejected here (pop() through memory, lambda * ni), which no TRACKING_ITS case reaches
_c("tracking_rejected_trials_cam", ["CAM"], None, True)(lambda r: [tracking(r, [12] * 5, n_fixed_cams=1)])
# one global graph: LM below 512 edges, the device-resident phases from 512; > 16 free objects: the host-scheduled phases at any size
_c("global_511", ["LM"])(lambda r: [global_graph(r, 511, 8, 6)])
_c("global_512", ["PHASES"])(lambda r: [global_graph(r, 512, 8, 6)])
_c("global_17_objects_300", ["PHASEWISE"])(lambda r: [global_graph(r, 300, 5, 17)])
_c("global_17_objects_700", ["PHASEWISE"])(lambda r: [global_graph(r, 700, 8, 17)])
# several free cameras, every object fixed: the block-diagonal (non-Schur) branch of lm_kernel
_c("free_cameras_fixed_objects", ["LM"])(
    lambda r: [graph(r, spread(r, 300, 5, 6, miss=0.0), np.zeros(5), np.ones(6))])
_c("free_cameras_fixed_objects_big", ["LM_BIG"])(
    lambda r: [graph(r, spread(r, 700, 6, 6, miss=0.0), np.zeros(6), np.ones(6))])
# mixed batches: a batch runs on ONE kernel
_c("mixed_frame16", ["FRAME16", "FRAME16"])(lambda r: [frame(r, [20] * 12), frame(r, [300, 20, 20, 20, 20])])
_c("mixed_tracking_and_frame", ["LM", "LM"])(lambda r: [tracking(r, [15] * 4), frame(r, [25] * 4)])
_c("mixed_tracking_50_1100", ["CAM", "CAM"], TRACKING_ITS, True)(lambda r: [tracking(r, [10] * 5), tracking(r, [138] * 7 + [134])])
_c("mixed_two_global_600", ["LM_BIG", "LM_BIG"])(lambda r: [global_graph(r, 600, 10, 6), global_graph(r, 600, 12, 5)])
_c("mixed_frame_phasewise_tracking", ["FRAME2", "PHASEWISE", "CAM2"])(
    lambda r: [frame(r, [20] * 6), global_graph(r, 400, 4, 20), tracking(r, [12] * 5)])
# the LM route's LDS layouts: everything resident, partially resident, with and without the Jacobian stage (> 384 edges)
_c("lds_40", ["LM"])(lambda r: [global_graph(r, 40, 3, 2, miss=0.0)])
_c("lds_120_few_pairs", ["LM"])(lambda r: [global_graph(r, 120, 3, 3, miss=0.0)])
_c("lds_160_many_pairs", ["LM"])(lambda r: [global_graph(r, 160, 12, 8, miss=0.3)])
_c("lds_300_many_pairs", ["LM"])(lambda r: [global_graph(r, 300, 30, 10, miss=0.2)])
_c("lds_384", ["LM"])(lambda r: [global_graph(r, 384, 16, 8)])
_c("lds_385", ["LM"])(lambda r: [global_graph(r, 385, 16, 8)])
_c("lds_511_many_pairs", ["LM"])(lambda r: [global_graph(r, 511, 40, 12, miss=0.1)])
# LM_BIG graphs that ask for several times the LDS cap
_c("lds_big_two_global", ["LM_BIG", "LM_BIG"])(lambda r: [global_graph(r, 1600, 40, 8), global_graph(r, 1400, 35, 10)])
_c("lds_big_free_cameras_fixed_objects", ["LM_BIG"])(
    lambda r: [graph(r, spread(r, 2000, 40, 8, miss=0.0), np.zeros(40), np.ones(8))])
# degenerate blocks: a free camera seen through one / two keypoints (H_cc of rank 2 / 4 before lambda); a free object whose every edge is a gross outlier
_c("degenerate_weak_camera_1kp_lm", ["LM"])(lambda r: [with_weak_camera(r, global_graph(r, 300, 6, 5), 1)])
_c("degenerate_weak_camera_2kp_lm", ["LM"])(lambda r: [with_weak_camera(r, global_graph(r, 300, 6, 5), 2)])
_c("degenerate_weak_camera_2kp_phases", ["PHASES"])(lambda r: [with_weak_camera(r, global_graph(r, 700, 10, 6), 2)])
_c("degenerate_outlier_object_lm", ["LM"])(
    lambda r: [graph(r, spread(r, 300, 6, 5, miss=0.0), np.r_[1, np.zeros(5)], np.zeros(5), gross_objects=(3,))])
_c("degenerate_outlier_object_phases", ["PHASES"])(
    lambda r: [graph(r, spread(r, 700, 10, 6, miss=0.0), np.r_[1, np.zeros(9)], np.zeros(6), gross_objects=(2,))])

CASE_IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}


def routes_of(problems, its=None, init_with_outliers=False):
    """(route names, lds_need) suo_debug_lm_routes reports for these graphs as ONE batch."""
    import ctypes as C

    from suo_slam_amd import _lib, ba
    lib = _lib.lib()
    kw = {} if its is None else {"its": its}
    probs = [ba.Problem(*[P[k] for k in KEYS], init_with_outliers=init_with_outliers, **kw) for P in problems]
    arr = (_lib.BaProblem * len(probs))()
    for s, p in zip(arr, probs):
        p._fill(s)
    route = np.zeros(len(probs), np.int32)
    need = np.zeros(len(probs), np.int32)
    _lib.check(lib.suo_debug_lm_routes(C.cast(arr, C.c_void_p), len(probs), route.ctypes.data, need.ctypes.data), "suo_debug_lm_routes")
    names = {v: k for k, v in route_codes().items()}
    return [names.get(int(x), f"?{int(x)}") for x in route], need.tolist()
