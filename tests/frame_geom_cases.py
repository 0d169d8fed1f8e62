"""Designed inputs of the frame chain (csrc/frame_geom.hip) for tests/test_frame_geom_ref.py (CPU: every case takes the branch it was built for) and
tests/test_gpu_frame_geom_edges.py.  A frame is a dict of what suo_frame_geom_launch takes for its crops: uv [L,41,2] f32, cov [L,41,2,2] f32, mask [L,41] uint8,
kps [L,41,3] f32, K_bbox [L,3,3] f32, min_depth [L] f64 -- synthetic.make_frame frames with masks, covariances and diameters overwritten (model_kps is defined for
all 41 slots, so any mask is legal)."""
from __future__ import annotations

import numpy as np

from suo_slam_amd import synthetic as S
from suo_slam_amd.geometry import project_ndc

NUM_KP = 41


def frame(seed, n_obj, drop=0.25, full=False):
    """A synthetic frame with random drop-outs on the class masks; full: all 41 keypoints of every crop."""
    rng = np.random.default_rng(seed)
    fr = S.make_frame(rng, n_obj, noise=0.004, outlier_frac=0.08, with_image=False)
    mask = np.ones((n_obj, NUM_KP), np.uint8) if full else (fr["model_kps_masks"] & (rng.random((n_obj, NUM_KP)) >= drop)).astype(np.uint8)
    return {"uv": fr["uv"].copy(), "cov": fr["cov"].copy(), "mask": mask, "kps": fr["model_kps"].copy(), "K_bbox": fr["K_bbox"].astype(np.float32),
            "min_depth": 0.5 * fr["diameter"], "T_gt": fr["T_OtoC"].copy()}


def copy(f):
    return {k: v.copy() for k, v in f.items()}


def exact_uv(f, crop):
    """The crop's measurements replaced by the float32-rounded projections of its ground-truth pose: PnP cannot fail on them for lack of inliers."""
    uv, _ = project_ndc(f["K_bbox"][crop].astype(np.float64), f["T_gt"][crop], f["kps"][crop].astype(np.float64))
    f["uv"][crop] = uv.astype(np.float32)
    return f


# ---- masks -----------------------------------------------------------------------------------------------------------------------------------------------------
MASK_ROWS = ("count 0", "count 1", "count 3", "count 4", "count 5", "count 40", "count 41", "only slot 0", "only slot 40", "every second", "middle block", "bytes 2 / 255")
MASK_COUNTS = (0, 1, 3, 4, 5, 40, 41, 1, 1, 21, 11, 41)


def mask_frame(seed=21):
    """12 crops, one per row of MASK_ROWS."""
    f = frame(seed, len(MASK_ROWS))
    rng = np.random.default_rng(seed + 1)
    m = np.zeros((len(MASK_ROWS), NUM_KP), np.uint8)
    for row, cnt in ((1, 1), (2, 3), (3, 4), (4, 5)):
        m[row, np.sort(rng.choice(NUM_KP, cnt, replace=False))] = 1
    m[5] = 1; m[5, 13] = 0
    m[6] = 1
    m[7, 0] = 1
    m[8, 40] = 1
    m[9, ::2] = 1
    m[10, 15:26] = 1
    m[11, ::2] = 2; m[11, 1::2] = 255
    f["mask"] = m
    for crop in (3, 4):
        exact_uv(f, crop)
    return f


# ---- frame shapes ----------------------------------------------------------------------------------------------------------------------------------------------
def shape_frames():
    """name -> list of frames of one launch."""
    return {"1": [frame(31, 1)], "8": [frame(38, 8)], "9": [frame(39, 9)], "16": [frame(46, 16)], "16 x 41": [frame(47, 16, full=True)],
            "[0, 3, 3, 8]": [frame(51, 3), frame(52, 0), frame(53, 5)]}


# ---- covariances -----------------------------------------------------------------------------------------------------------------------------------------------
def _f32(M):
    return np.array(M, np.float32).reshape(2, 2)


def regular_covs():
    b = np.float32(7e-6)
    c, s = np.cos(0.5), np.sin(0.5)
    R = np.array([[c, -s], [s, c]])
    sym = _f32([[2e-5, 5e-6], [5e-6, 1e-5]])
    return {"symmetric": sym, "asymmetric": _f32([[2e-5, 8e-6], [2e-6, 1e-5]]), "b ~ -c": _f32([[2e-5, b], [-np.nextafter(b, np.float32(1)), 1e-5]]),
            "scaled 1e-12": _f32(sym.astype(np.float64) * 1e-12), "scaled 1e6": _f32(sym.astype(np.float64) * 1e6),
            "condition 1e6": _f32(1e-4 * R @ np.diag([1.0, 1e-6]) @ R.T)}


def degenerate_covs():
    q = 3e-5
    return {"zero": _f32([[0, 0], [0, 0]]), "rank one": _f32([[q, q], [q, q]]), "det < 0": _f32([[1e-5, 2e-5], [2e-5, 1e-5]]),
            "NaN": _f32([[np.nan, 0], [0, 1e-5]]), "inf": _f32([[np.inf, 0], [0, 1e-5]])}


def cov_frame(seed=39):
    """The 9-object frame with one keypoint of crop j carrying the j-th regular covariance; returns (frame, {name: (crop, slot)})."""
    f = frame(seed, 9)
    where = {}
    for j, (name, M) in enumerate(regular_covs().items()):
        slot = int(np.nonzero(f["mask"][j])[0][2])
        f["cov"][j, slot] = M
        where[name] = (j, slot)
    return f, where


def singular_frames(seed=39, crop=4):
    """name -> (frame with the degenerate matrix on one counted keypoint of `crop`, the same frame with that keypoint masked off by hand, crop, slot)."""
    out = {}
    for name, M in degenerate_covs().items():
        f = frame(seed, 9)
        slot = int(np.nonzero(f["mask"][crop])[0][3])
        f["cov"][crop, slot] = M
        g = copy(f)
        g["mask"][crop, slot] = 0
        out[name] = (f, g, crop, slot)
    return out


def four_to_three_frame(seed=39, crop=2):
    """Crop `crop` keeps 4 keypoints (exact measurements: PnP succeeds on them), one of them with the all-zero covariance."""
    f = frame(seed, 9)
    keep = np.nonzero(f["mask"][crop])[0][:4]
    f["mask"][crop] = 0
    f["mask"][crop, keep] = 1
    exact_uv(f, crop)
    g = copy(f)
    f["cov"][crop, keep[1]] = 0
    return f, g, crop, int(keep[1])


LM_LIMIT_SEEDS = (("16 x 41", 5), ("9", 5))          # (shape case, PnP seed) of the frames that meet the oracle's LM on the device
CHI2_THR = 5.991


def oracle_near_gate(f, st, seed):
    """The frame through the CPU oracle alone -- its PnP with the chain's sampler keys (solvable crop j of the frame: seed + j * SEED_STRIDE), the acceptance rule,
    its LM on the mp information matrices of st = frame_geom_ref.stage(f) -- and the count of edges whose final chi2 lies within 1e-5 thr of the gate.
    Returns (near, n_edge)."""
    from oracle import geometry as G
    from suo_slam_amd.lambdatwist import SEED_STRIDE
    from tests import frame_geom_ref as R
    L = len(f["mask"])
    T, status, j = np.tile(np.eye(4), (L, 1, 1)), np.ones(L, np.int32), 0
    for l in range(L):
        n = int(st["n"][l])
        if n >= 4:
            ys = np.array([[float(y[0]), float(y[1])] for y in st["ys"][l]])
            T[l] = G.pnp(st["xs"][l, :n], ys, 1e-3, seed=(seed + j * SEED_STRIDE) % 2 ** 64)[0]
            status[l] = int(np.array_equal(T[l], np.eye(4)))
            j += 1
    acc = R.accept(st["n"], status, T, f["min_depth"])
    objs = [l for l in range(L) if acc[l]]
    e_obj = np.concatenate([np.full(int(st["n"][l]), i, np.int32) for i, l in enumerate(objs)])
    cat = lambda key: np.concatenate([st[key][l, :st["n"][l]] for l in objs])
    info = np.array([[float(x) for x in st["info"][l][i]] for l in objs for i in range(st["n"][l])])
    res = G.optimize(np.eye(4)[None, :3], np.array([1], np.uint8), T[objs][:, :3], np.zeros(len(objs), np.uint8), np.zeros(len(e_obj), np.int32), e_obj,
                     cat("edge_k"), cat("xs"), cat("edge_uv"), info, np.ones(len(e_obj), np.uint8))
    return int(np.count_nonzero(np.abs(res[3] - CHI2_THR) <= 1e-5 * CHI2_THR)), len(e_obj)


def concat(frames):
    """The launch arguments of a list of frames: frame_first and the concatenated arrays."""
    first = np.concatenate([[0], np.cumsum([len(f["mask"]) for f in frames])]).astype(np.int32)
    cat = {k: np.concatenate([f[k] for f in frames]) for k in ("uv", "cov", "mask", "kps", "K_bbox", "min_depth")}
    return first, cat
