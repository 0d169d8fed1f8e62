"""Numpy yardsticks of the BOP-19 VSD row (N6); a helper, not a test.

    render_depth          the depth rasteriser, written in fp64 from the rules of include/suo_hip.h (suo_render_depth), not from the kernel
    vsd_from_depth        pose_error.vsd written from the toolkit's text (pose_error.py:40-93, misc.py:130-163, visibility.py:9-75)
    RefVsdErrors          stands in for bop_eval.BopErrors under a Bop19Meter (numpy MSSD / MSPD of tests/bop_errors_ref.py + the two above)
    add_depth             adds depth PNGs to a synthetic tree of tests/bop_tree.py (which is called unchanged by the caller)
    box_mesh / icosphere / soup   the small meshes of the tests
"""
import json
import os

import numpy as np

NEAR = 1e-9                     # an edge function within NEAR * |doubled area| of zero: the sample's coverage is not compared


# ---- rasteriser ----------------------------------------------------------------------------------------
def project(points, T, K):
    """Camera-space Z and screen (u, v) of float32 points under T [3,4] and K [3,3], each row ((r0 x + r1 y) + r2 z) + t in fp64."""
    P = np.asarray(points, np.float32).astype(np.float64)
    T = np.asarray(T, np.float64).reshape(-1, 4)[:3]
    K = np.asarray(K, np.float64).reshape(3, 3)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    X = ((T[0, 0] * x + T[0, 1] * y) + T[0, 2] * z) + T[0, 3]
    Y = ((T[1, 0] * x + T[1, 1] * y) + T[1, 2] * z) + T[1, 3]
    Z = ((T[2, 0] * x + T[2, 1] * y) + T[2, 2] * z) + T[2, 3]
    with np.errstate(all="ignore"):
        u = K[0, 0] * (X / Z) + K[0, 2]
        v = K[1, 1] * (Y / Z) + K[1, 2]
    return u, v, Z


def _top_left(s, dx, dy):
    nx, ny = s * -dy, s * dx
    return nx > 0.0 or (nx == 0.0 and ny > 0.0)


def render_depth(points, faces, T, K, width, height, with_near=False):
    """float32 [height,width] depth, 0 where nothing is drawn.  ``with_near``: also the bool mask of the samples at which an edge function of a triangle
    whose pixel box holds them lies within NEAR (relative to the triangle's doubled area) of zero."""
    u, v, Z = project(points, T, K)
    depth = np.full((height, width), np.inf, np.float32)
    near = np.zeros((height, width), bool)
    for a, b, c in np.asarray(faces, np.int64).reshape(-1, 3):
        if not (Z[a] > 0 and Z[b] > 0 and Z[c] > 0):
            continue                                           # the stated deviation: no near-plane clipping, the triangle is skipped whole
        u0, v0, u1, v1, u2, v2 = u[a], v[a], u[b], v[b], u[c], v[c]
        area2 = (u1 - u0) * (v2 - v0) - (v1 - v0) * (u2 - u0)
        if not np.isfinite(area2) or area2 == 0.0:
            continue
        s = -1.0 if area2 < 0 else 1.0
        A = s * area2
        x0, x1 = max(np.ceil(min(u0, u1, u2) - 0.5), 0.0), min(np.floor(max(u0, u1, u2) - 0.5), width - 1.0)
        y0, y1 = max(np.ceil(min(v0, v1, v2) - 0.5), 0.0), min(np.floor(max(v0, v1, v2) - 0.5), height - 1.0)
        if x0 > x1 or y0 > y1:
            continue
        x0, x1, y0, y1 = int(x0), int(x1), int(y0), int(y1)
        px = (np.arange(x0, x1 + 1, dtype=np.float64) + 0.5)[None, :]
        py = (np.arange(y0, y1 + 1, dtype=np.float64) + 0.5)[:, None]
        w0 = s * ((u2 - u1) * (py - v1) - (v2 - v1) * (px - u1))
        w1 = s * ((u0 - u2) * (py - v2) - (v0 - v2) * (px - u2))
        w2 = s * ((u1 - u0) * (py - v0) - (v1 - v0) * (px - u0))
        cov = np.ones(w0.shape, bool)
        for w, tl in ((w0, _top_left(s, u2 - u1, v2 - v1)), (w1, _top_left(s, u0 - u2, v0 - v2)), (w2, _top_left(s, u1 - u0, v1 - v0))):
            cov &= (w > 0.0) | ((w == 0.0) & tl)
            if with_near:
                near[y0:y1 + 1, x0:x1 + 1] |= np.abs(w) <= NEAR * A
        iz = ((w0 * (1.0 / Z[a]) + w1 * (1.0 / Z[b])) + w2 * (1.0 / Z[c])) / A
        with np.errstate(all="ignore"):
            z = (1.0 / iz).astype(np.float32)
        tile = depth[y0:y1 + 1, x0:x1 + 1]
        tile[cov] = np.minimum(tile[cov], z[cov])
    depth[np.isinf(depth)] = 0.0
    return (depth, near) if with_near else depth


# ---- VSD -----------------------------------------------------------------------------------------------
def _dist_im(depth_im, K):
    xs, ys = np.meshgrid(np.arange(depth_im.shape[1]), np.arange(depth_im.shape[0]))
    pre_Xs = (xs - K[0, 2]) / np.float64(K[0, 0])
    pre_Ys = (ys - K[1, 2]) / np.float64(K[1, 1])
    return np.sqrt(np.multiply(pre_Xs, depth_im) ** 2 + np.multiply(pre_Ys, depth_im) ** 2 + depth_im.astype(np.float64) ** 2)


def _visib(d_test, d_model, delta):
    d_diff = d_model.astype(np.float32) - d_test.astype(np.float32)
    return np.logical_and(np.logical_or(d_diff <= delta, d_test == 0), d_model > 0)


def vsd_from_depth(depth_est, depth_gt, depth_test, K, delta, taus, normalized_by_diameter, diameter):
    """``(errors [len(taus)], counts [2 + len(taus)]: union, intersection, cost per tau)`` of one pair of float32 depth images."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    dist_test, dist_gt, dist_est = _dist_im(depth_test, K), _dist_im(depth_gt, K), _dist_im(depth_est, K)
    visib_gt = _visib(dist_test, dist_gt, delta)
    visib_est = np.logical_or(_visib(dist_test, dist_est, delta), np.logical_and(visib_gt, dist_est > 0))
    visib_inter = np.logical_and(visib_gt, visib_est)
    visib_union = np.logical_or(visib_gt, visib_est)
    union, inter = int(visib_union.sum()), int(visib_inter.sum())
    dists = np.abs(dist_gt[visib_inter] - dist_est[visib_inter])
    if normalized_by_diameter:
        dists /= diameter
    costs = [int(np.sum(dists >= tau)) for tau in taus]
    errors = [1.0] * len(taus) if union == 0 else [(c + (union - inter)) / float(union) for c in costs]
    return errors, [union, inter] + costs


def decision_margins(depth_est, depth_gt, depth_test, K, delta, taus, normalized_by_diameter, diameter):
    """How far the pair's pixels are from deciding otherwise: ``(min |float32 difference - delta| over the pixels with a model distance, in mm,
    min |dists - tau| over the intersection and the taus)`` -- the recorded fixtures must keep both well away from zero."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    dist_test, dist_gt, dist_est = _dist_im(depth_test, K), _dist_im(depth_gt, K), _dist_im(depth_est, K)
    m_delta = np.inf
    for d in (dist_gt, dist_est):
        sel = (d > 0) & (dist_test != 0)
        if sel.any():
            m_delta = min(m_delta, float(np.abs((d.astype(np.float32) - dist_test.astype(np.float32))[sel].astype(np.float64) - delta).min()))
    visib_gt = _visib(dist_test, dist_gt, delta)
    visib_est = np.logical_or(_visib(dist_test, dist_est, delta), np.logical_and(visib_gt, dist_est > 0))
    inter = visib_gt & visib_est
    dists = np.abs(dist_gt[inter] - dist_est[inter])
    if normalized_by_diameter:
        dists = dists / diameter
    m_tau = float(np.abs(dists[:, None] - np.asarray(taus)[None, :]).min()) if dists.size else np.inf
    return m_delta, m_tau


class RefVsdErrors:
    """The numpy counterpart of bop_eval.BopErrors for a Bop19Meter: MSSD / MSPD of tests/bop_errors_ref.py, VSD of this module."""

    def __init__(self, mesh_db, models_info, max_sym_disc_step=0.01):
        from tests import bop_errors_ref
        self._ref = bop_errors_ref.RefErrors(mesh_db, models_info, max_sym_disc_step)
        self.mesh_db, self.models_info, self.max_sym_disc_step = mesh_db, models_info, max_sym_disc_step

    def errors(self, *a, **k):
        return self._ref.errors(*a, **k)

    def vsd(self, obj_ids, T_est, T_gt, K, depth_images, image_index, delta=15, taus=None, normalized=True):
        out, cache = [], {}

        def ren(o, T, Kk, hw):
            key = (int(o), np.asarray(T, np.float64).tobytes(), np.asarray(Kk, np.float64).tobytes())
            if key not in cache:
                cache[key] = render_depth(self.mesh_db[int(o)]["points"], self.mesh_db[int(o)]["faces"], T, Kk, hw[1], hw[0])
            return cache[key]
        for o, Te, Tg, Kk, ii in zip(obj_ids, T_est, T_gt, K, image_index):
            test = np.asarray(depth_images[ii], np.float32)
            out.append(vsd_from_depth(ren(o, Te, Kk, test.shape), ren(o, Tg, Kk, test.shape), test, Kk, delta, taus, normalized,
                                      float(self.models_info[int(o)]["diameter"]))[0])
        return np.array(out, np.float64).reshape(len(out), len(taus))


# ---- the synthetic tree with depth ------------------------------------------------------------------------
def add_depth(desc, mesh_db, seed=0):
    """Writes ``depth/%06d.png`` (16-bit, depth_scale of scene_camera.json) for every image of the tree ``desc`` describes: the ground truths drawn by
    render_depth, a background plane behind them, an occluding slab in front of part of the image and a rectangle of missing depth (zeros)."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    split_dir = os.path.join(desc["data_root"], desc["split"])
    for scene in sorted(os.listdir(split_dir)):
        sdir = os.path.join(split_dir, scene)
        cam = json.load(open(os.path.join(sdir, "scene_camera.json")))
        gt = json.load(open(os.path.join(sdir, "scene_gt.json")))
        os.makedirs(os.path.join(sdir, "depth"), exist_ok=True)
        for view, gts in gt.items():
            W, H = Image.open(os.path.join(sdir, "rgb", f"{int(view):06d}.png")).size
            K = np.array(cam[view]["cam_K"], np.float64).reshape(3, 3)
            depth = np.full((H, W), 1500.0, np.float32)
            for g in gts:
                T = np.hstack((np.reshape(g["cam_R_m2c"], (3, 3)), np.reshape(g["cam_t_m2c"], (3, 1))))
                d = render_depth(mesh_db[g["obj_id"]]["points"], mesh_db[g["obj_id"]]["faces"], T, K, W, H)
                depth = np.where((d > 0) & (d < depth), d, depth)
            x, y = int(rng.integers(0, W - 80)), int(rng.integers(0, H - 60))
            depth[y:y + 60, x:x + 80] = 420.0                                 # the slab: nearer than any object
            x, y = int(rng.integers(0, W - 50)), int(rng.integers(0, H - 40))
            depth[y:y + 40, x:x + 50] = 0.0                                   # missing depth
            raw = np.round(depth / np.float32(cam[view]["depth_scale"])).astype(np.uint16)
            Image.fromarray(raw).save(os.path.join(sdir, "depth", f"{int(view):06d}.png"))


# ---- small meshes ----------------------------------------------------------------------------------------
def box_mesh(ext=(40.0, 30.0, 20.0)):
    """12 faces, mixed windings."""
    e = np.asarray(ext, np.float32)
    pts = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float32) * e
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = []
    for k, (a, b, c, d) in enumerate(quads):
        faces += [(a, b, c), (a, c, d)] if k % 2 == 0 else [(a, c, b), (a, d, c)]
    return pts, np.array(faces, np.int32)


def icosphere(radius=35.0, subdivisions=2):
    """20 * 4^subdivisions faces (320 at 2)."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6),
         (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius).astype(np.float32), np.array(f, np.int32)


def soup(n_faces=200, ext=45.0, seed=3):
    """Random triangles with both windings; small ones, so that many lanes walk their own."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-ext, ext, (n_faces, 1, 3))
    pts = (centres + rng.uniform(-12, 12, (n_faces, 3, 3))).reshape(-1, 3).astype(np.float32)
    return pts, np.arange(n_faces * 3, dtype=np.int32).reshape(n_faces, 3)
