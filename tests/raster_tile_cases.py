"""Seeded inputs for the structural edges of the rasteriser's tile pass (csrc/raster_tile.h), and a census of the route every triangle takes; a helper,
not a test.  Nothing is recorded in a file: tests/test_raster_tile_cases.py (no GPU) asserts on the numpy rasteriser alone that these inputs reach what
they were designed to reach, tests/test_gpu_raster_tile_edges.py asks the device.

The rule the census restates, from the comment of draw_tile: a render's triangles are scanned CHUNK = 256 at a time, triangle f in chunk f // 256 on lane
f % 256.  The pixel box of a triangle holds the pixels whose sample (x + 0.5, y + 0.5) lies within the bounding box of its three screen vertices, clipped
to the image; a triangle that draws nothing (a vertex at Z <= 0, no area, an empty box) has none.  Per 64 x 64 tile the lane walks the samples of box ∩
tile itself when they are at most SMALL = 32, and appends the triangle to the tile's list (one per lane, 256 entries) when they are more.

Meshes: ico3 (1280 faces, 5 chunks), shingles (700 large independent triangles, 3 chunks), full_list (600 triangles that all land on the list of the one
tile they are drawn in: 256, 256 and 88 in its three chunks), threshold_rects (rectangles on integer screen coordinates with box ∩ tile of exactly 32
and 33 samples), the 12-face box."""
import functools

import numpy as np

from tests import vsd_ref as VR
from tests.golden import bop19_cases as BC

TILE, CHUNK, SMALL = 64, 256, 32
SIZES = [(1, 1), (3, 2), (5, 64), (63, 65), (64, 64), (65, 63), (67, 70), (97, 130), (131, 67), (161, 99)]      # (W, H)
CHUNK_SIZES = [(160, 96), (131, 67), (161, 99)]          # where the many-chunk meshes are drawn: the 16-byte stores, W = 4 k + 3, W = 4 k + 1
ODD = (131, 67)                                          # the size of the order, mask and VSD cases
GT_SIZE = (67, 70)                                       # scene_gt_info: a canvas of 201 x 210
N_SHINGLES, N_FULL = 700, 600
DELTA = 15
DEPTH_SCALE = 0.1
BACKGROUND = 900.0


# ---- meshes ------------------------------------------------------------------------------------------------
def ico3():
    return VR.icosphere(35.0, 3)


def shingles(n=N_SHINGLES, seed=7):
    """``n`` independent triangles (three vertices each, either winding) of some 90 mm across, their centres scattered over 300 x 180 x 80 mm."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-1.0, 1.0, (n, 1, 3)) * np.array([150.0, 90.0, 40.0])
    pts = centres + rng.uniform(-1.0, 1.0, (n, 3, 3)) * np.array([45.0, 45.0, 10.0])
    return pts.reshape(-1, 3).astype(np.float32), np.arange(3 * n, dtype=np.int32).reshape(n, 3)


FULL_K = np.array([[150.0, 0.0, 32.3], [0.0, 150.0, 31.8], [0.0, 0.0, 1.0]])
FULL_T = np.hstack((np.eye(3), [[0.0], [0.0], [400.0]]))


def full_list(n=N_FULL, seed=9):
    """``n`` equilateral triangles facing the camera of FULL_K / FULL_T, one per plane z = 0.25 i mm.  On the screen triangle i has a circumradius of
    8 to 22 pixels about a centre within 3 pixels of (32.3, 31.8), at any rotation: its bounding box is at least 1.5 x 8 = 12 pixels wide and high (at
    least 11 x 11 = 121 samples) and stays within 3 + 22 = 25 pixels of the centre, inside the tile [0, 64)^2."""
    rng = np.random.default_rng(seed)
    pts = np.zeros((n, 3, 3))
    for i in range(n):
        z = 0.25 * i
        px_to_mm = (FULL_T[2, 3] + z) / FULL_K[0, 0]
        R, phi, c = rng.uniform(8.0, 22.0), rng.uniform(0.0, 2.0 * np.pi), rng.uniform(-3.0, 3.0, 2)
        ang = phi + np.array([0.0, 2.0, 4.0] if i % 2 == 0 else [0.0, 4.0, 2.0]) * np.pi / 3.0
        pts[i, :, 0] = (c[0] + R * np.cos(ang)) * px_to_mm
        pts[i, :, 1] = (c[1] + R * np.sin(ang)) * px_to_mm
        pts[i, :, 2] = z
    return pts.reshape(-1, 3).astype(np.float32), np.arange(3 * n, dtype=np.int32).reshape(n, 3)


RECT_K = np.array([[64.0, 0.0, 64.0], [0.0, 64.0, 32.0], [0.0, 0.0, 1.0]])
RECT_T = np.hstack((np.eye(3), np.zeros((3, 1))))
RECT_SIZES = [(128, 64), (130, 66)]
# (x0, y0, x1, y1, Z): the rectangle [x0, x1] x [y0, y1] of the screen covers the pixels x0 .. x1 - 1, y0 .. y1 - 1
RECTS = [(10, 5, 18, 9, 2.0),          # 8 x 4 = 32 samples in tile (0, 0): the largest box a lane walks
         (30, 20, 41, 23, 4.0),        # 11 x 3 = 33: the smallest on the list; a sample lies on its diagonal (top-left rule between its two triangles)
         (14, 7, 22, 11, 4.0),         # 8 x 4 behind the first: the two overlap
         (60, 30, 69, 38, 8.0),        # across x = 64: 4 x 8 = 32 in the left tile, 5 x 8 = 40 in the right
         (120, 58, 131, 67, 2.0),      # across x = 128 and y = 64, past both sizes' borders: 8 x 6 = 48 | 2 x 6 | 8 x 2 | 2 x 2 at 130 x 66
         (70, 40, 103, 41, 8.0)]       # one row of 33 samples


def threshold_rects():
    """Axis-aligned rectangles of two triangles (one of either winding) whose vertices have integer screen coordinates under RECT_K / RECT_T: x / Z and
    y / Z are multiples of 1 / 64 at Z in {2, 4, 8}, so every edge function and every depth is an integer computed without rounding."""
    pts, faces = [], []
    for x0, y0, x1, y1, Z in RECTS:
        b = len(pts)
        pts += [[(x - RECT_K[0, 2]) / 64.0 * Z, (y - RECT_K[1, 2]) / 64.0 * Z, Z] for x, y in ((x0, y0), (x1, y0), (x1, y1), (x0, y1))]
        faces += [(b, b + 1, b + 2), (b, b + 3, b + 2)]
    return np.array(pts, np.float32), np.array(faces, np.int32)


@functools.lru_cache(maxsize=None)
def meshes():
    return {"ico3": ico3(), "shingles": shingles(), "full_list": full_list(), "box": VR.box_mesh(), "threshold_rects": threshold_rects()}


# ---- cameras and poses ---------------------------------------------------------------------------------------
def camera(w, h, f=150.0):
    """The principal point a fraction of a pixel off the image centre."""
    return np.array([[f, 0.0, w / 2.0 + 0.13], [0.0, f, h / 2.0 - 0.21], [0.0, 0.0, 1.0]])


def _pose(rng, z, rot=None):
    R = BC.random_rotation(rng) if rot is None else BC.rotvec(rng.standard_normal(3) * rot)
    return np.hstack((R, [[0.0], [0.0], [z]]))


def perturbed(T, seed, rot=0.03, trans=(3.0, 3.0, 8.0)):
    """An estimate: ``T`` times a small motion."""
    rng = np.random.default_rng(seed)
    return BC.compose(T, np.hstack((BC.rotvec(rng.standard_normal(3) * rot), rng.standard_normal((3, 1)) * np.array(trans)[:, None])))


@functools.lru_cache(maxsize=None)
def render_cases():
    """``{label: (mesh name, T [3,4], K [3,3], w, h)}`` of every render that is compared with the numpy rasteriser.
    chunks/*   the many-chunk meshes at CHUNK_SIZES (full_list also at the 64 x 64 of its census): ico3 near (triangles of ~50 samples: the list) and far
               (~3 samples: the lanes), the shingles facing the camera, full_list under its own camera
    sizes/*    the box and ico3 close up at every size of SIZES, the focal length grown with the image so that they overflow it
    est/*      the estimates of the mask pairs (their ground truths are chunks/ico3_near and chunks/shingles)"""
    rng = np.random.default_rng(101)
    out = {}
    T_near, T_far, T_sh = _pose(rng, 120.0), _pose(rng, 330.0), _pose(rng, 300.0, rot=0.15)
    for w, h in CHUNK_SIZES + [(64, 64)]:
        K = camera(w, h)
        if (w, h) != (64, 64):
            out[f"chunks/ico3_near@{w}x{h}"] = ("ico3", T_near, K, w, h)
            out[f"chunks/ico3_far@{w}x{h}"] = ("ico3", T_far, K, w, h)
            out[f"chunks/shingles@{w}x{h}"] = ("shingles", T_sh, K, w, h)
        out[f"chunks/full_list@{w}x{h}"] = ("full_list", FULL_T, FULL_K, w, h)
    for w, h in SIZES:
        K = camera(w, h, max(150.0, 1.9 * max(w, h)))
        out[f"sizes/box@{w}x{h}"] = ("box", _pose(rng, 95.0), K, w, h)
        out[f"sizes/ico3@{w}x{h}"] = ("ico3", _pose(rng, 95.0), K, w, h)
    for w, h in (ODD, (160, 96)):
        for k, name in enumerate(("ico3_near", "shingles")):
            mesh, T, K, _, _ = out[f"chunks/{name}@{w}x{h}"]
            out[f"est/{name}@{w}x{h}"] = (mesh, perturbed(T, 200 + k), K, w, h)
    return out


@functools.lru_cache(maxsize=None)
def reference(label):
    """``(depth float32 [h,w], near bool [h,w])`` of a render case by the numpy rasteriser, computed once per process; the arrays are read-only."""
    mesh, T, K, w, h = render_cases()[label]
    P, F = meshes()[mesh]
    depth, near = VR.render_depth(P, F, T, K, w, h, with_near=True)
    depth.setflags(write=False)
    near.setflags(write=False)
    return depth, near


def mask_pairs():
    """``[(label, mesh name, T_est, T_gt, K, w, h, label of the estimate's render, label of the ground truth's)]``."""
    rc = render_cases()
    out = []
    for w, h in (ODD, (160, 96)):
        for name in ("ico3_near", "shingles"):
            e, g = f"est/{name}@{w}x{h}", f"chunks/{name}@{w}x{h}"
            out.append((f"{name}@{w}x{h}", rc[g][0], rc[e][1], rc[g][1], rc[g][2], w, h, e, g))
    return out


def vsd_pairs():
    """Two shingles pairs at the odd width: ``(pairs [(T_est, T_gt, K)], test depth float32 [2,h,w])``; the test image is the ground truth's render over a
    background with a slab in front of part of it and a rectangle of missing depth."""
    rc = render_cases()
    w, h = ODD
    _, Tg, K, _, _ = rc[f"chunks/shingles@{w}x{h}"]
    pairs = [(rc[f"est/shingles@{w}x{h}"][1], Tg, K), (perturbed(Tg, 311, rot=0.2, trans=(15.0, 15.0, 40.0)), Tg, K)]
    d = reference(f"chunks/shingles@{w}x{h}")[0]
    test = np.where(d > 0, d, np.float32(BACKGROUND)).astype(np.float32)
    test[:, 40:60] = 180.0
    test[20:40, 80:110] = 0.0
    return pairs, np.stack([test, np.where(d > 0, d, np.float32(BACKGROUND)).astype(np.float32)])


@functools.lru_cache(maxsize=None)
def gt_cases():
    """``[(label, mesh name, T, K, test depth float32 [h,w])]`` at GT_SIZE: the object overflows the image into the canvas; the test image is what a 16-bit
    PNG with depth_scale 0.1 holds, the object over a background, with a slab in front of some columns and a rectangle of missing depth."""
    rng = np.random.default_rng(151)
    w, h = GT_SIZE
    K = camera(w, h)
    out = []
    for name, T in (("ico3", _pose(rng, 120.0)), ("shingles", _pose(rng, 300.0, rot=0.15))):
        P, F = meshes()[name]
        d = VR.render_depth(P, F, T, K, w, h)
        depth = np.where(d > 0, d, np.float32(BACKGROUND)).astype(np.float32)
        raw = np.round(depth / np.float32(DEPTH_SCALE)).astype(np.uint16)
        raw[:, 20:30] = 600                                                    # 60 mm: nearer than either object
        raw[40:55, 35:60] = 0
        test = raw.astype(np.float32) * np.float32(DEPTH_SCALE)
        test.setflags(write=False)
        out.append((name, name, T, K, test))
    return out


# ---- the census ------------------------------------------------------------------------------------------------
def pixel_boxes(points, faces, T, K, w, h):
    """int64 [F,4] x0, y0, x1, y1 of every triangle's pixel box, x0 > x1 where it draws nothing."""
    u, v, Z = VR.project(points, T, K)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    out = np.tile(np.array([1, 1, 0, 0], np.int64), (len(F), 1))
    for i, (a, b, c) in enumerate(F):
        if not (Z[a] > 0 and Z[b] > 0 and Z[c] > 0):
            continue
        area2 = (u[b] - u[a]) * (v[c] - v[a]) - (v[b] - v[a]) * (u[c] - u[a])
        if not np.isfinite(area2) or area2 == 0.0:
            continue
        x0, x1 = max(np.ceil(min(u[a], u[b], u[c]) - 0.5), 0.0), min(np.floor(max(u[a], u[b], u[c]) - 0.5), w - 1.0)
        y0, y1 = max(np.ceil(min(v[a], v[b], v[c]) - 0.5), 0.0), min(np.floor(max(v[a], v[b], v[c]) - 0.5), h - 1.0)
        if x0 <= x1 and y0 <= y1:
            out[i] = (x0, y0, x1, y1)
    return out


def census(points, faces, T, K, w, h):
    """``{"list": int [tiles, chunks], "lane": int [tiles, chunks], "both": int, "samples": int [F, tiles]}``: per (tile, chunk) the triangles on the
    tile's list and those a lane walks, the number of triangles that take the list in one tile and a lane in another, and the samples of box ∩ tile.  Tiles
    are numbered row by row."""
    box = pixel_boxes(points, faces, T, K, w, h)
    tx, ty = (w + TILE - 1) // TILE, (h + TILE - 1) // TILE
    nf = len(box)
    samples = np.zeros((nf, tx * ty), np.int64)
    for t in range(tx * ty):
        X0, Y0 = (t % tx) * TILE, (t // tx) * TILE
        X1, Y1 = min(X0 + TILE, w) - 1, min(Y0 + TILE, h) - 1
        nx = np.minimum(box[:, 2], X1) - np.maximum(box[:, 0], X0) + 1
        ny = np.minimum(box[:, 3], Y1) - np.maximum(box[:, 1], Y0) + 1
        samples[:, t] = np.where((nx > 0) & (ny > 0), nx * ny, 0)
    chunks = (nf + CHUNK - 1) // CHUNK
    on_list, on_lane = samples > SMALL, (samples > 0) & (samples <= SMALL)
    chunk_of = np.arange(nf) // CHUNK
    lst, lane = np.zeros((tx * ty, chunks), np.int64), np.zeros((tx * ty, chunks), np.int64)
    for c in range(chunks):
        lst[:, c] = on_list[chunk_of == c].sum(0)
        lane[:, c] = on_lane[chunk_of == c].sum(0)
    return {"list": lst, "lane": lane, "both": int((on_list.any(1) & on_lane.any(1)).sum()), "samples": samples}


def case_census(label):
    mesh, T, K, w, h = render_cases()[label]
    return census(*meshes()[mesh], T, K, w, h)
