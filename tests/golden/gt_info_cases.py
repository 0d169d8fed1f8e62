"""Seeded inputs of the scene_gt_info goldens and GPU tests (row N7), shared by tests/golden/make_gt_info_golden.py (which runs the REFERENCE's vendored
bop_toolkit scripts on them, build container only) and by the tests (which regenerate them).  Nothing here comes from the toolkit.

Images are 160 x 96, so calc_gt_info.py's canvas is 480 x 288: 8 x 5 tiles of 64 x 64 samples with a partial last row, and the image window starts 2.5
tiles in (x = 160) and 1.5 tiles down (y = 96).  The models are those of tests/golden/vsd_cases.py; object id = model index + 1.  A test depth image is what
a 16-bit PNG with depth_scale 0.1 holds: the objects of the image drawn by the numpy rasteriser over a background, rounded to 0.1 mm."""
import numpy as np

from tests import vsd_ref as VR
from tests.golden import vsd_cases as VC

W, H = VC.W, VC.H
K0 = VC.K0
K1 = np.array([[131.7, 0.0, 77.3], [0.0, 140.2, 51.9], [0.0, 0.0, 1.0]])      # fractional cx, cy and fx != fy
DELTA = 15
DEPTH_SCALE = 0.1
SCENE_ID = 1
W2, H2 = 100, 70                                  # the second size: no multiple of 64, offsets no multiple of 32


def read_raw(raw, depth_scale=DEPTH_SCALE):
    """float32 mm of a 16-bit image, the in-place float32 product of the scripts (and of bop.BopDataset.read_depth)."""
    return np.asarray(raw).astype(np.float32) * np.float32(depth_scale)


def _scene_raw(models, K, instances, background=VC.BACKGROUND, w=W, h=H):
    depth = np.full((h, w), background, np.float32)
    for _, m, T in instances:
        d = VR.render_depth(models[m][1], models[m][2], T, K, w, h)
        depth = np.where((d > 0) & (d < depth), d, depth)
    return np.round(depth / np.float32(DEPTH_SCALE)).astype(np.uint16)


def images(seed=41):
    """``[{"label", "K" [3,3], "instances": [(label, model index, T [3,4])], "raw" uint16 [H,W]}]``, image id = position in the list."""
    rng = np.random.default_rng(seed)
    models = VC.models()
    out = []
    # 0: the poses of vsd_cases.render_cases() under K0, all in one image (they hide parts of one another)
    rc = VC.render_cases()
    inst = [(lab, m, T) for lab, m, T, K in rc if np.array_equal(K, K0)]
    out.append({"label": "render_cases", "K": K0, "instances": inst, "raw": _scene_raw(models, K0, inst)})
    # 1: the second camera
    inst = [(lab, m, T) for lab, m, T, K in rc if not np.array_equal(K, K0)]
    inst.append(("k1_left", 0, VC.pose(rng, (-4.3, 40.2), 340.0, K1)))
    inst.append(("k1_bottom", 1, VC.pose(rng, (90.6, 99.1), 360.0, K1)))
    out.append({"label": "other_K", "K": K1, "instances": inst, "raw": _scene_raw(models, K1, inst)})
    # 2: across each border, inside the canvas but outside the image, outside the canvas, the spike past the canvas
    inst = [("left", 0, VC.pose(rng, (-6.0, 50.0), 330.0)), ("right", 1, VC.pose(rng, (163.0, 40.0), 350.0)), ("top", 2, VC.pose(rng, (80.0, -8.0), 340.0)),
            ("bottom", 3, VC.pose(rng, (70.0, 101.0), 360.0)), ("canvas_only", 1, VC.pose(rng, (250.0, -40.0), 350.0)),
            ("nowhere", 0, VC.pose(rng, (700.0, -450.0), 350.0)), ("spike", 4, VC.pose(rng, (60.0, 40.0), 380.0))]
    out.append({"label": "borders", "K": K0, "instances": inst, "raw": _scene_raw(models, K0, inst)})
    # 3 - 6: three objects in the middle under an occluding slab, a rectangle of missing depth, no depth at all, a wall in front of everything
    mid = [(f"mid{m}", m, VC.pose(rng, (64.0 + 14.0 * m, 50.0 - 6.0 * m), 340.0 + 30.0 * m)) for m in range(3)]
    base = _scene_raw(models, K0, mid)
    slab, holes = base.copy(), base.copy()
    slab[:, 70:110] = 1800                                                     # 180 mm: nearer than any object
    holes[30:70, 50:100] = 0
    out.append({"label": "slab", "K": K0, "instances": mid, "raw": slab})
    out.append({"label": "holes", "K": K0, "instances": mid, "raw": holes})
    out.append({"label": "no_depth", "K": K0, "instances": mid, "raw": np.zeros_like(base)})
    out.append({"label": "wall", "K": K0, "instances": mid, "raw": np.full_like(base, 1500)})
    return out


def images_second_size(seed=43):
    """The same kind of scene at W2 x H2 under K1 (moved towards the smaller image): a slab and a hole in one image."""
    rng = np.random.default_rng(seed)
    models = VC.models()
    K = K1.copy()
    K[0, 2], K[1, 2] = 47.3, 36.9
    inst = [("a", 0, VC.pose(rng, (30.2, 30.7), 330.0, K)), ("b", 1, VC.pose(rng, (97.0, 20.0), 350.0, K)), ("c", 2, VC.pose(rng, (50.0, 66.0), 340.0, K)),
            ("d", 4, VC.pose(rng, (60.0, 40.0), 380.0, K)), ("e", 3, VC.pose(rng, (-20.0, 90.0), 350.0, K)), ("f", 1, VC.pose(rng, (400.0, 300.0), 350.0, K))]
    raw = _scene_raw(models, K, inst, w=W2, h=H2)
    raw[:, 40:55] = 1800
    raw[10:30, 60:90] = 0
    return [{"label": "second_size", "K": K, "instances": inst, "raw": raw}]


def flat(imgs):
    """``(model index [n], T [n,3,4], K [n,3,3], image_index [n], depth float32 [n_images,H,W])`` of a list of images, in file order."""
    m = np.array([i[1] for im in imgs for i in im["instances"]], np.int32)
    T = np.stack([i[2] for im in imgs for i in im["instances"]])
    K = np.stack([im["K"] for im in imgs for _ in im["instances"]])
    ii = np.array([k for k, im in enumerate(imgs) for _ in im["instances"]], np.int32)
    depth = np.stack([read_raw(im["raw"]) for im in imgs])
    return m, T, K, ii, depth


def labels(imgs):
    return [f"{im['label']}/{i[0]}" for im in imgs for i in im["instances"]]
