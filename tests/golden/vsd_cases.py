"""Seeded inputs of the VSD goldens and GPU tests (row N6), shared by tests/golden/make_vsd_golden.py (which runs the REFERENCE's vendored bop_toolkit on
them, build container only) and by the tests (which regenerate them, so tests/golden/vsd_golden.npz holds results only).  Nothing here comes from the toolkit.

Images are 160 x 96: 3 x 2 tiles of 64 x 64 pixels, the last column and the last row partial."""
import numpy as np

from tests import vsd_ref as VR
from tests.golden import bop19_cases as BC

W, H = 160, 96
K0 = np.array([[150.0, 0.0, 80.0], [0.0, 150.0, 48.0], [0.0, 0.0, 1.0]])
DELTA = 15
TAUS = np.arange(0.05, 0.51, 0.05)
BACKGROUND = 900.0
PLY_TREE = dict(dset="tless", seed=31, n_scenes=1, n_views=1)      # the tree of tests/bop_tree.py whose objects 1 (binary PLY) and 2 (ascii) are recorded


def models():
    """``[(name, points float32 [P,3], faces int32 [F,3], diameter)]``: box (12 faces), icosphere (320), soup (200, both windings), the box with a zero-area
    face and a face of three equal indices, and a box with six spikes of 1000 mm along its axes (one tip is behind the camera at every pose used here, whatever the rotation)."""
    bp, bf = VR.box_mesh()
    ip, if_ = VR.icosphere()
    sp, sf = VR.soup()
    dp = np.vstack((bp, (bp[0] + bp[7])[None] / 2)).astype(np.float32)                      # vertex 8: the midpoint of a diagonal -> collinear with 0 and 7
    df = np.vstack((bf, [[0, 8, 7], [3, 3, 3]])).astype(np.int32)
    tips = [[1000.0 * sg if ax == k else 0.0 for k in range(3)] for ax in range(3) for sg in (-1, 1)]      # |R[2, k]| >= 0.577 for some k: one tip has Z < 0 below Z = 577
    kp = np.vstack((bp, tips)).astype(np.float32)
    kf = np.vstack((bf, [[0, 8 + j, 7 - j] for j in range(6)])).astype(np.int32)
    out = []
    for name, p, f in (("box", bp, bf), ("ico", ip, if_), ("soup", sp, sf), ("degenerate", dp, df), ("spike", kp, kf)):
        d = float(np.max(np.linalg.norm(p[:8 if name == "spike" else None, None, :] - p[None, :8 if name == "spike" else None, :], axis=-1)))
        out.append((name, p, f, d))
    return out


def pose(rng, centre_px, z, K=K0):
    """A random rotation with the object's origin projecting to ``centre_px`` at depth ``z``."""
    t = np.array([(centre_px[0] - K[0, 2]) / K[0, 0] * z, (centre_px[1] - K[1, 2]) / K[1, 1] * z, z])
    return np.hstack((BC.random_rotation(rng), t[:, None]))


def render_cases(seed=11):
    """``[(label, model index, T [3,4], K [3,3])]``: every model straddling a tile corner, crossing the image border, the box near the camera (large
    triangles), one object wholly outside the image, other focal lengths and principal points."""
    rng = np.random.default_rng(seed)
    out = []
    for m in range(5):
        out.append((f"corner{m}", m, pose(rng, (64.0 + rng.uniform(-3, 3), 64.0 + rng.uniform(-3, 3)), rng.uniform(330, 420)), K0))
        out.append((f"border{m}", m, pose(rng, (rng.uniform(150, 165), rng.uniform(-5, 10)), rng.uniform(300, 380)), K0))
    out.append(("near_box", 0, pose(rng, (70.0, 50.0), 95.0), K0))
    out.append(("outside", 1, pose(rng, (400.0, -300.0), 350.0), K0))
    K1 = np.array([[131.7, 0.0, 77.3], [0.0, 140.2, 51.9], [0.0, 0.0, 1.0]])
    out.append(("other_K", 2, pose(rng, (128.2, 63.7), 300.0, K1), K1))
    out.append(("far_ico", 1, pose(rng, (30.0, 30.0), 1400.0), K0))                       # a few pixels across: sub-pixel triangles
    return out


def vsd_pairs(seed=23):
    """``[{"label", "m", "Te", "Tg", "K", "test" float32 [H,W] mm, "normalized"}]``: estimates near and far from the ground truth, est == gt, scenes with an
    occluding slab, with missing depth (holes, and a wholly empty image), and pairs whose union is empty (the object outside the image; the object hidden
    behind a wall)."""
    rng = np.random.default_rng(seed)
    ms = models()
    out = []
    kinds = ("near", "far", "same", "holes", "occluded", "no_depth", "outside", "hidden", "near", "far", "occluded", "holes")
    for i, kind in enumerate(kinds):
        m = i % 3 if kind != "near" else (3 + i % 2)
        _, p, f, _ = ms[m]
        Tg = pose(rng, (rng.uniform(40, 120), rng.uniform(30, 66)), rng.uniform(320, 420))
        if kind == "outside":
            Tg = pose(rng, (500.0, 400.0), 350.0)
        small = np.hstack((BC.rotvec(rng.standard_normal(3) * 0.05), rng.standard_normal((3, 1)) * np.array([[3.0], [3.0], [8.0]])))
        large = np.hstack((BC.rotvec(rng.standard_normal(3) * 0.5), rng.standard_normal((3, 1)) * np.array([[15.0], [15.0], [40.0]])))
        Te = Tg.copy() if kind in ("same", "no_depth") else BC.compose(Tg, large if kind == "far" else small)
        if kind == "outside":
            Te = BC.compose(Tg, small)
        test = np.full((H, W), BACKGROUND, np.float32)
        d = VR.render_depth(p, f, Tg, K0, W, H)
        test = np.where(d > 0, d, test).astype(np.float32)
        if kind == "occluded":
            test[:, 70:110] = 180.0                                            # a slab in front of the middle of the image
        if kind == "holes":
            test[30:60, 50:100] = 0.0
        if kind == "no_depth":
            test[:] = 0.0
        if kind == "hidden":
            test[:] = 150.0                                                    # a wall in front of everything
        out.append({"label": f"{kind}{i}", "m": m, "Te": Te, "Tg": Tg, "K": K0.copy(), "test": test, "normalized": bool(i % 2 == 0)})
    return out


SPHERE_CASES = (
    (50.0, [0.0, 0.0, 0.0], [10.0, 0.0, 500.0]),          # Z = 0 of the first centre
    (50.0, [0.0, 0.0, 500.0], [10.0, 0.0, 0.0]),          # ... of the second
    (50.0, [0.0, 0.0, 500.0], [99.0, 0.0, 500.0]),        # just inside the bound (100 / 500)
    (50.0, [0.0, 0.0, 500.0], [101.0, 0.0, 500.0]),       # just outside it
    (80.0, [30.0, -20.0, 700.0], [-80.0, 45.0, 450.0]),
    (60.0, [30.0, -20.0, 700.0], [-230.0, 145.0, 450.0]),
    (50.0, [0.0, 0.0, -500.0], [10.0, 0.0, 500.0]),       # a centre behind the camera: a negative bound
)


def vsd_match_case():
    """The matching case of tests/golden/bop19_cases.py with VSD-like errors: per ground truth one error per tau in [0, 1], falling with tau; an infinite
    error there becomes 1.0."""
    gt_obj_ids, gt_valid, inst_count, ests = BC.match_case()
    out = {}
    for key, rows in ests.items():
        out[key] = [{"score": r["score"], "errors": {g: [1.0 if not np.isfinite(e) else float(np.round(min(1.0, e) * (1.0 - 0.07 * t), 3)) for t in range(len(TAUS))]
                                                     for g, e in r["errors"].items()}} for r in rows]
    return gt_obj_ids, gt_valid, inst_count, out
