"""The tile pass of the rasteriser (csrc/raster_tile.h: draw_tile, shade) at its structural edges, on the device through the C ABI and under all three of its
epilogues (csrc/raster.hip, csrc/eval_masks.hip, csrc/gt_info.hip): renders of three and more chunks of 256 triangles, a tile list filled to its 256
entries in consecutive chunks, a triangle on the list in one tile and on a lane in the next, box ∩ tile of exactly 32 and 33 samples, widths that are no
multiple of 4 (the scalar stores of raster_tile_kernel), images smaller than a tile, last tile columns and rows of one pixel, permuted and doubled faces.

Inputs: tests/raster_tile_cases.py; tests/test_raster_tile_cases.py asserts without a GPU that they reach all of this.  Yardstick: the fp64 numpy rasteriser
tests/vsd_ref.render_depth, computed once per case (raster_tile_cases.reference).

Tolerances are those of tests/test_gpu_vsd.py.  Coverage is equal at every sample outside the NEAR band of a triangle edge (at most 0.1 % of an image, which
the reference alone is checked to meet; the cases here have none).  Depth is within one float32 ulp where both cover.  What is not covered is exactly 0.0,
and no pixel keeps the -7 the output buffer was filled with.  Integer-coordinate rectangles, permuted faces, doubled faces and batches are compared bit
for bit; mask counts, boxes, scene_gt_info entries and mask bytes are integers and compared exactly; the fused VSD route equals the render-then-error
route bit for bit."""
import numpy as np
import pytest

from suo_slam_amd import bop_eval
from tests import gt_info_ref as GR
from tests import points_errors_ref as PR
from tests import raster_tile_cases as RC
from tests import vsd_ref as VR
from tests.golden import vsd_cases as VC
from tests.test_gpu_vsd import Db, vsd_from_depth

pytestmark = pytest.mark.gpu

NAMES = ("ico3", "shingles", "full_list", "box")


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _models(names=NAMES):
    return [(n, RC.meshes()[n][0], RC.meshes()[n][1], 100.0) for n in names]


@pytest.fixture(scope="module")
def db():
    d = Db(_models())
    yield d
    d.close()


@pytest.fixture(scope="module")
def be():
    e = bop_eval.BopErrors({k + 1: {"points": RC.meshes()[n][0], "faces": RC.meshes()[n][1]} for k, n in enumerate(NAMES)}, {k + 1: {"diameter": 100.0} for k in range(len(NAMES))})
    yield e
    e.close()


def _render_case(db, label):
    mesh, T, K, w, h = RC.render_cases()[label]
    return db.render([(NAMES.index(mesh), T, K)], w, h)[0]


def _check(label, g):
    """One device image against the numpy render of the same case."""
    want, near = RC.reference(label)
    assert near.mean() <= 1e-3, (label, near.mean())                            # the reference alone: few samples sit on an edge
    assert g.shape == want.shape and not (g == -7.0).any(), (label, int((g == -7.0).sum()))      # every pixel of every row tail was written
    cmp = ~near
    assert np.array_equal((g > 0)[cmp], (want > 0)[cmp]), (label, int(((g > 0) != (want > 0))[cmp].sum()), np.argwhere(((g > 0) != (want > 0)) & cmp)[:5].tolist())
    both = cmp & (g > 0) & (want > 0)
    worst = int(_ulps(g[both], want[both]).max()) if both.any() else 0
    print(label, "covered", int((want > 0).sum()), "near", int(near.sum()), "max ulp", worst, "bit-equal", bool(np.array_equal(g, want)))
    assert worst <= 1, (label, worst, np.argwhere(both & (np.abs(g - want) > 0))[:5].tolist())
    assert (g[~(g > 0)] == 0).all(), label


@pytest.mark.parametrize("size", RC.CHUNK_SIZES + [(64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_many_chunks_and_a_full_list_equal_the_numpy_rasteriser(db, size):
    labels = [lab for lab, c in RC.render_cases().items() if lab.startswith("chunks/") and c[3:] == size]
    assert len(labels) == (1 if size == (64, 64) else 4)
    for lab in labels:
        _check(lab, _render_case(db, lab))
    # all of a size in one call: renders of 1280, 700 and 600 triangles side by side
    cases = [RC.render_cases()[lab] for lab in labels]
    got = db.render([(NAMES.index(c[0]), c[1], c[2]) for c in cases], *size)
    for lab, g in zip(labels, got):
        assert np.array_equal(g, _render_case(db, lab)), lab


@pytest.mark.parametrize("size", RC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_size_equals_the_numpy_rasteriser(db, size):
    w, h = size
    for name in ("box", "ico3"):
        lab = f"sizes/{name}@{w}x{h}"
        g = _render_case(db, lab)
        _check(lab, g)
        if size in ((1, 1), (3, 2)):
            assert (RC.reference(lab)[0] > 0).all() and (g > 0).all(), lab         # the pixel(s) are covered


def test_threshold_rectangles_are_bit_equal():
    P, F = RC.meshes()["threshold_rects"]
    d = Db([("threshold_rects", P, F, 1.0)])
    for w, h in RC.RECT_SIZES:
        got = d.render([(0, RC.RECT_T, RC.RECT_K)], w, h)[0]
        want = VR.render_depth(P, F, RC.RECT_T, RC.RECT_K, w, h)
        hand = np.zeros((h, w), np.float32)                                     # integers throughout: the image can be written down
        for x0, y0, x1, y1, Z in sorted(RC.RECTS, key=lambda r: -r[4]):
            hand[y0:min(y1, h), x0:min(x1, w)] = Z
        print(f"threshold_rects@{w}x{h}", "covered", int((want > 0).sum()), "max ulp", int(_ulps(got, want).max()), "bit-equal", bool(np.array_equal(got, want)))
        assert np.array_equal(want, hand)
        assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()
    d.close()


@pytest.mark.parametrize("name", ["ico3_near", "shingles"])
def test_face_order_and_doubled_faces_change_no_bit(db, name):
    w, h = RC.ODD
    lab = f"chunks/{name}@{w}x{h}"
    mesh, T, K, _, _ = RC.render_cases()[lab]
    P, F = RC.meshes()[mesh]
    base = _render_case(db, lab)
    assert (base > 0).sum() > 2000
    rng = np.random.default_rng(17)
    variants = {"permuted 1": F[rng.permutation(len(F))], "permuted 2": F[rng.permutation(len(F))], "doubled, reversed winding": np.vstack((F, F[:, ::-1])),
                "reversed order": F[::-1]}
    for what, faces in variants.items():
        d = Db([(mesh, P, np.ascontiguousarray(faces, np.int32), 100.0)])
        got = d.render([(0, T, K)], w, h)[0]
        d.close()
        assert np.array_equal(got, base), (name, what, int((got != base).sum()), np.argwhere(got != base)[:5].tolist())


def test_a_render_has_the_same_bits_alone_and_between_two_boxes(db):
    """1280 (and 700) triangles next to 12 in one call: the setup kernel's blocks past a render's last triangle return early, the tile kernel's chunk
    loops have different lengths in one launch."""
    box = NAMES.index("box")
    for w, h in (RC.ODD, (160, 96)):
        _, Tb, Kb, _, _ = RC.render_cases()["sizes/box@161x99"]
        for name in ("ico3_near", "shingles"):
            lab = f"chunks/{name}@{w}x{h}"
            mesh, T, K, _, _ = RC.render_cases()[lab]
            alone = _render_case(db, lab)
            batch = db.render([(box, Tb, Kb), (NAMES.index(mesh), T, K), (box, Tb, Kb)], w, h)
            assert np.array_equal(batch[1], alone), (lab, int((batch[1] != alone).sum()))
            assert np.array_equal(batch[0], batch[2]) and np.array_equal(batch[0], db.render([(box, Tb, Kb)], w, h)[0]) and (batch[0] > 0).any()


def test_mask_counts_and_boxes_equal_the_numpy_rasteriser(be):
    pairs = RC.mask_pairs()
    for w, h in sorted({(p[5], p[6]) for p in pairs}):
        sel = [p for p in pairs if (p[5], p[6]) == (w, h)]
        got = be.mask_errors([NAMES.index(p[1]) + 1 for p in sel], np.stack([p[2] for p in sel]), np.stack([p[3] for p in sel]), np.stack([p[4] for p in sel]), (h, w))
        for i, (lab, mesh, Te, Tg, K, _, _, e, g) in enumerate(sel):
            renders = {Te.tobytes(): RC.reference(e), Tg.tobytes(): RC.reference(g)}
            assert not any(r[1].any() for r in renders.values()), lab            # the reference alone: no sample in the NEAR band
            want = PR.mask_counts(None, None, Te, Tg, K, w, h, renders=lambda T: renders[T.tobytes()][0])
            dev = (int(got["union"][i]), int(got["inter"][i]), got["box_est"][i].tolist(), got["box_gt"][i].tolist())
            print(lab, "numpy", want, "device", dev)
            assert dev == want, lab
            assert want[0] > want[1] > 0
            # the pair alone and with estimate and ground truth exchanged: the two z-buffers of the kernel change places
            one = be.mask_errors([NAMES.index(mesh) + 1], Tg[None], Te[None], K[None], (h, w))
            assert (int(one["union"][0]), int(one["inter"][0]), one["box_gt"][0].tolist(), one["box_est"][0].tolist()) == want, lab


@pytest.fixture(scope="module")
def gt_reference():
    """``[(info, mask, mask_visib)]`` of raster_tile_cases.gt_cases() by tests/gt_info_ref.py, with the two conditions of tests/test_gpu_gt_info.py asserted."""
    out = []
    for lab, mesh, T, K, test in RC.gt_cases():
        P, F = RC.meshes()[mesh]
        info, _, near_l, margin = GR.gt_info(P, F, T, K, test, RC.DELTA, details=True)
        mask, mask_visib, _, near_p = GR.gt_masks(P, F, T, K, test, RC.DELTA, details=True)
        assert not near_l.any() and not near_p.any(), lab
        assert margin > 1e-3, (lab, margin)
        out.append((info, mask, mask_visib))
    return out


def test_gt_info_and_masks_equal_the_numpy_restatement(be, gt_reference):
    cases = RC.gt_cases()
    objs = [NAMES.index(c[1]) + 1 for c in cases]
    T, K, depth = np.stack([c[2] for c in cases]), np.stack([c[3] for c in cases]), [np.array(c[4]) for c in cases]
    got = be.gt_info(objs, T, K, depth, list(range(len(cases))), RC.DELTA)
    mask, mask_visib = be.gt_masks(objs, T, K, depth, list(range(len(cases))), RC.DELTA)
    for k, (c, g, r) in enumerate(zip(cases, got, gt_reference)):
        print(c[0], g)
        assert g == r[0], (c[0], g, r[0])
        assert np.array_equal(mask[k], r[1]) and np.array_equal(mask_visib[k], r[2]), c[0]
        assert mask[k].any() and (mask[k] != mask_visib[k]).any()
    rev = be.gt_info(objs[::-1], T[::-1], K[::-1], depth, list(range(len(cases)))[::-1], RC.DELTA)
    assert rev[::-1] == got


def test_fused_vsd_on_an_odd_width_equals_render_then_error_kernel(db):
    w, h = RC.ODD
    pairs, tests = RC.vsd_pairs()
    m = NAMES.index("shingles")
    for normalized in (True, False):
        e, c = db.vsd_poses([(m, Te, Tg, K, 100.0 if normalized else None) for Te, Tg, K in pairs], tests, [0, 1], w, h)
        de, dg = db.render([(m, Te, K) for Te, _, K in pairs], w, h), db.render([(m, Tg, K) for _, Tg, K in pairs], w, h)
        e2, c2 = vsd_from_depth(de, dg, tests, [0, 1], np.stack([p[2] for p in pairs]), normalized, [100.0, 100.0])
        print("normalized", normalized, "counts", c.tolist(), "errors", e.tolist())
        assert np.array_equal(c, c2) and np.array_equal(e, e2)
        assert (c[:, 0] > c[:, 1]).all() and (c[:, 1] > 0).all() and (e > 0).any() and (e < 1).any()
    assert VC.DELTA == RC.DELTA
