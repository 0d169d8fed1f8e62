"""The visualisation's host half against the reference's own draw calls and pictures (tests/golden/viz_golden.npz, made by tests/golden/make_viz_golden.py
from the reference's collect_results(no_viz=False) over the cv2 stand-in).  No GPU: suo_slam_amd.viz.build_primitives is numpy, the colour tables are data of
the library, and tests/viz_ref.py is the numpy statement of the rasterisation rules that tests/test_gpu_viz.py holds the kernels to."""
import os
import types

import numpy as np
import pytest

from tests import viz_ref
from tests.golden import treeio, viz_cases

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def built():
    from suo_slam_amd import build
    return build.build(verbose=False)


@pytest.fixture(scope="module")
def golden():
    return treeio.load(os.path.join(HERE, "golden", "viz_golden.npz"))


@pytest.fixture(scope="module")
def cases():
    return {c["name"]: c for c in viz_cases.all_cases()}


def primitives(case):
    from suo_slam_amd import viz
    return viz.view_primitives(viz_cases.install(types.SimpleNamespace(), case), viz_cases.VIEW)


def prior_window_mask(H, W, stamps):
    """Pixels some prior stamp reaches: where the picture may differ from the golden by one level (see test_viz_ref_reproduces_golden_pictures)."""
    m = np.zeros((H, W), bool)
    for _, ulx, uly, x0, x1, y0, y1, _ in np.asarray(stamps, np.int64).reshape(-1, 8):
        lx, hx = max(ulx, x0, 0), min(ulx + 90, x1, W)
        ly, hy = max(uly, y0, 0), min(uly + 90, y1, H)
        if lx < hx and ly < hy:
            m[ly:hy, lx:hx] = True
    return m


def compare_with_golden(img, want, case, prims):
    """(pixels differing by one level inside prior windows); asserts exact equality everywhere else and at most one level inside."""
    H, W = case["H"], case["W"]
    diff = np.abs(img.astype(np.int64) - want.astype(np.int64)).max(axis=2)
    allowed = np.zeros((H, 3 * W), bool)
    allowed[:, :W] = prior_window_mask(H, W, prims["stamp"])                  # the left panel only
    assert (diff[~allowed] == 0).all(), f"{case['name']}: {int((diff[~allowed] != 0).sum())} pixels differ outside the prior windows"
    assert diff.max(initial=0) <= 1, f"{case['name']}: a pixel differs by {int(diff.max())} levels"
    return int((diff != 0).sum())


def test_colour_tables_are_the_reference_s(built, golden):
    from suo_slam_amd import viz
    kp, bb = viz.colour_tables()
    assert np.array_equal(kp, golden["kp_colors"]) and np.array_equal(bb, golden["bbox_colors"])
    assert viz.bbox_color(1) == golden["bbox_colors"][0].tolist() and viz.bbox_color(0) == golden["bbox_colors"][-1].tolist()
    with pytest.raises(ValueError):
        viz.bbox_color(31)


def test_build_primitives_reproduces_the_recorded_draw_calls(built, golden, cases):
    """Centres, radii, half-axes, the angle to the last bit, colours and order: the rows make_viz_golden.py recorded from the reference's cv2 calls."""
    assert set(cases) == set(golden["cases"])
    n_ellipses = 0
    for name, case in cases.items():
        prims = primitives(case)
        rows = [[0, x1, y1, x2, y2, 0, 0, 0.0] + viz_ref.unpack(col) for x1, y1, x2, y2, col in prims["box"]]
        for (x, y, ro, ri, col, has, A, B), ang in zip(prims["kp"], prims["kp_angle"]):
            rows.append([1, x, y, ro, 0, 0, 0, 0.0, 0, 0, 0])
            rows.append([1, x, y, ri, 0, 0, 0, 0.0] + viz_ref.unpack(col))
            if has:
                rows.append([2, x, y, A, B, 0, 0, ang] + viz_ref.unpack(col))
                n_ellipses += 1
        got, want = np.array(rows, np.float64).reshape(-1, 11), golden["cases"][name]["calls"].reshape(-1, 11)
        assert got.shape == want.shape and np.array_equal(got, want), name          # (array_equal on float64: the angle bit for bit)
        assert golden["cases"][name]["n_text"] == len(prims["box"])                 # one label per box: counted, not drawn
        assert golden["cases"][name]["n_dilate"] == len(prims["overlay"])
    assert n_ellipses >= 10


def test_cases_hold_what_they_promise(cases):
    """No projected mesh coordinate within 1e-3 px of a pixel boundary under fp64, so that the reference's float32 projection and the fp64 rule agree; and
    the designed edges are there: keypoints dropped for an off-canvas centre, half-axes 0, 1, 2 and large, a negative x1, a shared prior channel."""
    from suo_slam_amd import viz  # noqa: F401
    to4 = lambda M: np.concatenate((M, np.eye(4)[3:4, :]), axis=0) if M.shape[0] == 3 else M        # noqa: E731
    for case in cases.values():
        for o, T in case["obj_poses"].items():
            assert viz_ref.boundary_margin(case["meshes"][o], to4(case["cam_pose"]) @ to4(T), case["K"], case["H"], case["W"]) >= 1e-3
    kp = primitives(cases["keypoints"])
    assert len(kp["kp"]) == 17 - 4                                                  # four centres one pixel off the canvas
    assert kp["box"][:, 0].min() < 0
    ell = primitives(cases["ellipses"])["kp"]
    axes = set(ell[:, 6].tolist()) | set(ell[:, 7].tolist())
    assert {0, 1, 2} <= axes and max(axes) >= 25
    st = primitives(cases["priors"])["stamp"]
    assert len(st) == 10 and (np.bincount(st[:, 0], minlength=41) == 2).sum() == 2  # channels 0 and 2 come from two objects
    assert ((st[:, 4] - st[:, 3]) == 0).any()                                       # the window Python's slice leaves empty (negative x1)
    ov = primitives(cases["overlay"])["overlay"]
    assert [o for o, *_ in ov] == [4, 1, 7, 5, 6, 2, 10, 3]                         # far to near, the stable order within the equal pair (5, 6)
    assert primitives(cases["empty"])["box"].size == 0


def test_viz_ref_reproduces_golden_pictures(built, golden, cases):
    """tests/viz_ref.py fed the product's primitives equals the reference's pictures.  Exact everywhere outside the prior windows.  Inside them the golden's
    stamp comes from the cv2 stand-in's GaussianBlur (float32 outer product of a normalised kernel, divided by its maximum, and no doubling of the
    outermost ring) and the product's from its own table (include/suo_hip.h): the two differ in float32's last bit, and by the ring's factor 2 in the stamp's
    row 0 and column 0, which moves a blended byte by at most one level.  Counted over all six cases: 66 pixels, all in the case "priors" (none in "all", whose
    two stamps stay clear of it); the assertion is the bound of one level, the count is printed."""
    total = 0
    for name, case in cases.items():
        prims = primitives(case)
        img = viz_ref.render(case["frame"], prims, case["meshes"], golden["kp_colors"])
        assert img.shape == (case["H"], 3 * case["W"], 3) and img.dtype == np.uint8
        n = compare_with_golden(img, golden["cases"][name]["viz"], case, prims)
        print(f"{name}: {n} pixels one level off inside prior windows")
        total += n
    print(f"total: {total}")


def test_empty_view_is_three_frames(cases):
    case = cases["empty"]
    from suo_slam_amd import viz  # noqa: F401
    img = viz_ref.render(case["frame"], primitives(case), {}, np.zeros((41, 3), np.int64))
    assert np.array_equal(img, np.concatenate([case["frame"]] * 3, axis=1))
