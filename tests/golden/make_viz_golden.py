#!/usr/bin/env python3
"""Golden pictures and draw calls of the three-panel visualisation, produced by running the REFERENCE's own ObjectSLAM.collect_results(no_viz=False) and
utils.make_kp_viz / draw_points / bbox_color (imported unmodified) in the build container:

    python tests/golden/make_viz_golden.py          ->  tests/golden/viz_golden.npz

tests/golden/ref_stubs.py installs the stand-ins for the reference's missing imports; its cv2 module is extended HERE, after install(), by the calls the
visualisation makes: circle / ellipse / rectangle / putText / dilate / getStructuringElement / cvtColor RECORD their arguments and rasterise by the stated
rules of tests/viz_ref.py (cv2 is absent: how a primitive is rasterised is unpinned; everything up to the list of primitives is the reference's own
arithmetic).  make_kp_viz is wrapped only to cast K to float32 (with a float64 K its ``pts @ K.T`` raises a dtype error under this torch).

Stored per case of tests/golden/viz_cases.py: the picture uint8 [H,3W,3] and the recorded draw calls as rows (kind, x, y, a, b, c, d, angle, b, g, r):
kind 0 = rectangle (x1, y1, x2, y2), 1 = circle (x, y, r), 2 = ellipse (x, y, A, B, angle in degrees as handed over), in call order; putText and dilate
calls are counted only.  Once: the reference's two colour tables.  The fixture is data only."""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import ref_stubs  # noqa: E402
import treeio  # noqa: E402
from tests import viz_ref  # noqa: E402
from tests.golden import viz_cases  # noqa: E402

ref = ref_stubs.install(ref_stubs.PnpStub())
import cv2  # noqa: E402  (the stand-in ref_stubs installed)
import torch  # noqa: E402

LOG = {"calls": [], "text": 0, "dilate": 0}


def _bgr(col):
    return [int(c) for c in list(col)[:3]]


def circle(img, center, radius, color, thickness):
    assert thickness == -1
    LOG["calls"].append([1, center[0], center[1], radius, 0, 0, 0, 0.0] + _bgr(color))
    return viz_ref.disc(img, center[0], center[1], radius, _bgr(color))


def ellipse(img, center, axes, angle, start, end, color, thickness):
    assert (start, end, thickness) == (0, 360, 2)
    LOG["calls"].append([2, center[0], center[1], axes[0], axes[1], 0, 0, float(angle)] + _bgr(color))
    return viz_ref.ellipse(img, center[0], center[1], axes[0], axes[1], float(angle), _bgr(color))


def rectangle(img, p1, p2, color, thickness):
    assert thickness == 3
    LOG["calls"].append([0, p1[0], p1[1], p2[0], p2[1], 0, 0, 0.0] + _bgr(color))
    return viz_ref.box(img, p1[0], p1[1], p2[0], p2[1], _bgr(color))


def put_text(img, *a, **kw):
    LOG["text"] += 1                               # (labels are not drawn: a stated deviation)
    return img


def dilate(mask, kernel, iterations=1):
    assert kernel.shape == (3, 3) and kernel.all() and iterations == 1
    LOG["dilate"] += 1
    return viz_ref.dilate3(mask)


def cvt_color(img, code):
    assert code == cv2.COLOR_BGR2GRAY
    return viz_ref.gray(img)


cv2.circle, cv2.ellipse, cv2.rectangle, cv2.putText, cv2.dilate, cv2.cvtColor = circle, ellipse, rectangle, put_text, dilate, cvt_color
cv2.getStructuringElement = lambda shape, size: np.ones(size, np.uint8)
cv2.MORPH_RECT, cv2.COLOR_BGR2GRAY, cv2.FONT_HERSHEY_PLAIN, cv2.LINE_AA = 0, 6, 1, 16

_make_kp_viz = ref.utils.make_kp_viz


def make_kp_viz(image, *a, K=None, **kw):
    return _make_kp_viz(image, *a, K=None if K is None else np.asarray(K, np.float32), **kw)


ref.utils.make_kp_viz = make_kp_viz


def quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return f(*a, **kw)


def run_case(case):
    mesh_db = {o: {"points": torch.from_numpy(p.copy()), "diameter": 100.0, "is_symmetric": False} for o, p in case["meshes"].items()}
    s = quiet(ref.ObjectSLAM, None, mesh_db, debug_gt_kp=True, sfm_mode=True, viz_cov=case["viz_cov"])
    viz_cases.install(s, case)
    for o, T in case["obj_poses"].items():         # the generator asserts what the cases promise: no projected coordinate near a pixel boundary
        to4 = lambda M: np.concatenate((M, np.eye(4)[3:4, :]), axis=0) if M.shape[0] == 3 else M        # noqa: E731
        m = viz_ref.boundary_margin(case["meshes"][o], to4(case["cam_pose"]) @ to4(T), case["K"], case["H"], case["W"])
        assert m >= 1e-3, (case["name"], o, m)
    LOG["calls"], LOG["text"], LOG["dilate"] = [], 0, 0
    res = quiet(s.collect_results, False, False, False)
    img = res[viz_cases.VIEW]["viz"]
    assert img.dtype == np.uint8 and img.shape == (case["H"], 3 * case["W"], 3)
    return {"viz": img, "calls": np.array(LOG["calls"], np.float64).reshape(-1, 11), "n_text": LOG["text"], "n_dilate": LOG["dilate"]}


def main():
    out = {"kp_colors": np.asarray(ref.kp_config.kp_colors(), np.int64), "bbox_colors": np.array([ref.utils.bbox_color(o) for o in range(1, 31)], np.int64), "cases": {}}
    for case in viz_cases.all_cases():
        rec = run_case(case)
        out["cases"][case["name"]] = rec
        print(f"{case['name']}: {case['W']} x {case['H']}, {len(rec['calls'])} draw calls, {rec['n_text']} labels, {rec['n_dilate']} dilations, "
              f"{int((rec['viz'] != np.concatenate([case['frame']] * 3, axis=1)).any(axis=2).sum())} pixels painted")
    path = os.path.join(HERE, "viz_golden.npz")
    treeio.save(path, out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
