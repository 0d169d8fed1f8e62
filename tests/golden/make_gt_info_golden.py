"""Pin the scene_gt_info / ground-truth mask row (N7) against the REFERENCE's vendored bop_toolkit (imported from /root/reference in the build container):
its two scripts, scripts/calc_gt_info.py and scripts/calc_gt_masks.py, are run THEMSELVES, unmodified, with runpy.run_path on a small tree this generator
writes from tests/golden/gt_info_cases.py.  The toolkit's renderer needs OpenGL, so ``renderer.create_renderer`` returns a stub whose ``render_object``
draws with the numpy rasteriser of tests/vsd_ref.py at the width and height the script asked for -- what is pinned is everything after the renderer.  The
other stubs only point the scripts at the tree (dataset_params) and stand in for the absent image codec (inout.load_depth: PIL; inout.save_im: captured).

Recorded (tests/golden/gt_info_golden.npz): the text of scene_gt_info.json as the script wrote it, the masks as packed bits, and the 16-bit depth images
(they are regenerated from seeds by the tests, which compare them with these).

    python tests/golden/make_gt_info_golden.py
"""
import json
import os
import runpy
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TOOLKIT = "/root/reference/thirdparty/bop_toolkit"
sys.path.insert(0, ROOT)
sys.path.insert(0, TOOLKIT)
np.float = float                                  # the vendored toolkit predates numpy 1.24
for _absent in ("imageio", "png"):                # image codecs imported at the top of inout.py; replaced below where the scripts use them
    sys.modules.setdefault(_absent, types.ModuleType(_absent))

from bop_toolkit_lib import dataset_params, inout, renderer  # noqa: E402

from tests import gt_info_ref as GR  # noqa: E402
from tests import vsd_ref as VR  # noqa: E402
from tests.golden import gt_info_cases as GC  # noqa: E402
from tests.golden import vsd_cases as VC  # noqa: E402


class StubRenderer:
    def __init__(self, width, height, models):
        self.width, self.height, self.models = width, height, models

    def add_object(self, obj_id, model_path, **kwargs):
        assert obj_id - 1 in range(len(self.models))

    def render_object(self, obj_id, R, t, fx, fy, cx, cy):
        _, p, f, _ = self.models[obj_id - 1]
        K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
        return {"depth": VR.render_depth(p, f, np.hstack((R, np.reshape(t, (3, 1)))), K, self.width, self.height)}


def write_tree(root, imgs):
    from PIL import Image
    sdir = os.path.join(root, "ds", "test", f"{GC.SCENE_ID:06d}")
    os.makedirs(os.path.join(sdir, "depth"))
    cam = {str(i): {"cam_K": im["K"].ravel().tolist(), "depth_scale": GC.DEPTH_SCALE} for i, im in enumerate(imgs)}
    gt = {str(i): [{"cam_R_m2c": T[:, :3].ravel().tolist(), "cam_t_m2c": T[:, 3].tolist(), "obj_id": int(m) + 1} for _, m, T in im["instances"]]
          for i, im in enumerate(imgs)}
    for name, obj in (("scene_camera.json", cam), ("scene_gt.json", gt)):
        with open(os.path.join(sdir, name), "w") as f:
            json.dump(obj, f)
    for i, im in enumerate(imgs):
        Image.fromarray(im["raw"]).save(os.path.join(sdir, "depth", f"{i:06d}.png"))
    return sdir


def check_conditions(imgs, models):
    """What makes every output an integer that can be compared exactly: no sample of either canvas within the NEAR band of an edge, the window of the 3x
    render equal to the plain render bit for bit, no pixel deciding within 1e-3 mm of delta."""
    worst = np.inf
    for im in imgs:
        test = GC.read_raw(im["raw"])
        h, w = test.shape
        for lab, m, T in im["instances"]:
            _, large, near_l, margin = GR.gt_info(models[m][1], models[m][2], T, im["K"], test, GC.DELTA, details=True)
            _, _, plain, near_p = GR.gt_masks(models[m][1], models[m][2], T, im["K"], test, GC.DELTA, details=True)
            assert not near_l.any() and not near_p.any(), (im["label"], lab, int(near_l.sum()), int(near_p.sum()))
            assert np.array_equal(large[h:2 * h, w:2 * w].view(np.uint32), plain.view(np.uint32)), (im["label"], lab)
            assert margin > 1e-3, (im["label"], lab, margin)
            worst = min(worst, margin)
    return worst


if __name__ == "__main__":
    from PIL import Image
    models = VC.models()
    imgs = GC.images()
    print("conditions hold; smallest |float32 difference - delta|:", check_conditions(imgs, models), "mm;",
          "second size:", check_conditions(GC.images_second_size(), models), "mm")
    saved = {}
    with tempfile.TemporaryDirectory() as tmp:
        sdir = write_tree(tmp, imgs)
        split = {"im_size": (GC.W, GC.H), "scene_camera_tpath": os.path.join(tmp, "ds", "test", "{scene_id:06d}", "scene_camera.json"),
                 "scene_gt_tpath": os.path.join(tmp, "ds", "test", "{scene_id:06d}", "scene_gt.json"),
                 "scene_gt_info_tpath": os.path.join(tmp, "ds", "test", "{scene_id:06d}", "scene_gt_info.json"),
                 "depth_tpath": os.path.join(tmp, "ds", "test", "{scene_id:06d}", "depth", "{im_id:06d}.png"),
                 "mask_tpath": os.path.join(tmp, "ds", "test", "{scene_id:06d}", "mask", "{im_id:06d}_{gt_id:06d}.png"),
                 "mask_visib_tpath": os.path.join(tmp, "ds", "test", "{scene_id:06d}", "mask_visib", "{im_id:06d}_{gt_id:06d}.png")}
        dataset_params.get_split_params = lambda *a, **k: split
        dataset_params.get_model_params = lambda *a, **k: {"obj_ids": list(range(1, len(models) + 1)), "model_tpath": os.path.join(tmp, "obj_{obj_id:06d}.ply")}
        dataset_params.get_present_scene_ids = lambda dp: [GC.SCENE_ID]
        renderer.create_renderer = lambda width, height, *a, **k: StubRenderer(width, height, models)
        inout.load_depth = lambda path: np.asarray(Image.open(path)).astype(np.float32)
        inout.save_im = lambda path, im, jpg_quality=95: saved.__setitem__(os.path.relpath(path, sdir), np.array(im))
        runpy.run_path(os.path.join(TOOLKIT, "scripts", "calc_gt_info.py"), run_name="__main__")
        runpy.run_path(os.path.join(TOOLKIT, "scripts", "calc_gt_masks.py"), run_name="__main__")
        with open(os.path.join(sdir, "scene_gt_info.json"), "r") as f:
            text = f.read()
    masks, masks_visib = [], []
    for i, im in enumerate(imgs):
        for g in range(len(im["instances"])):
            for kind, dst in (("mask", masks), ("mask_visib", masks_visib)):
                a = saved.pop(os.path.join(kind, f"{i:06d}_{g:06d}.png"))
                assert a.dtype == np.uint8 and a.shape == (GC.H, GC.W) and np.isin(a, (0, 255)).all()
                dst.append(a > 0)
    assert not saved
    info = json.loads(text)
    fr = [e["visib_fract"] for v in info.values() for e in v]
    print("instances", len(fr), "visib_fract: zero", sum(f == 0 for f in fr), "partial", sum(0 < f < 1 for f in fr), "full", sum(f == 1 for f in fr))
    for lab, e in zip(GC.labels(imgs), [e for k in sorted(info, key=int) for e in info[k]]):
        print(f"{lab:28s}", e)
    out = {"text": np.frombuffer(text.encode(), np.uint8), "mask_bits": np.packbits(np.stack(masks)), "mask_visib_bits": np.packbits(np.stack(masks_visib)),
           "raw": np.stack([im["raw"] for im in imgs])}
    path = os.path.join(ROOT, "tests", "golden", "gt_info_golden.npz")
    np.savez_compressed(path, **out)
    print("recorded", {k: v.shape for k, v in out.items()}, os.path.getsize(path), "bytes")
