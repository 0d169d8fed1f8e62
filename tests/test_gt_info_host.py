"""Host side of the scene_gt_info / ground-truth mask row (N7).  No GPU.

The toolkit's own scripts/calc_gt_info.py and scripts/calc_gt_masks.py wrote tests/golden/gt_info_golden.npz (tests/golden/make_gt_info_golden.py); the
numpy restatement tests/gt_info_ref.py -- the yardstick of the GPU tests at sizes the scripts were not run on -- must reproduce that exactly, the formatter
must write the script's text byte for byte, and the two entries must refuse bad arguments before they need a device."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from suo_slam_amd import _lib, bop_gt_info
from tests import gt_info_ref as GR
from tests.golden import gt_info_cases as GC
from tests.golden import vsd_cases as VC

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "gt_info_golden.npz"))
TEXT = GOLD["text"].tobytes().decode()
SUO_ERR_ARG = 1


def gold_info():
    return {int(k): v for k, v in json.loads(TEXT).items()}


def gold_masks():
    n = sum(len(v) for v in gold_info().values())
    return tuple(255 * np.unpackbits(GOLD[k]).reshape(n, GC.H, GC.W).astype(np.uint8) for k in ("mask_bits", "mask_visib_bits"))


@pytest.fixture(scope="module")
def cases():
    return GC.images()


def test_the_cases_are_the_recorded_ones(cases):
    assert np.array_equal(np.stack([im["raw"] for im in cases]), GOLD["raw"])
    info = gold_info()
    assert sorted(info) == list(range(len(cases))) and [len(info[i]) for i in range(len(cases))] == [len(im["instances"]) for im in cases]
    by = dict(zip(GC.labels(cases), [e for i in range(len(cases)) for e in info[i]]))
    # what the cases were designed to hold
    for lab in ("borders/left", "borders/top"):
        assert min(by[lab]["bbox_obj"][:2]) < 0 and by[lab]["px_count_visib"] > 0
    assert by["borders/right"]["bbox_obj"][0] + by["borders/right"]["bbox_obj"][2] >= GC.W
    assert by["borders/bottom"]["bbox_obj"][1] + by["borders/bottom"]["bbox_obj"][3] >= GC.H
    e = by["borders/canvas_only"]
    assert e["px_count_all"] > 0 and e["px_count_visib"] == 0 and e["bbox_obj"] == [-1] * 4 and e["bbox_visib"] == [-1] * 4
    assert by["borders/nowhere"] == {"px_count_all": 0, "px_count_valid": 0, "px_count_visib": 0, "visib_fract": 0.0, "bbox_obj": [-1] * 4, "bbox_visib": [-1] * 4}
    assert by["borders/spike"]["bbox_obj"][0] == -GC.W                          # the spike reaches the canvas's left edge
    assert all(0 < by[f"slab/mid{m}"]["visib_fract"] < 1 for m in range(3))
    assert all(by[f"holes/mid{m}"]["px_count_valid"] < by[f"holes/mid{m}"]["px_count_visib"] for m in range(3))
    assert all(by[f"no_depth/mid{m}"]["px_count_valid"] == 0 and by[f"no_depth/mid{m}"]["visib_fract"] == 1.0 for m in range(3))
    assert all(by[f"wall/mid{m}"]["px_count_visib"] == 0 and by[f"wall/mid{m}"]["px_count_all"] > 0 for m in range(3))
    assert by["other_K/other_K"]["px_count_visib"] > 0


def test_numpy_restatement_equals_the_toolkit_scripts(cases):
    models = VC.models()
    info, masks, masks_visib = {}, [], []
    for i, im in enumerate(cases):
        test = GC.read_raw(im["raw"])
        info[i] = [GR.gt_info(models[m][1], models[m][2], T, im["K"], test, GC.DELTA) for _, m, T in im["instances"]]
        for _, m, T in im["instances"]:
            a, b = GR.gt_masks(models[m][1], models[m][2], T, im["K"], test, GC.DELTA)
            masks.append(a)
            masks_visib.append(b)
    assert info == gold_info()
    assert bop_gt_info.format_scene_gt_info(info) == TEXT
    gm, gv = gold_masks()
    assert np.array_equal(np.stack(masks), gm) and np.array_equal(np.stack(masks_visib), gv)
    assert gm.any() and gv.any() and (gm != gv).any()


def test_format_is_byte_identical_and_floats_round_trip():
    info = gold_info()
    assert bop_gt_info.format_scene_gt_info(info) == TEXT
    assert not TEXT.endswith("\n") and TEXT.count("\n") == len(info) + 1
    fracts = [e["visib_fract"] for v in info.values() for e in v]
    assert any(0 < f < 1 for f in fracts)
    for f in fracts:
        assert float(repr(f)) == f and f" {repr(f)}" in TEXT
    # a fraction formed from the integers, as the entry's caller forms it, prints as the script printed it
    for v in info.values():
        for e in v:
            assert e["visib_fract"] == (e["px_count_visib"] / float(e["px_count_all"]) if e["px_count_all"] > 0 else 0.0)
    # keys of any order, one image, no image
    assert bop_gt_info.format_scene_gt_info({7: [], 3: [{"b": 1, "a": [2]}]}) == '{\n  "3": [{"a": [2], "b": 1}],\n  "7": []\n}'
    assert bop_gt_info.format_scene_gt_info({}) == "{\n}"


def test_symbols_are_declared_exported_and_typed():
    with open(os.path.join(HERE, "..", "include", "suo_hip.h"), "r") as f:
        header = f.read()
    lib = _lib.lib()
    for name, n_args in (("suo_gt_info", 14), ("suo_gt_masks", 13)):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == n_args
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args and args[10] is C.c_double
        assert getattr(lib, name).argtypes == args


def _call(lib, which, h, n, m, T, K, w, h_, n_images, test, ii, delta, null=None):
    outs = [np.zeros((max(n, 1), 3), np.int64), np.zeros((max(n, 1), 4), np.int32), np.zeros((max(n, 1), 4), np.int32)] if which == "suo_gt_info" else \
        [np.zeros((max(n, 1), h_ if h_ > 0 else 1, w if 0 < w < 4096 else 1), np.uint8) for _ in range(2)]
    ptr = [a.ctypes.data for a in (m, T, K, test, ii)] + [o.ctypes.data for o in outs]
    if null is not None:
        ptr[null] = None
    return getattr(lib, which)(h, n, ptr[0], ptr[1], ptr[2], w, h_, n_images, ptr[3], ptr[4], delta, *ptr[5:])


@pytest.mark.parametrize("which", ["suo_gt_info", "suo_gt_masks"])
def test_refusals_need_no_device(which):
    """Every argument rule that does not depend on the database is checked before the database is looked at: with a null handle the message names the
    argument, and only a call that passes them all is refused for the handle.  (A bad model index and a model without faces need a database: GPU test.)"""
    lib = _lib.lib()
    n, w, h = 2, 8, 6
    m, ii = np.zeros(n, np.int32), np.zeros(n, np.int32)
    T = np.tile(np.hstack((np.eye(3), [[0.0], [0.0], [400.0]])).reshape(1, 12), (n, 1))
    K = np.tile(np.array([[100.0, 0, 4], [0, 100.0, 3], [0, 0, 1]]).reshape(1, 9), (n, 1))
    test = np.zeros((1, h, w), np.float32)

    def refused(why, **kw):
        a = dict(h=None, n=n, m=m, T=T, K=K, w=w, h_=h, n_images=1, test=test, ii=ii, delta=15.0, null=None)
        a.update(kw)
        rc = _call(lib, which, **a)
        msg = lib.suo_last_error().decode()
        assert rc == SUO_ERR_ARG and why in msg and which in msg, (why, rc, msg)

    refused("null mesh database")                                              # everything else is fine
    for k in range(5):                                                         # model_index, T, K, depth_test, image_index
        refused("null pointer", null=k)
    if which == "suo_gt_info":
        for k in range(5, 8):
            refused("null pointer", null=k)
    bad = T.copy()
    bad[1, 7] = np.nan
    refused("pose 1 is not finite", T=bad)
    bad = K.copy()
    bad[0, 4] = np.inf
    refused("camera matrix 0 is not finite", K=bad)
    refused("delta is not finite", delta=float("nan"))
    refused("delta is not finite", delta=float("inf"))
    refused("image_index[1]=1 out of range", ii=np.array([0, 1], np.int32))
    refused("image_index[0]=-1 out of range", ii=np.array([-1, 0], np.int32))
    refused("n_images=0", n_images=0)
    refused("width and height >= 1", w=0)
    refused("width and height >= 1", h_=-3)
    refused("n >= 0", n=-1)
    # 3 width x 3 height beyond the rasteriser's pixel boxes; nothing is read before the refusal, so the small buffers do
    refused("overflows", w=2 ** 31 - 1, h_=1)
    refused("overflows", w=1, h_=2 ** 30)
    refused("overflows", w=8192, h_=4096)                                      # 9 w h = 2^28 * 1.125
    # n = 0 returns 0 whatever the rest holds, as for the VSD entries -- but only with a database
    assert _call(lib, which, None, 0, m, T, K, w, h, 0, test, ii, 15.0) == SUO_ERR_ARG
