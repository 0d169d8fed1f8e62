"""suo_gt_info / suo_gt_masks (csrc/gt_info.hip, row N7) on the device, through BopErrors and the C ABI.

Yardsticks: what the toolkit's own scripts/calc_gt_info.py and scripts/calc_gt_masks.py wrote on the cases of tests/golden/gt_info_cases.py
(tests/golden/gt_info_golden.npz, made by tests/golden/make_gt_info_golden.py), and, where the scripts were not run, the numpy restatement
tests/gt_info_ref.py, which tests/test_gt_info_host.py ties to them.

Tolerance: none.  Every output is an integer (or a mask byte) and is compared exactly, under two conditions the generator asserted and these tests assert
again on the regenerated inputs: no sample of a canvas lies within the NEAR band of a triangle edge in the numpy rasteriser (the only place where the
device's coverage may differ from it), and no pixel has |float32 distance difference - delta| <= 1e-3 mm (a rendered depth may differ from numpy's by one
float32 ulp, 3e-5 mm at these depths).  Images are 160 x 96: a canvas of 480 x 288 is 8 x 5 tiles with a partial last row, the window starts 2.5 tiles in."""
import json
import os

import numpy as np
import pytest

from suo_slam_amd import _lib, bop, bop_eval, bop_gt_info
from tests import bop_tree
from tests import gt_info_ref as GR
from tests import vsd_ref as VR
from tests.golden import gt_info_cases as GC
from tests.golden import vsd_cases as VC

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gt_info_golden.npz"))
TEXT = GOLD["text"].tobytes().decode()
SUO_ERR_ARG = 1
MARGIN = 1e-3


def _errors(models):
    return bop_eval.BopErrors({m + 1: {"points": p, "faces": f} for m, (_, p, f, _) in enumerate(models)}, {m + 1: {"diameter": d} for m, (_, _, _, d) in enumerate(models)})


@pytest.fixture(scope="module")
def be():
    e = _errors(VC.models())
    yield e
    e.close()


def _reference(imgs):
    """The numpy restatement of every instance of ``imgs``, with the two conditions asserted: ``[(info, mask, mask_visib, plain depth)]``."""
    models = VC.models()
    out = []
    for im in imgs:
        test = GC.read_raw(im["raw"])
        for lab, m, T in im["instances"]:
            info, _, near_l, margin = GR.gt_info(models[m][1], models[m][2], T, im["K"], test, GC.DELTA, details=True)
            mask, mask_visib, plain, near_p = GR.gt_masks(models[m][1], models[m][2], T, im["K"], test, GC.DELTA, details=True)
            assert not near_l.any() and not near_p.any(), (im["label"], lab)
            assert margin > MARGIN, (im["label"], lab, margin)
            out.append((info, mask, mask_visib, plain))
    return out


@pytest.fixture(scope="module")
def cases():
    imgs = GC.images()
    assert np.array_equal(np.stack([im["raw"] for im in imgs]), GOLD["raw"])
    return imgs


@pytest.fixture(scope="module")
def ref(cases):
    return _reference(cases)


def _run_info(be, imgs, order=None):
    m, T, K, ii, depth = GC.flat(imgs)
    order = np.arange(len(m)) if order is None else np.asarray(order)
    got = be.gt_info((m[order] + 1).tolist(), T[order], K[order], list(depth), ii[order].tolist(), GC.DELTA)
    return got


def _per_image(imgs, entries):
    it = iter(entries)
    return {i: [next(it) for _ in im["instances"]] for i, im in enumerate(imgs)}


def test_info_equals_the_toolkit(be, cases, ref):
    got = _run_info(be, cases)
    gold = {int(k): v for k, v in json.loads(TEXT).items()}
    flat_gold = [e for i in range(len(cases)) for e in gold[i]]
    for lab, g, w, r in zip(GC.labels(cases), got, flat_gold, ref):
        print(lab, g)
        assert g == w, (lab, g, w)
        assert g == r[0], lab
        assert all(type(g[k]) is int for k in ("px_count_all", "px_count_valid", "px_count_visib")) and type(g["visib_fract"]) is float
        assert all(type(v) is int for k in ("bbox_obj", "bbox_visib") for v in g[k])
    assert bop_gt_info.format_scene_gt_info(_per_image(cases, got)) == TEXT


def test_masks_equal_the_toolkit(be, cases, ref):
    m, T, K, ii, depth = GC.flat(cases)
    mask, mask_visib = be.gt_masks((m + 1).tolist(), T, K, list(depth), ii.tolist(), GC.DELTA)
    n = len(m)
    gm, gv = (255 * np.unpackbits(GOLD[k]).reshape(n, GC.H, GC.W).astype(np.uint8) for k in ("mask_bits", "mask_visib_bits"))
    assert mask.dtype == np.uint8 and mask_visib.dtype == np.uint8
    assert np.array_equal(mask, gm) and np.array_equal(mask_visib, gv)
    assert np.array_equal(mask, np.stack([r[1] for r in ref])) and np.array_equal(mask_visib, np.stack([r[2] for r in ref]))
    depth_dev = be.render_depth((m + 1).tolist(), T, K, (GC.H, GC.W))
    for k in range(n):
        assert int(mask[k].sum()) // 255 == int((depth_dev[k] > 0).sum())
    assert mask.any() and (mask != mask_visib).any()
    # one mask alone, the other alone, neither: the C entry takes NULL for either
    lib = be.lib
    idx, Tn, Kn = np.ascontiguousarray(m), np.ascontiguousarray(T.reshape(n, 12)), np.ascontiguousarray(K.reshape(n, 9))
    only = np.full_like(mask, 7)
    for args, want in (((only.ctypes.data, None), gm), ((None, only.ctypes.data), gv)):
        _lib.check(lib.suo_gt_masks(be._h, n, idx.ctypes.data, Tn.ctypes.data, Kn.ctypes.data, GC.W, GC.H, len(depth), depth.ctypes.data, ii.ctypes.data, 15.0, *args),
                   "suo_gt_masks")
        assert np.array_equal(only, want)
    assert lib.suo_gt_masks(be._h, n, idx.ctypes.data, Tn.ctypes.data, Kn.ctypes.data, GC.W, GC.H, len(depth), depth.ctypes.data, ii.ctypes.data, 15.0, None, None) == 0


def test_second_size_equals_the_numpy_restatement(be):
    """100 x 70 under a camera with fractional cx, cy and fx != fy: a canvas of 300 x 210 (5 x 4 tiles, both last ones partial), the window from x = 100,
    y = 70 -- no multiple of 32."""
    imgs = GC.images_second_size()
    ref2 = _reference(imgs)
    got = _run_info(be, imgs)
    for lab, g, r in zip(GC.labels(imgs), got, ref2):
        print(lab, g)
        assert g == r[0], (lab, g, r[0])
    assert sum(0 < g["visib_fract"] < 1 for g in got) >= 2 and any(g["px_count_all"] == 0 for g in got) and any(g["px_count_valid"] < g["px_count_visib"] for g in got)
    m, T, K, ii, depth = GC.flat(imgs)
    mask, mask_visib = be.gt_masks((m + 1).tolist(), T, K, list(depth), ii.tolist(), GC.DELTA)
    assert np.array_equal(mask, np.stack([r[1] for r in ref2])) and np.array_equal(mask_visib, np.stack([r[2] for r in ref2]))


def test_values_do_not_depend_on_the_batch(be, cases):
    n = len(GC.flat(cases)[0])
    batch = _run_info(be, cases)
    assert _run_info(be, cases) == batch                                        # two calls
    rng = np.random.default_rng(3)
    for order in (np.arange(n)[::-1], rng.permutation(n)):
        got = _run_info(be, cases, order)
        assert [got[int(np.nonzero(order == k)[0][0])] for k in range(n)] == batch
    m, T, K, ii, depth = GC.flat(cases)
    for k in (1, 8, 10, 15, 22, 24):                                           # alone, with its image alone
        one = be.gt_info([int(m[k]) + 1], T[k:k + 1], K[k:k + 1], [depth[ii[k]]], [0], GC.DELTA)
        assert one[0] == batch[k], k
    # more instances than one launch takes (1024): the entry splits them, every copy has the values of the first
    reps = 1024 // n + 2
    big = be.gt_info(np.tile(m + 1, reps).tolist(), np.tile(T, (reps, 1, 1)), np.tile(K, (reps, 1, 1)), list(depth), np.tile(ii, reps).tolist(), GC.DELTA)
    assert len(big) == reps * n > 1024 and big == batch * reps
    m3, T3, K3, ii3 = (np.tile(a, (3,) + (1,) * (a.ndim - 1)) for a in (m, T, K, ii))
    ma, va = be.gt_masks((m + 1).tolist(), T, K, list(depth), ii.tolist(), GC.DELTA)
    mb, vb = be.gt_masks((m3 + 1).tolist()[::-1], T3[::-1], K3[::-1], list(depth), ii3.tolist()[::-1], GC.DELTA)
    assert np.array_equal(mb[::-1], np.tile(ma, (3, 1, 1))) and np.array_equal(vb[::-1], np.tile(va, (3, 1, 1)))


def test_refusals_that_need_a_database_and_odd_test_depth(be, cases):
    lib = be.lib
    m, T, K, ii, depth = GC.flat(cases)
    n = 3
    Tn, Kn = np.ascontiguousarray(T[:n].reshape(n, 12)), np.ascontiguousarray(K[:n].reshape(n, 9))
    counts, bo, bv = np.zeros((n, 3), np.int64), np.zeros((n, 4), np.int32), np.zeros((n, 4), np.int32)

    def call(h, idx, d=depth, n_=n):
        idx = np.ascontiguousarray(idx, np.int32)
        return lib.suo_gt_info(h, n_, idx.ctypes.data, Tn.ctypes.data, Kn.ctypes.data, GC.W, GC.H, len(d), d.ctypes.data, ii[:n].ctypes.data, 15.0, counts.ctypes.data,
                               bo.ctypes.data, bv.ctypes.data)
    assert call(be._h, m[:n]) == 0
    assert call(be._h, [0, len(VC.models()), 0]) == SUO_ERR_ARG and b"model_index[1]" in lib.suo_last_error()
    assert call(be._h, [0, 0, -1]) == SUO_ERR_ARG
    assert call(be._h, m[:n], n_=0) == 0 and lib.suo_gt_info(be._h, 0, None, None, None, GC.W, GC.H, 0, None, None, 15.0, None, None, None) == 0
    bare = bop_eval.BopErrors({1: {"points": VC.models()[0][1]}}, {1: {"diameter": 1.0}})
    assert call(bare._h, [0, 0, 0]) == SUO_ERR_ARG and b"no faces" in lib.suo_last_error()
    bare.close()
    # NaN, negative and infinite test depth follow the formulas and fault nothing: NaN is neither valid nor visible; -d is |d|
    base = depth[ii[0]]
    k = 10                                                                      # near_box: covers most of the image
    plain = be.gt_info([int(m[k]) + 1], T[k:k + 1], K[k:k + 1], [base], [0])[0]
    odd = base.copy()
    odd[:, :40] = np.nan
    odd[:, 40:80] = -base[:, 40:80]
    got = be.gt_info([int(m[k]) + 1], T[k:k + 1], K[k:k + 1], [odd], [0])[0]
    mk, mv = be.gt_masks([int(m[k]) + 1], T[k:k + 1], K[k:k + 1], [odd], [0])
    _, mv0 = be.gt_masks([int(m[k]) + 1], T[k:k + 1], K[k:k + 1], [base], [0])
    assert not mv[0][:, :40].any() and mk[0][:, :40].any()
    assert np.array_equal(mv[0][:, 40:], mv0[0][:, 40:])
    assert got["px_count_all"] == plain["px_count_all"] and got["px_count_visib"] == int(mv[0].sum()) // 255
    assert got["px_count_valid"] == int(((mk[0] > 0) & (odd != 0) & ~np.isnan(odd)).sum())
    inf = np.full_like(base, np.inf)
    got = be.gt_info([int(m[k]) + 1], T[k:k + 1], K[k:k + 1], [inf], [0])[0]
    assert got["px_count_all"] == plain["px_count_all"] and 0 < got["px_count_visib"] <= int(mk[0].sum()) // 255


def test_a_tree_without_gt_info_is_indexed_and_scored(tmp_path):
    desc = bop_tree.build(str(tmp_path), dset="tless", seed=12, n_scenes=1, n_views=1)
    model_dir = os.path.join(desc["data_root"], "models_eval")
    mesh_db = bop.load_mesh_db(model_dir, faces=True)
    VR.add_depth(desc, mesh_db, seed=2)
    split_dir = os.path.join(desc["data_root"], desc["split"])
    (scene_id,) = desc["scenes"]
    sdir = os.path.join(split_dir, f"{scene_id:06d}")
    os.remove(os.path.join(sdir, "scene_gt_info.json"))
    with pytest.raises(FileNotFoundError):
        bop.BopDataset(desc["data_root"], desc["split"], bop_dset="tless", ignore_symmetry=True)
    errors = bop_eval.BopErrors(mesh_db, bop_eval.load_models_info(model_dir))
    out = bop_gt_info.calc_scene_gt_info(errors, split_dir, masks=True, images_per_call=1)
    again = bop_gt_info.calc_scene_gt_info(errors, split_dir, masks=False, write=False)
    assert again == out and list(out) == [scene_id]
    # the values are those of the numpy restatement on the same tree, under the same two conditions
    from PIL import Image
    cam = json.load(open(os.path.join(sdir, "scene_camera.json")))
    gt = json.load(open(os.path.join(sdir, "scene_gt.json")))
    for view, gts in gt.items():
        depth = bop_gt_info.read_depth(sdir, int(view), cam[view]["depth_scale"])
        K = np.array(cam[view]["cam_K"], np.float64).reshape(3, 3)
        for gt_id, g in enumerate(gts):
            T = np.hstack((np.reshape(g["cam_R_m2c"], (3, 3)), np.reshape(g["cam_t_m2c"], (3, 1))))
            o = g["obj_id"]
            want, _, near, margin = GR.gt_info(mesh_db[o]["points"], mesh_db[o]["faces"], T, K, depth, 15, details=True)
            mask, mask_visib, _, near_p = GR.gt_masks(mesh_db[o]["points"], mesh_db[o]["faces"], T, K, depth, 15, details=True)
            assert not near.any() and not near_p.any() and margin > MARGIN, (view, gt_id, margin)
            print(view, gt_id, out[scene_id][int(view)][gt_id])
            assert out[scene_id][int(view)][gt_id] == want, (view, gt_id)
            for kind, w in (("mask", mask), ("mask_visib", mask_visib)):
                im = Image.open(os.path.join(sdir, kind, f"{int(view):06d}_{gt_id:06d}.png"))
                assert im.mode == "L" and np.array_equal(np.asarray(im), w), (kind, view, gt_id)
    # the file is what the script's writer writes, and the readers take it
    with open(os.path.join(sdir, "scene_gt_info.json"), "r") as f:
        text = f.read()
    assert text == bop_gt_info.format_scene_gt_info(out[scene_id]) and {int(k): v for k, v in json.loads(text).items()} == out[scene_id]
    ds = bop.BopDataset(desc["data_root"], desc["split"], bop_dset="tless", ignore_symmetry=True)
    seen = 0
    for view, frame in ds.data[scene_id].items():
        for o, obj in frame["objects"].items():
            (gt_id,) = [k for k, g in enumerate(gt[str(view)]) if g["obj_id"] == o]
            assert obj["bbox"] == out[scene_id][view][gt_id]["bbox_visib"] and out[scene_id][view][gt_id]["visib_fract"] >= 0.1
            assert os.path.exists(obj["mask_path"])
            seen += 1
    assert seen > 0
    meter = bop_eval.Bop19Meter.from_dataset_tree(errors, split_dir, ds.targets_filename, 640)
    assert meter.scene_gt_info[scene_id] == out[scene_id]
    errors.close()
