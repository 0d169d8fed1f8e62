"""The visualisation on the device (csrc/viz.hip, suo_viz_view) against tests/viz_ref.py, the numpy statement of include/suo_hip.h's rules: every byte, on the
designed views of tests/golden/viz_cases.py and on primitive lists long enough to cross the kernels' LDS chunk; against the reference's own pictures
(tests/golden/viz_golden.npz); and through ObjectSLAM.collect_results(no_viz=False) and Evaluator(no_viz=False)."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from tests import slam_states as SS
from tests import viz_ref
from tests.golden import treeio, viz_cases
from tests.test_viz_ref import compare_with_golden

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    return treeio.load(os.path.join(HERE, "golden", "viz_golden.npz"))


@pytest.fixture(scope="module")
def cases():
    """name -> (case, primitives, the numpy picture): computed once, shared, never modified."""
    from suo_slam_amd import viz
    kp_cols = viz.colour_tables()[0]
    out = {}
    for c in viz_cases.all_cases():
        prims = viz.view_primitives(viz_cases.install(types.SimpleNamespace(), c), viz_cases.VIEW)
        out[c["name"]] = (c, prims, viz_ref.render(c["frame"], prims, c["meshes"], kp_cols))
    return out


def visualizer(case):
    from suo_slam_amd import viz
    return viz.Visualizer({o: {"points": p} for o, p in case["meshes"].items()}, case["H"], case["W"])


@pytest.mark.parametrize("name", ["empty", "keypoints", "ellipses", "priors", "overlay", "all"])
def test_view_equals_the_rules_and_the_reference_s_picture(cases, golden, name):
    case, prims, want = cases[name]
    vz = visualizer(case)
    got = vz.render(case["frame"], prims)
    vz.close()
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, f"{len(bad)} pixels differ from tests/viz_ref.py, the first at (y, x) = {bad[0].tolist()} (panel {bad[0][1] // case['W']})"
    compare_with_golden(got, golden["cases"][name]["viz"], case, prims)         # exact outside prior windows, one level inside


def synthetic_prims(H, W, seed, n_kp, n_stamp, n_box):
    """Primitive lists that build_primitives would not make: more than one LDS chunk (128) of keypoints and of stamps, centres off the canvas (the device
    clips), ellipses at exactly 0, 90, 45 and 180 degrees, degenerate and huge half-axes, boxes with x2 < x1."""
    rng = np.random.default_rng(seed)
    col = lambda: int(rng.integers(0, 1 << 24))                                 # noqa: E731
    kp, ang = [], []
    for i in range(n_kp):
        has = int(i % 3 != 0)
        A, B = ((0, 0), (1, 0), (0, 7), (1, 1), (2, 2), (2, 1), (30, 3), (400, 250))[i % 8] if i < 32 else (int(rng.integers(0, 25)), int(rng.integers(0, 25)))
        kp.append([int(rng.integers(-12, W + 12)), int(rng.integers(-12, H + 12)), int(rng.integers(0, 12)), int(rng.integers(0, 9)), col(), has, A if has else 0, B if has else 0])
        ang.append((0.0, 90.0, 45.0, 180.0, -90.0)[i % 5] if i < 40 else float(rng.uniform(-180, 180)))
    stamp = [[int(rng.integers(0, 41)), int(rng.integers(-80, W)), int(rng.integers(-80, H))] + sorted(rng.integers(0, W + 1, 2).tolist()) + sorted(rng.integers(0, H + 1, 2).tolist()) + [i]
             for i in range(n_stamp)]
    box = [[int(rng.integers(-20, W + 20)), int(rng.integers(-20, H + 20)), int(rng.integers(-20, W + 20)), int(rng.integers(-20, H + 20)), col()] for _ in range(n_box)]
    return {"box": np.array(box, np.int64).reshape(-1, 5), "stamp": np.array(stamp, np.int64).reshape(-1, 8), "kp": np.array(kp, np.int64).reshape(-1, 8),
            "kp_angle": np.array(ang), "overlay": []}


@pytest.mark.parametrize("H,W,n_kp,n_stamp,n_box", [(117, 150, 300, 260, 64), (5, 3, 129, 128, 3), (64, 256, 128, 129, 0), (1, 70, 656, 656, 1)])
def test_long_primitive_lists_cross_the_lds_chunk(H, W, n_kp, n_stamp, n_box):
    from suo_slam_amd import viz
    frame = viz_cases.frame(H, W, 11)
    prims = synthetic_prims(H, W, 100 + n_kp, n_kp, n_stamp, n_box)
    want = viz_ref.render(frame, prims, {}, viz.colour_tables()[0])
    vz = viz.Visualizer({}, H, W)
    got = vz.render(frame, prims)
    vz.close()
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, f"{len(bad)} pixels differ, the first at (y, x) = {bad[0].tolist()}"
    assert (want[:, W:2 * W] != frame).any()


def test_a_second_view_on_the_same_handle_leaves_nothing_behind(cases):
    """overlay -> ellipses -> overlay on one 160 x 120 handle: the owner plane of the first call must not show in the second, nor the second's keypoints in the
    third."""
    (c1, p1, w1), (c2, p2, w2) = cases["overlay"], cases["ellipses"]
    assert (c1["H"], c1["W"]) == (c2["H"], c2["W"])
    vz = visualizer(c1)
    for case, prims, want in ((c1, p1, w1), (c2, p2, w2), (c1, p1, w1)):
        assert np.array_equal(vz.render(case["frame"], prims), want), case["name"]
    vz.close()


def test_host_refusals_launch_nothing(cases):
    import torch
    from suo_slam_amd import _lib, viz
    lib = _lib.lib()
    h = C.c_void_p()
    for H, W in ((0, 5), (5, 0), (65536, 32768), (-1, 4)):
        assert lib.suo_viz_create(H, W, C.byref(h)) == 1 and not h.value           # SUO_ERR_ARG; 65536 x 32768 = 2^31
    case, prims, want = cases["overlay"]
    vz = visualizer(case)
    frame = torch.from_numpy(case["frame"]).cuda()
    out = torch.full((case["H"], 3 * case["W"], 3), 77, dtype=torch.uint8, device="cuda")

    def call(p, db=True, frame_ptr=None, out_ptr=None):
        d, keep = vz.descriptor(p)
        d.frame = frame.data_ptr() if frame_ptr is None else frame_ptr
        return lib.suo_viz_view(vz._h, C.byref(d), vz._db if db else None, out.data_ptr() if out_ptr is None else out_ptr, _lib.current_stream_ptr())

    def grown(key, n, row):
        q = dict(prims)
        q[key] = np.array([row] * n, np.int64)
        if key == "kp":
            q["kp_angle"] = np.zeros(n)
        return q
    ov65 = dict(prims, overlay=[prims["overlay"][0]] * 65)
    bad_channel = grown("stamp", 1, [41, 0, 0, 0, 10, 0, 10, 1])
    bad_radius = grown("kp", 1, [5, 5, -1, 3, 0, 0, 0, 0])
    bad_axis = grown("kp", 1, [5, 5, 3, 3, 0, 1, (1 << 20) + 1, 2])
    refused = [grown("kp", 657, [5, 5, 3, 2, 9, 0, 0, 0]), grown("stamp", 657, [0, 0, 0, 0, 10, 0, 10, 1]), grown("box", 65, [1, 1, 9, 9, 5]), ov65, bad_channel, bad_radius, bad_axis]
    for p in refused:
        assert call(p) == 1
        assert b"suo_viz_view" in lib.suo_last_error()
    assert call(prims, db=False) == 1                                               # overlays without a mesh database
    assert call(prims, frame_ptr=0) == 1 and call(prims, out_ptr=0) == 1
    d, keep = vz.descriptor(prims)
    d.frame = frame.data_ptr()
    past = np.full(len(prims["overlay"]), len(case["meshes"]), np.int32)           # a model index one past the database
    d.overlay_model = past.ctypes.data
    assert lib.suo_viz_view(vz._h, C.byref(d), vz._db, out.data_ptr(), _lib.current_stream_ptr()) == 1
    torch.cuda.synchronize()
    assert bool((out == 77).all())                                                  # nothing was written
    assert call(grown("kp", 656, [5, 5, 3, 2, 9, 0, 0, 0])) == 0                    # the limit itself is taken
    torch.cuda.synchronize()
    assert call(prims) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    vz.close()


@pytest.fixture(scope="module")
def slam_run():
    """A short --debug_gt_kp SLAM sequence (symmetric objects: prior detections) on 96 x 128 frames, collected with and without pictures."""
    from suo_slam_amd.object_slam import ObjectSLAM
    seq = SS.make_sequence(seed=8100, n_views=4, n_obj=4, sym_every=2)
    rng = np.random.default_rng(5)
    mesh_db = {o: dict(m, points=rng.uniform(-40, 40, (500, 3)).astype(np.float32)) for o, m in seq["mesh_db"].items()}
    S = np.diag([0.2, 0.2, 1.0])                                                    # the sequence's 640 x 480 camera, scaled to a 128 x 96 frame
    s = ObjectSLAM(None, mesh_db, debug_gt_kp=True, manual_kp_std=0.01, global_opt_every=3, viz_cov=True)
    s._rng = np.random.RandomState(1)
    for i, vw in enumerate(seq["views"]):
        s.process_view(vw["view_id"], viz_cases.frame(96, 128, 20 + i), S @ vw["K"], vw["obj_ids"].copy(), vw["bboxes"].copy() * 0.2, vw["model_kps"], vw["model_kps_masks"],
                       vw["kp_masks"], uv_gt=vw["uv_gt"])
    return s, mesh_db, s.collect_results(no_viz=True), s.collect_results(no_viz=False)


def test_collect_results_pictures_equal_the_rules(slam_run):
    """Fails on the parent commit, where no_viz is ignored and the key is absent."""
    from suo_slam_amd import viz
    s, mesh_db, _, with_viz = slam_run
    n_stamps = 0
    for v in s.view_ids:
        img = with_viz[v]["viz"]
        assert img.dtype == np.uint8 and img.shape == (96, 3 * 128, 3)
        prims = viz.view_primitives(s, v)
        n_stamps += len(prims["stamp"])
        assert not prims["kp"][:, 5].any()                                          # debug_gt_kp means no_network_cov: viz_cov draws no ellipses (:239-268)
        want = viz_ref.render(s.images[v], prims, {o: m["points"] for o, m in mesh_db.items()}, viz.colour_tables()[0])
        assert np.array_equal(img, want), v
        assert (img[:, 256:] != s.images[v]).any()                                  # the meshes are on the right panel
    assert n_stamps > 0                                                             # the symmetric objects' priors were blended in


def test_collect_results_without_pictures_is_what_it_was(slam_run):
    s, _, plain, with_viz = slam_run
    assert list(plain) == list(with_viz) == s.view_ids
    for v in plain:
        assert set(plain[v]) == {"poses"} and set(with_viz[v]) == {"poses", "viz"}
        assert list(plain[v]["poses"]) == list(with_viz[v]["poses"])
        for o, r in plain[v]["poses"].items():
            assert set(r) == {"T_OtoC", "score"} and r["score"] == with_viz[v]["poses"][o]["score"]
            assert (r["T_OtoC"] is None) == (with_viz[v]["poses"][o]["T_OtoC"] is None)
            if r["T_OtoC"] is not None:
                assert np.array_equal(r["T_OtoC"], with_viz[v]["poses"][o]["T_OtoC"])
    s.do_viz_extra = True
    with pytest.raises(NotImplementedError):
        s.collect_results(no_viz=False)
    s.do_viz_extra = False


def test_evaluator_writes_one_png_per_view(tmp_path):
    from PIL import Image
    from suo_slam_amd import evaluator
    from tests import bop_tree
    desc = bop_tree.build(str(tmp_path), dset="ycbv", seed=23, n_scenes=1, n_views=2)
    ev = evaluator.Evaluator("ycbv", desc["data_root"], None, nviews=1, debug_gt_kp=True, out_dir=str(tmp_path / "out"), no_viz=False)
    seen = []
    collect = ev.object_slam.collect_results

    def spy(**kw):                                                                  # what the evaluator was handed, to compare the files with
        res = collect(**kw)
        seen.extend(r["viz"] for r in res.values())
        return res
    ev.object_slam.collect_results = spy
    out = ev.run()
    viz_dir = os.path.join(os.path.dirname(out["csv_path"]), "viz_images")
    ds = ev.dataset
    names = [f"scene_{s}_{j:06d}.png" for s in ds.scene_ids() for j, _ in enumerate(ds.view_ids(s))]
    assert sorted(os.listdir(viz_dir)) == sorted(names) and len(seen) == len(names) == 2
    for name, img in zip(names, seen):
        png = np.asarray(Image.open(os.path.join(viz_dir, name)))
        assert png.shape == img.shape and img.shape[1] % 3 == 0 and np.array_equal(png[..., ::-1], img)        # the file is RGB, the array BGR
    with pytest.raises(ValueError):
        evaluator.Evaluator("ycbv", desc["data_root"], None, nviews=1, debug_gt_kp=True, out_dir=str(tmp_path / "o2"), no_viz=False, frames_per_call=2)
    # SfM with two views a call: their pictures stacked vertically (evaluate.py:204-213), into the directory asked for
    ev2 = evaluator.Evaluator("ycbv", desc["data_root"], None, nviews=2, debug_gt_kp=True, out_dir=str(tmp_path / "o3"), no_viz=False, viz_dir=str(tmp_path / "pics"))
    seen2 = []
    collect2 = ev2.object_slam.collect_results

    def spy2(**kw):
        res = collect2(**kw)
        seen2.append(np.concatenate([res[v]["viz"] for v in ev2.object_slam.view_ids], axis=0))
        return res
    ev2.object_slam.collect_results = spy2
    ev2.run()
    assert sorted(os.listdir(tmp_path / "pics")) == sorted(names) and len(seen2) == 2
    for name, img in zip(names, seen2):
        png = np.asarray(Image.open(tmp_path / "pics" / name))
        assert png.shape == (2 * seen[0].shape[0], seen[0].shape[1], 3) and np.array_equal(png[..., ::-1], img)
