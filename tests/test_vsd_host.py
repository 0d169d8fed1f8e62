"""Host side of the BOP-19 VSD row (N6) against the toolkit's recorded results (tests/golden/vsd_golden.npz, made by tests/golden/make_vsd_golden.py), and
the numpy rasteriser of tests/vsd_ref.py at the one place where its rules can be checked by hand.  No GPU."""
import os

import numpy as np
import pytest

from suo_slam_amd import bop, bop_eval
from tests import bop_tree
from tests import vsd_ref as VR
from tests.golden import vsd_cases as VC

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "vsd_golden.npz"))


def test_load_ply_mesh_equals_the_toolkit_loader(tmp_path):
    desc = bop_tree.build(str(tmp_path), **VC.PLY_TREE)
    model_dir = os.path.join(desc["data_root"], "models_eval")
    for oid in (1, 2):                                                # binary little endian, ascii
        path = os.path.join(model_dir, f"obj_{oid:06d}.ply")
        pts, faces = bop.load_ply_mesh(path)
        assert pts.dtype == np.float32 and faces.dtype == np.int32 and faces.shape[1] == 3
        assert np.array_equal(pts.astype(np.float64), GOLD[f"ply{oid}_pts"])
        assert np.array_equal(faces.astype(np.float64), GOLD[f"ply{oid}_faces"])
        assert np.array_equal(bop.load_ply_points(path), GOLD[f"ply{oid}_pts"])
    plain, with_faces = bop.load_mesh_db(model_dir), bop.load_mesh_db(model_dir, faces=True)
    assert all("faces" not in v for v in plain.values())
    for o, v in with_faces.items():
        assert set(v) == set(plain[o]) | {"faces"} and np.array_equal(v["points"], plain[o]["points"])
    assert np.array_equal(with_faces[1]["faces"].astype(np.float64), GOLD["ply1_faces"])


def test_load_ply_mesh_uint_lists_and_other_properties(tmp_path):
    import struct
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    faces = [(0, 1, 2), (0, 2, 3)]
    hdr = ("ply\nformat {} 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n"
           "element face 2\nproperty list uchar uint vertex_indices\nproperty uchar flag\nend_header\n")
    with open(tmp_path / "b.ply", "wb") as f:
        f.write(hdr.format("binary_little_endian").encode())
        for p in pts:
            f.write(struct.pack("<fffB", *p, 7))
        for t in faces:
            f.write(struct.pack("<BIIIB", 3, *t, 1))
    with open(tmp_path / "a.ply", "wb") as f:
        f.write(hdr.format("ascii").encode())
        for p in pts:
            f.write((" ".join(str(float(v)) for v in p) + " 7\n").encode())
        for t in faces:
            f.write(("3 " + " ".join(map(str, t)) + " 1\n").encode())
    for name in ("a.ply", "b.ply"):
        p, fc = bop.load_ply_mesh(str(tmp_path / name))
        assert np.array_equal(p, pts) and np.array_equal(fc, np.array(faces, np.int32))
    with open(tmp_path / "q.ply", "wb") as f:
        f.write(hdr.format("ascii").encode())
        f.write(b"0 0 0 7\n1 0 0 7\n0 1 0 7\n0 0 1 7\n4 0 1 2 3 1\n3 0 1 2 1\n")
    with pytest.raises(ValueError, match="triangular"):
        bop.load_ply_mesh(str(tmp_path / "q.ply"))


def test_load_ply_mesh_binary_file_with_the_uint_list_alone(tmp_path):
    """The usual binary layout -- a count byte and three indices per face, nothing else on the face element -- with ``uint`` indices, and its ascii twin;
    an index that does not fit int32 is refused, not wrapped."""
    import struct
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    faces = [(0, 1, 2), (3, 2, 1), (0, 3, 1)]
    for typ, code in (("uint", "I"), ("int", "i")):
        hdr = ("ply\nformat {} 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
               f"element face 3\nproperty list uchar {typ} vertex_indices\nend_header\n")
        with open(tmp_path / "b.ply", "wb") as f:
            f.write(hdr.format("binary_little_endian").encode())
            for p in pts:
                f.write(struct.pack("<fff", *p))
            for t in faces:
                f.write(struct.pack("<B" + 3 * code, 3, *t))
        with open(tmp_path / "a.ply", "wb") as f:
            f.write(hdr.format("ascii").encode())
            for p in pts:
                f.write((" ".join(str(float(v)) for v in p) + "\n").encode())
            for t in faces:
                f.write(("3 " + " ".join(map(str, t)) + "\n").encode())
        for name in ("a.ply", "b.ply"):
            p, fc = bop.load_ply_mesh(str(tmp_path / name))
            assert fc.dtype == np.int32 and np.array_equal(p, pts) and np.array_equal(fc, np.array(faces, np.int32)), (typ, name)
    with open(tmp_path / "big.ply", "wb") as f:                        # the header left by the loop: int; write the uint one again
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
                 "element face 1\nproperty list uchar uint vertex_indices\nend_header\n").encode())
        for p in pts:
            f.write(struct.pack("<fff", *p))
        f.write(struct.pack("<BIII", 3, 0, 1, 2 ** 31))
    with pytest.raises(ValueError, match="int32"):
        bop.load_ply_mesh(str(tmp_path / "big.ply"))
    with open(tmp_path / "big_a.ply", "wb") as f:
        f.write(("ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
                 "element face 1\nproperty list uchar uint vertex_indices\nend_header\n0 0 0\n1 0 0\n0 1 0\n0 0 1\n3 0 1 4294967295\n").encode())
    with pytest.raises(ValueError, match="int32"):
        bop.load_ply_mesh(str(tmp_path / "big_a.ply"))


def test_read_depth_is_the_float32_product(tmp_path):
    desc = bop_tree.build(str(tmp_path), dset="tless", seed=4, n_scenes=1, n_views=1)
    VR.add_depth(desc, bop.load_mesh_db(os.path.join(desc["data_root"], "models_eval"), faces=True), seed=1)
    from PIL import Image
    ds = bop.BopDataset(desc["data_root"], desc["split"], bop_dset="tless", ignore_symmetry=True)
    s = ds.scene_ids()[0]
    v = ds.view_ids(s)[0]
    d = ds.read_depth(s, v)
    raw = np.asarray(Image.open(os.path.join(desc["data_root"], desc["split"], f"{s:06d}", "depth", f"{v:06d}.png")))
    assert raw.dtype == np.uint16 and d.dtype == np.float32 and d.shape == (480, 640)
    want = raw.astype(np.float32)
    want *= 0.1                                                       # eval_calc_errors.py:241-242: in place, so the product is float32
    assert np.array_equal(d, want) and (d == 0).any() and (d == np.float32(4200) * np.float32(0.1)).any() and ((d > 500) & (d < 1400)).any()


def test_sphere_gate_equals_the_toolkit():
    got = [bop_eval.overlapping_sphere_projections(r, p1, p2) for r, p1, p2 in VC.SPHERE_CASES]
    assert got == GOLD["sphere"].tolist() and True in got and False in got


def test_constants():
    assert np.array_equal(bop_eval.VSD_TAUS, np.arange(0.05, 0.51, 0.05)) and np.array_equal(bop_eval.VSD_THRESHOLDS, bop_eval.VSD_TAUS)
    assert bop_eval.VSD_DELTAS["tless"] == 15 and bop_eval.VSD_DELTAS["ycbv"] == 15 and bop_eval.VSD_DELTAS["itodd"] == 5 and len(bop_eval.VSD_DELTAS) == 11


def test_numpy_vsd_equals_the_toolkit_errors():
    models = VC.models()
    kinds = set()
    for p, want in zip(VC.vsd_pairs(), GOLD["vsd_errors"]):
        _, P, F, diam = models[p["m"]]
        de, dg = VR.render_depth(P, F, p["Te"], p["K"], VC.W, VC.H), VR.render_depth(P, F, p["Tg"], p["K"], VC.W, VC.H)
        errors, counts = VR.vsd_from_depth(de, dg, p["test"], p["K"], VC.DELTA, VC.TAUS, p["normalized"], diam)
        assert errors == want.tolist(), p["label"]
        union, inter = counts[:2]
        if union:
            assert errors == [(c + union - inter) / float(union) for c in counts[2:]]
        kinds.add(("empty" if union == 0 else "zero" if max(errors) == 0 else "one" if min(errors) == 1 else "between", p["normalized"]))
    assert {k for k, _ in kinds} >= {"empty", "zero", "between"}
    assert {n for _, n in kinds} == {True, False}


class _Table:
    """A Bop19Meter whose VSD error table is given: only its matching and recall run."""

    def __init__(self):
        gt_obj_ids, gt_valid, inst_count, ests = VC.vsd_match_case()
        self.gt_obj_ids, self.gt_valid = gt_obj_ids, gt_valid
        self.table = {}
        for (im, o), rows in ests.items():
            kept = bop_eval.top_estimates(rows, inst_count[(im, o)])
            self.table.setdefault(im, {})[o] = [{"est_id": i, "score": r["score"], "errors": r["errors"]} for i, r in kept]


def test_vsd_matching_and_recall_equal_the_toolkit():
    c = _Table()
    ims = sorted(c.gt_obj_ids)
    for t in range(len(VC.TAUS)):
        for k, th in enumerate(bop_eval.VSD_THRESHOLDS):
            est, tp, tars = [], 0, 0
            for im in ims:
                errs = {o: [{"est_id": r["est_id"], "score": r["score"], "errors": {g: e[t] for g, e in r["errors"].items()}} for r in rows]
                        for o, rows in c.table.get(im, {}).items()}
                e = bop_eval.match_poses_image(c.gt_obj_ids[im], c.gt_valid[im], errs, float(th))
                est += e
                tars += sum(c.gt_valid[im])
                tp += sum(1 for g, v in enumerate(c.gt_valid[im]) if v and e[g] != -1)
            assert est == GOLD["match_vsd_est"][t, k].tolist(), (t, k)
            assert tp / float(tars) == GOLD["match_vsd_recall"][t, k]
    assert GOLD["match_vsd_recall"].min() < GOLD["match_vsd_recall"].max()


def test_meter_without_a_loader_reports_what_it_reported(monkeypatch):
    """depth_loader=None: result() has exactly the keys of before and never asks for VSD."""
    from tests import bop_errors_ref
    from tests.golden import bop19_cases as BC
    pts = {1: {"points": BC.model_points(1)}}
    info = {1: {"diameter": 180.0}}
    errs = bop_errors_ref.RefErrors(pts, info)
    T = np.hstack((np.eye(3), [[0.0], [0.0], [600.0]]))
    gt = {1: {5: [{"obj_id": 1, "cam_R_m2c": np.eye(3).ravel().tolist(), "cam_t_m2c": [1.0, 0.0, 600.0]}]}}
    gi = {1: {5: [{"visib_fract": 0.9}]}}
    tg = [{"scene_id": 1, "im_id": 5, "obj_id": 1, "inst_count": 1}]
    m = bop_eval.Bop19Meter(errs, tg, gt, gi, 640)
    m.add(1, 5, 1, 1.0, T, np.array(bop_tree.K_YCBV).reshape(3, 3))
    assert set(m.result()) == {"mssd", "mspd", "n_targets", "n_estimates", "max_sym_disc_step"}

    class Vsd(bop_errors_ref.RefErrors):
        def vsd(self, obj_ids, T_est, T_gt, K, depth_images, image_index, delta=15, taus=None, normalized=True):
            assert delta == 7 and normalized and depth_images[0].shape == (4, 4)
            return np.full((len(obj_ids), len(taus)), 0.25)
    m = bop_eval.Bop19Meter(Vsd(pts, info), tg, gt, gi, 640, depth_loader=lambda s, im: np.zeros((4, 4), np.float32), vsd_delta=7)
    m.add(1, 5, 1, 1.0, T, np.array(bop_tree.K_YCBV).reshape(3, 3))
    r = m.result()
    assert np.array(r["vsd"]["recalls"]).shape == (10, 10)
    assert r["vsd"]["recalls"][0] == [0.0] * 5 + [1.0] * 5                      # 0.25 < th from 0.3 on
    assert r["vsd"]["ar"] == float(np.mean(r["vsd"]["recalls"])) and r["ar"] == float(np.mean([r["vsd"]["ar"], r["mssd"]["ar"], r["mspd"]["ar"]]))


def test_rasteriser_rectangle_through_sample_points():
    """fx = fy = 64, Z = 4, vertices at multiples of 1/32 mm: every coordinate, edge function and depth is exact.  The rectangle's edges run through sample
    points (x + 0.5, y + 0.5): the samples on its left and top edges are covered, those on its right and bottom edges are not, for either winding and
    either diagonal, and each covered sample is covered by exactly one of the two triangles."""
    K = np.array([[64.0, 0.0, 8.0], [0.0, 64.0, 8.0], [0.0, 0.0, 1.0]])
    T = np.hstack((np.eye(3), [[0.0], [0.0], [4.0]]))
    # u = 16 x + 8, v = 16 y + 8: the rectangle u in [2.5, 10.5], v in [3.5, 7.5]
    corners = [((2.5 - 8) / 16, (3.5 - 8) / 16), ((10.5 - 8) / 16, (3.5 - 8) / 16), ((10.5 - 8) / 16, (7.5 - 8) / 16), ((2.5 - 8) / 16, (7.5 - 8) / 16)]
    pts = np.array([[x, y, 0.0] for x, y in corners], np.float32)
    want = np.zeros((12, 16), np.float32)
    want[3:7, 2:10] = 4.0
    for faces in ([(0, 1, 2), (0, 2, 3)], [(0, 2, 1), (0, 2, 3)], [(1, 2, 3), (1, 3, 0)], [(3, 2, 1), (0, 1, 3)]):
        d, near = VR.render_depth(pts, np.array(faces), T, K, 16, 12, with_near=True)
        assert np.array_equal(d, want), faces
        assert near[3:8, 2].all() and near[3, 2:11].all()                 # the samples on the edges are the ones a tolerance would skip
        a = VR.render_depth(pts, np.array(faces[:1]), T, K, 16, 12) > 0
        b = VR.render_depth(pts, np.array(faces[1:]), T, K, 16, 12) > 0
        assert not (a & b).any() and np.array_equal(a | b, want > 0)
