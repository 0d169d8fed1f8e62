"""The depth rasteriser and the VSD error kernel (csrc/raster.hip, csrc/eval_vsd.hip, row N6) on the device, through the C ABI.

Yardsticks: the fp64 numpy rasteriser of tests/vsd_ref.py (written from the rules of include/suo_hip.h) and the toolkit's recorded VSD errors
(tests/golden/vsd_golden.npz).  Images are 160 x 96 -- 3 x 2 tiles, the last column and row partial -- with objects on a tile corner, across the image border
and wholly outside it (tests/golden/vsd_cases.py).

Tolerances.  Coverage is compared at every pixel but those at which an edge function of a candidate triangle lies within 1e-9 of zero relative to the
triangle's doubled area in the reference (the two implementations round their screen coordinates alike, so this guards against a difference of a few 2^-53
only); their share must stay below 0.1 % of an image, which the reference alone is checked to meet.  Depth at a covered pixel is one rounding to float32
of fp64 values that differ by ~1e-15 relative: at most one float32 ulp.  The error kernel counts integers: counts are compared exactly, and errors -- one
fp64 division of the same integers -- bit for bit with the toolkit's."""
import ctypes as C
import os

import numpy as np
import pytest

from suo_slam_amd import _lib
from tests import vsd_ref as VR
from tests.golden import vsd_cases as VC

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vsd_golden.npz"))
SUO_ERR_ARG = 1


class Db:
    """A mesh database handle over the models of tests/golden/vsd_cases.py, with their faces."""

    def __init__(self, models=None, faces=True):
        self.lib = _lib.lib()
        self.models = models if models is not None else VC.models()
        clouds = [np.ascontiguousarray(m[1], np.float32) for m in self.models]
        n_pts = np.array([len(c) for c in clouds], np.int32)
        allpts = np.ascontiguousarray(np.concatenate(clouds, 0))
        self.h = C.c_void_p()
        _lib.check(self.lib.suo_mesh_db_create(len(clouds), n_pts.ctypes.data, allpts.ctypes.data, C.byref(self.h)), "suo_mesh_db_create")
        if faces:
            _lib.check(self.set_faces([m[2] for m in self.models]), "suo_mesh_db_set_faces")

    def set_faces(self, tris):
        tris = [np.ascontiguousarray(t, np.int32).reshape(-1, 3) for t in tris]
        n_faces = np.array([len(t) for t in tris], np.int32)
        flat = np.ascontiguousarray(np.concatenate(tris + [np.zeros((1, 3), np.int32)], 0))
        return self.lib.suo_mesh_db_set_faces(self.h, n_faces.ctypes.data, flat.ctypes.data)

    def render_rc(self, items, w=VC.W, h=VC.H):
        """items: [(model, T [3,4], K [3,3])] -> (return code, float32 [n,h,w])."""
        n = len(items)
        idx = np.array([it[0] for it in items], np.int32)
        T = np.ascontiguousarray(np.stack([np.asarray(it[1], np.float64) for it in items]).reshape(n, 12)) if n else np.zeros((1, 12))
        K = np.ascontiguousarray(np.stack([np.asarray(it[2], np.float64) for it in items]).reshape(n, 9)) if n else np.zeros((1, 9))
        out = np.full((max(n, 1), h, w), -7.0, np.float32)
        rc = self.lib.suo_render_depth(self.h, n, idx.ctypes.data, T.ctypes.data, K.ctypes.data, w, h, out.ctypes.data)
        return rc, out[:n]

    def render(self, items, w=VC.W, h=VC.H):
        rc, out = self.render_rc(items, w, h)
        _lib.check(rc, "suo_render_depth")
        return out

    def vsd_poses(self, pairs, tests, image_index, w=VC.W, h=VC.H, taus=VC.TAUS):
        """pairs: [(model, Te, Tg, K, normalized diameter or None)] -> (errors, counts)."""
        n = len(pairs)
        idx = np.array([p[0] for p in pairs], np.int32)
        Te, Tg, K = (np.ascontiguousarray(np.stack([np.asarray(p[j], np.float64) for p in pairs]).reshape(n, -1)) for j in (1, 2, 3))
        norm = pairs[0][4] is not None
        diam = np.array([p[4] if norm else 1.0 for p in pairs], np.float64)
        tests = np.ascontiguousarray(tests, np.float32)
        ii = np.ascontiguousarray(image_index, np.int32)
        taus = np.ascontiguousarray(taus, np.float64)
        e, c = np.full((n, len(taus)), -1.0), np.full((n, 2 + len(taus)), -1, np.int64)
        rc = self.lib.suo_pose_errors_vsd(self.h, n, idx.ctypes.data, Te.ctypes.data, Tg.ctypes.data, K.ctypes.data, w, h, len(tests), tests.ctypes.data,
                                          ii.ctypes.data, float(VC.DELTA), len(taus), taus.ctypes.data, int(norm), diam.ctypes.data, e.ctypes.data, c.ctypes.data)
        _lib.check(rc, "suo_pose_errors_vsd")
        return e, c

    def close(self):
        self.lib.suo_mesh_db_destroy(self.h)


def vsd_from_depth(de, dg, tests, image_index, K, normalized, diam, taus=VC.TAUS, delta=VC.DELTA):
    lib = _lib.lib()
    n, h, w = de.shape
    de, dg, tests = (np.ascontiguousarray(a, np.float32) for a in (de, dg, tests))
    ii = np.ascontiguousarray(image_index, np.int32)
    K = np.ascontiguousarray(np.asarray(K, np.float64).reshape(n, 9))
    diam = np.ascontiguousarray(diam, np.float64)
    taus = np.ascontiguousarray(taus, np.float64)
    e, c = np.full((n, len(taus)), -1.0), np.full((n, 2 + len(taus)), -1, np.int64)
    _lib.check(lib.suo_vsd_from_depth(n, w, h, de.ctypes.data, dg.ctypes.data, len(tests), tests.ctypes.data, ii.ctypes.data, K.ctypes.data, float(delta),
                                      len(taus), taus.ctypes.data, int(normalized), diam.ctypes.data, e.ctypes.data, c.ctypes.data), "suo_vsd_from_depth")
    return e, c


@pytest.fixture(scope="module")
def db():
    d = Db()
    yield d
    d.close()


@pytest.fixture(scope="module")
def ref_renders():
    """The numpy renders of the render cases, computed once: [(label, depth, near mask)]."""
    models = VC.models()
    return [(lab,) + VR.render_depth(models[m][1], models[m][2], T, K, VC.W, VC.H, with_near=True) for lab, m, T, K in VC.render_cases()]


@pytest.fixture(scope="module")
def ref_pairs():
    """The numpy renders of the VSD pairs, computed once: [(pair, depth_est, depth_gt, diameter)]."""
    models = VC.models()
    out = []
    for p in VC.vsd_pairs():
        _, P, F, diam = models[p["m"]]
        out.append((p, VR.render_depth(P, F, p["Te"], p["K"], VC.W, VC.H), VR.render_depth(P, F, p["Tg"], p["K"], VC.W, VC.H), diam))
    return out


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_render_equals_the_numpy_rasteriser(db, ref_renders):
    cases = VC.render_cases()
    got = db.render([(m, T, K) for _, m, T, K in cases])
    drawn = 0
    for (lab, want, near), g in zip(ref_renders, got):
        assert near.mean() <= 1e-3, (lab, near.mean())                          # the reference alone: few samples sit on an edge
        cmp = ~near
        assert np.array_equal((g > 0)[cmp], (want > 0)[cmp]), (lab, int(((g > 0) != (want > 0))[cmp].sum()))
        both = cmp & (g > 0) & (want > 0)
        worst = int(_ulps(g[both], want[both]).max()) if both.any() else 0
        print(lab, "covered", int((want > 0).sum()), "near", int(near.sum()), "max ulp", worst, "bit-equal", bool(np.array_equal(g, want)))
        assert worst <= 1, (lab, worst)
        assert (g[~(g > 0)] == 0).all()
        drawn += int((want > 0).sum())
    labels = [c[0] for c in cases]
    assert (got[labels.index("outside")] == 0).all() and (got[labels.index("near_box")] > 0).sum() > 5000 and drawn > 20000


def test_rectangle_through_sample_points_is_bit_equal():
    K = np.array([[64.0, 0.0, 8.0], [0.0, 64.0, 8.0], [0.0, 0.0, 1.0]])
    T = np.hstack((np.eye(3), [[0.0], [0.0], [4.0]]))
    corners = [((2.5 - 8) / 16, (3.5 - 8) / 16), ((10.5 - 8) / 16, (3.5 - 8) / 16), ((10.5 - 8) / 16, (7.5 - 8) / 16), ((2.5 - 8) / 16, (7.5 - 8) / 16)]
    pts = np.array([[x, y, 0.0] for x, y in corners], np.float32)
    want = np.zeros((12, 16), np.float32)
    want[3:7, 2:10] = 4.0                                                       # left and top samples covered, right and bottom not
    for faces in ([(0, 1, 2), (0, 2, 3)], [(0, 2, 1), (0, 2, 3)], [(1, 2, 3), (1, 3, 0)], [(3, 2, 1), (0, 1, 3)]):
        d = Db([("rect", pts, np.array(faces, np.int32), 1.0)])
        got = d.render([(0, T, K)], 16, 12)[0]
        d.close()
        assert np.array_equal(got, want) and np.array_equal(got, VR.render_depth(pts, np.array(faces), T, K, 16, 12)), faces


def test_a_render_has_the_same_bits_alone_in_a_batch_and_reversed(db):
    cases = [(m, T, K) for _, m, T, K in VC.render_cases()][:7]
    batch = db.render(cases)
    assert np.array_equal(db.render(cases[::-1])[::-1], batch)
    for i in (0, 2, 5):
        assert np.array_equal(db.render([cases[i]])[0], batch[i])


def test_a_shift_by_one_tile_shifts_the_image_exactly():
    """Vertices with x / Z and y / Z multiples of 1/16 at Z in {2, 4, 8} under fx = fy = 64 and an integer principal point: every screen coordinate is an
    integer, so moving cx by 64 moves every coordinate by exactly 64 and the edge functions and depths see the same numbers.  The image moves by one tile,
    part of it leaves on the left; what stays must have the same bits."""
    rng = np.random.default_rng(5)
    n = 60
    Z = rng.choice([2.0, 4.0, 8.0], (n, 3))
    k = rng.integers(-16, 17, (n, 3, 2)) + rng.integers(-3, 4, (n, 1, 2))
    pts = np.concatenate((np.clip(k, -18, 18) / 16.0 * Z[:, :, None], Z[:, :, None]), axis=2).reshape(-1, 3).astype(np.float32)
    faces = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    T = np.hstack((np.eye(3), np.zeros((3, 1))))
    K = np.array([[64.0, 0.0, 126.0], [0.0, 64.0, 48.0], [0.0, 0.0, 1.0]])
    Ks = K.copy()
    Ks[0, 2] -= 64.0
    d = Db([("dyadic", pts, faces, 1.0)])
    a, b = d.render([(0, T, K)], 224, VC.H)[0], d.render([(0, T, Ks)], 224, VC.H)[0]
    d.close()
    assert (a[:, 64:] > 0).sum() > 1000 and (b[:, :8] > 0).any()
    assert np.array_equal(a[:, 64:], b[:, :160])
    assert np.array_equal(a, VR.render_depth(pts, faces, T, K, 224, VC.H))      # integers throughout: the numpy rasteriser sees the same numbers too


def test_error_kernel_equals_the_toolkit(ref_pairs):
    for normalized in (True, False):
        sel = [r for r in ref_pairs if r[0]["normalized"] == normalized]
        gold = np.array([GOLD["vsd_errors"][i] for i, r in enumerate(ref_pairs) if r[0]["normalized"] == normalized])
        de, dg = np.stack([r[1] for r in sel]), np.stack([r[2] for r in sel])
        tests = np.stack([r[0]["test"] for r in sel])
        e, c = vsd_from_depth(de, dg, tests, np.arange(len(sel)), np.stack([r[0]["K"] for r in sel]), normalized, [r[3] for r in sel])
        for k, (p, d_e, d_g, diam) in enumerate(sel):
            errors, counts = VR.vsd_from_depth(d_e, d_g, p["test"], p["K"], VC.DELTA, VC.TAUS, normalized, diam)
            assert c[k].tolist() == counts, (p["label"], c[k].tolist(), counts)
        assert np.array_equal(e, gold), np.abs(e - gold).max()
        # the pairs and their images in another order: nothing depends on the batch
        e2, c2 = vsd_from_depth(de[::-1], dg[::-1], tests, np.arange(len(sel))[::-1], np.stack([r[0]["K"] for r in sel]), normalized, [r[3] for r in sel][::-1])
        assert np.array_equal(e2[::-1], e) and np.array_equal(c2[::-1], c)


def test_fused_route_equals_render_then_error_kernel(db, ref_pairs):
    models = db.models
    for normalized in (True, False):
        sel = [r[0] for r in ref_pairs if r[0]["normalized"] == normalized]
        pairs = [(p["m"], p["Te"], p["Tg"], p["K"], models[p["m"]][3] if normalized else None) for p in sel]
        tests = np.stack([p["test"] for p in sel])
        e, c = db.vsd_poses(pairs, tests, np.arange(len(sel)))
        de, dg = db.render([(p[0], p[1], p[3]) for p in pairs]), db.render([(p[0], p[2], p[3]) for p in pairs])
        e2, c2 = vsd_from_depth(de, dg, tests, np.arange(len(sel)), np.stack([p[3] for p in pairs]), normalized, [models[p[0]][3] for p in pairs])
        assert np.array_equal(c, c2) and np.array_equal(e, e2)
        assert (c[:, 0] > 0).any()
    # repeated ground truths (two estimates against one ground truth, and est == gt twice): the same as one pair at a time
    p = [r[0] for r in ref_pairs]
    rep = [(p[0]["m"], p[0]["Te"], p[0]["Tg"], p[0]["K"], 100.0), (p[0]["m"], p[0]["Tg"], p[0]["Tg"], p[0]["K"], 100.0),
           (p[0]["m"], BC_shift(p[0]["Te"]), p[0]["Tg"], p[0]["K"], 100.0), (p[2]["m"], p[2]["Tg"], p[2]["Tg"], p[2]["K"], 100.0)]
    tests = np.stack([p[0]["test"], p[2]["test"]])
    ii = [0, 0, 0, 1]
    e, c = db.vsd_poses(rep, tests, ii)
    for k in range(len(rep)):
        e1, c1 = db.vsd_poses([rep[k]], tests, [ii[k]])
        assert np.array_equal(e1[0], e[k]) and np.array_equal(c1[0], c[k])
    assert (e[1] == 0).all() and (e[3] == 0).all() and (e[0] > 0).any()         # est == gt, unoccluded: error 0.0


def BC_shift(T):
    T = np.array(T, np.float64)
    T[0, 3] += 6.0
    return T


def test_edges(db, ref_pairs):
    lib = _lib.lib()
    models = db.models
    _, m, T, K = VC.render_cases()[0]
    rc, out = db.render_rc([])
    assert rc == 0 and len(out) == 0                                            # n = 0
    assert lib.suo_pose_errors_vsd(db.h, 0, None, None, None, None, VC.W, VC.H, 0, None, None, 15.0, 10, VC.TAUS.ctypes.data, 1, None, None, None) == 0
    # a model without faces; faces never set
    bare = Db(faces=False)
    assert bare.render_rc([(m, T, K)])[0] == SUO_ERR_ARG
    assert bare.set_faces([mm[2] if k != 1 else np.zeros((0, 3), np.int32) for k, mm in enumerate(models)]) == 0
    assert bare.render_rc([(1, T, K)])[0] == SUO_ERR_ARG and b"no faces" in lib.suo_last_error()
    assert bare.render_rc([(0, T, K)])[0] == 0
    # a bad face index: nothing is uploaded, the earlier set stays
    bad = [mm[2].copy() for mm in models]
    bad[0][3, 1] = len(models[0][1])
    assert bare.set_faces(bad) == SUO_ERR_ARG
    bad[0][3, 1] = -1
    assert bare.set_faces(bad) == SUO_ERR_ARG
    assert np.array_equal(bare.render([(0, T, K)]), db.render([(0, T, K)]))
    bare.close()
    # non-finite pose or camera, empty image, model index outside
    for bad_T, bad_K in ((np.where(np.arange(12).reshape(3, 4) == 7, np.nan, T), K), (T, np.where(np.eye(3) == 1, np.inf, K))):
        assert db.render_rc([(m, T, K), (m, bad_T, bad_K)])[0] == SUO_ERR_ARG
    assert db.render_rc([(m, T, K)], 0, 5)[0] == SUO_ERR_ARG and db.render_rc([(len(models), T, K)])[0] == SUO_ERR_ARG
    # an object wholly outside the image: all-zero depth and error 1.0
    out_pair = [r[0] for r in ref_pairs if r[0]["label"].startswith("outside")][0]
    e, c = db.vsd_poses([(out_pair["m"], out_pair["Te"], out_pair["Tg"], out_pair["K"], 100.0)], out_pair["test"][None], [0])
    assert (db.render([(out_pair["m"], out_pair["Tg"], out_pair["K"])]) == 0).all() and (e == 1.0).all() and (c == 0).all()
    # all-zero test depth: everything with depth > 0 is visible
    p = ref_pairs[1][0]
    e, c = db.vsd_poses([(p["m"], p["Te"], p["Tg"], p["K"], None)], np.zeros((1, VC.H, VC.W), np.float32), [0])
    de, dg = db.render([(p["m"], p["Te"], p["K"])])[0], db.render([(p["m"], p["Tg"], p["K"])])[0]
    assert c[0, 0] == ((de > 0) | (dg > 0)).sum() and c[0, 1] == ((de > 0) & (dg > 0)).sum() and c[0, 0] > c[0, 1] > 0
