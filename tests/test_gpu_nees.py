"""suo_pose_nees / suo_keypoint_nees (csrc/eval_nees.hip) on the device against the numpy reference tests/nees_ref.py, and the Monte-Carlo test that says the
reported covariances mean something: 4096 single-view frames whose keypoint noise is drawn from the stated covariances, refined by ba.optimize_batch, must give
a NEES distributed as chi2 with six degrees of freedom under ba.pose_covariances_batch.

Lengths are metres (tests/nees_ref.py says why).  Bounds, as the feature's issue sets them: |xi - xi_ref| <= 1e3 eps (1 + |xi|_inf); |NEES - NEES_ref| <=
1e3 eps cond(Sigma) NEES_ref (the forward error of a solve through Cholesky, the form of tests/pose_cov_ref.py: bound); T_ref within 4 eps (1 + |t|) of the numpy
product; keypoint chi2 within 1e3 eps cond(C) chi2_ref.  The Monte-Carlo gates are six standard errors of the exact distributions (nees_ref.check_*_gates)."""
import ctypes as C

import numpy as np
import pytest

from suo_slam_amd import _lib, ba, bop_eval, consistency
from tests import nees_ref as R
from tests import pose_cov_cases as PC

pytestmark = pytest.mark.gpu
EPS = R.EPS


class Db:
    """A mesh database over clouds and symmetry sets with what consistency.pose_nees / keypoint_nees read of a BopErrors (lib, _h, _index)."""

    def __init__(self, clouds, syms):
        self.lib = _lib.lib()
        _lib.require_gpu()
        self.clouds = [np.ascontiguousarray(c, np.float32).reshape(-1, 3) for c in clouds]
        self.syms = [np.ascontiguousarray(s, np.float64).reshape(-1, 3, 4) for s in syms]
        n_pts = np.array([len(c) for c in self.clouds], np.int32)
        allpts = np.ascontiguousarray(np.concatenate(self.clouds, 0))
        self._h = C.c_void_p()
        _lib.check(self.lib.suo_mesh_db_create(len(self.clouds), n_pts.ctypes.data, allpts.ctypes.data, C.byref(self._h)), "suo_mesh_db_create")
        n_sym = np.array([len(s) for s in self.syms], np.int32)
        flat = np.ascontiguousarray(np.concatenate([s.reshape(-1, 12) for s in self.syms], 0))
        _lib.check(self.lib.suo_mesh_db_set_symmetries(self._h, n_sym.ctypes.data, flat.ctypes.data), "suo_mesh_db_set_symmetries")
        self._index = {i: i for i in range(len(self.clouds))}

    def close(self):
        self.lib.suo_mesh_db_destroy(self._h)


def _rz(a, offset=(0.0, 0.0, 0.0)):
    S = np.zeros((3, 4))
    S[:, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    S[:, 3] = -S[:, :3] @ np.array(offset) + np.array(offset)
    return S


IDENT, ROT2, ROT4, CONT, TWICE = range(5)


@pytest.fixture(scope="module")
def db():
    cloud = np.random.default_rng(11).uniform(-1, 1, (1500, 3)) * [0.05, 0.035, 0.06]           # 1500 points: crosses the 1024-point tile of bop_errors_kernel
    cont = bop_eval.symmetry_transformations({"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}, 0.01)
    assert len(cont) == 314                                                                      # ceil(pi / 0.01) - 1 rotations: crosses the 64-symmetry chunk
    syms = [np.eye(3, 4)[None], np.stack([np.eye(3, 4), _rz(np.pi)]), np.stack([_rz(0.5 * np.pi * k, (0.01, 0.02, 0.0)) for k in range(4)]), cont,
            np.stack([np.eye(3, 4), _rz(np.pi), _rz(np.pi)])]
    d = Db([cloud] * 5, syms)
    yield d
    d.close()


def _spd(rng, cond, scale=1e-4):
    Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
    return (Q * (scale * np.logspace(0, np.log10(cond), 6))) @ Q.T


@pytest.fixture(scope="module")
def covs():
    rng = np.random.default_rng(12)
    g, _ = PC.case("1x8")
    _, obj_cov, status = ba.pose_covariances(*PC.args(g))
    assert status.sum() == 0
    out = [np.diag([1e-4] * 3 + [2.5e-5] * 3), _spd(rng, 1e2), _spd(rng, 1e6), obj_cov[0].copy()]
    return [0.5 * (c + c.T) for c in out]


@pytest.fixture(scope="module")
def designed(db, covs):
    """The designed triples with their reference, computed once: T_est = exp(xi) T_gt S_j with a planted j and xi."""
    rng = np.random.default_rng(13)
    plan = [(IDENT, 0), (ROT2, 0), (ROT2, 1), (ROT4, 0), (ROT4, 1), (ROT4, 2), (ROT4, 3), (CONT, 0), (CONT, 63), (CONT, 64), (CONT, 200), (CONT, 310), (TWICE, 0),
            (TWICE, 2)]
    items = []
    for m, j in plan:
        for theta in (0.0, 1e-9, 1e-4, 0.05):
            for on_axis in (True, False):
                items.append((m, j, theta, on_axis))
    items += [(IDENT, 0, 0.3, True), (IDENT, 0, 0.3, False), (IDENT, 0, 3.0, True), (IDENT, 0, 3.0, False)]
    out = []
    for n, (m, j, theta, on_axis) in enumerate(items):
        T_gt = np.eye(4)
        T_gt[:3, :3], T_gt[:3, 3] = R._rot(rng), [rng.uniform(-0.1, 0.1), rng.uniform(-0.08, 0.08), rng.uniform(0.5, 0.7)]
        axis = T_gt[:3, :3] @ [0.0, 0.0, 1.0] if on_axis else np.cross(T_gt[:3, :3] @ [0.0, 0.0, 1.0], rng.normal(size=3))
        xi = np.r_[theta * axis / np.linalg.norm(axis), rng.normal(0, 0.01, 3)]
        T_est = R.exp_se3(xi) @ T_gt @ R.to4(db.syms[m][j])
        cov = covs[n % 4]
        ref = R.pose_nees(db.clouds[m].astype(np.float64), db.syms[m], T_est, T_gt, cov)
        out.append({"m": m, "j": j, "theta": theta, "on_axis": on_axis, "T_est": T_est, "T_gt": T_gt, "cov": cov, "xi": xi, "ref": ref})
    return out


def _call(db, items):
    return consistency.pose_nees(db, [it["m"] for it in items], np.stack([it["T_est"] for it in items]), np.stack([it["T_gt"] for it in items]),
                                 np.stack([it["cov"] for it in items]))


def test_designed_poses(db, designed):
    got = _call(db, designed)
    assert got["n_nan"] == 0
    worst_xi = worst_nees = 0.0
    for i, it in enumerate(designed):
        ref, tag = it["ref"], (it["m"], it["j"], it["theta"], it["on_axis"])
        # the planted symmetry is the minimiser wherever another one cannot win: everywhere but a rotation of 2.5 steps of the continuous set
        if not (it["m"] == CONT and it["theta"] > 1e-3):
            assert ref["sym_index"] == (1 if (it["m"], it["j"]) == (TWICE, 2) else it["j"]), tag
            assert np.abs(ref["xi"] - it["xi"]).max() < 1e-12, tag
        assert got["sym_index"][i] == ref["sym_index"], tag
        assert np.abs(got["T_ref"][i] - ref["T_ref"][:3]).max() <= 4 * EPS * (1 + np.abs(ref["T_ref"][:3, 3]).max()), tag
        dxi = np.abs(got["xi"][i] - ref["xi"]).max()
        assert dxi <= 1e3 * EPS * (1 + np.abs(ref["xi"]).max()), (tag, dxi)
        dn = abs(got["nees"][i] - ref["nees"])
        assert dn <= 1e3 * EPS * np.linalg.cond(it["cov"]) * ref["nees"], (tag, dn, ref["nees"])
        worst_xi, worst_nees = max(worst_xi, dxi / (EPS * (1 + np.abs(ref["xi"]).max()))), max(worst_nees, dn / (EPS * np.linalg.cond(it["cov"]) * ref["nees"]))
    print(f"designed poses: worst |xi - ref| = {worst_xi:.2f} eps (1 + |xi|), worst |NEES - ref| = {worst_nees:.3f} eps cond NEES (bounds: 1e3)")
    big = [i for i, it in enumerate(designed) if it["theta"] == 3.0]
    assert len(big) == 2 and all(abs(np.linalg.norm(got["xi"][i][:3]) - 3.0) < 1e-12 for i in big)


def test_nan_rules(db, designed, covs):
    good = [designed[3], designed[40], designed[77]]
    neg = covs[0].copy()
    neg[0, 1] = neg[1, 0] = 2e-4                                  # positive diagonal, one negative eigenvalue
    assert np.linalg.eigvalsh(neg).min() < 0
    nan_block = covs[1].copy()
    nan_block[5, 2] = np.nan                                      # (an entry of the upper triangle would do too: all 36 are looked at)
    nan_upper = covs[1].copy()
    nan_upper[0, 5] = np.inf
    nan_pose = dict(good[0], T_est=good[0]["T_est"].copy())
    nan_pose["T_est"][1, 3] = np.nan
    batch = [good[0], dict(good[1], cov=nan_block), good[1], dict(good[2], cov=neg), dict(good[0], cov=np.zeros((6, 6))), nan_pose, good[2],
             dict(good[1], cov=nan_upper)]
    got = _call(db, batch)
    bad = [1, 3, 4, 5, 7]
    assert np.isnan(got["nees"][bad]).all() and got["n_nan"] == len(bad)
    assert got["sym_index"][5] == -1 and np.isnan(got["xi"][5]).all() and np.isnan(got["T_ref"][5]).all()
    for i in (1, 3, 4, 7):                                        # a bad block spoils the NEES only
        assert got["sym_index"][i] == batch[i]["ref"]["sym_index"] and np.isfinite(got["xi"][i]).all()
    for i, g in ((0, good[0]), (2, good[1]), (6, good[2])):       # the neighbours have the bits they have alone
        alone = _call(db, [g])
        assert got["nees"][i] == alone["nees"][0] and np.isfinite(got["nees"][i])
        assert np.array_equal(got["xi"][i], alone["xi"][0])


def test_batch_independence_and_empty_call(db, designed):
    pick = [0, 9, 18, 27, 37, 46, 58, 67, 76, 89, 104, len(designed) - 1]
    items = [designed[i] for i in pick]
    assert len({it["m"] for it in items}) == 5
    a, b = _call(db, items), _call(db, items)
    for k in ("nees", "xi", "sym_index", "T_ref"):
        assert np.array_equal(a[k], b[k]), k
    for i, it in enumerate(items):
        alone = _call(db, [it])
        for k in ("nees", "xi", "sym_index", "T_ref"):
            assert np.array_equal(a[k][i], alone[k][0]), (k, i)
    empty = consistency.pose_nees(db, [], np.zeros((0, 4, 4)), np.zeros((0, 4, 4)), np.zeros((0, 6, 6)))
    assert empty["nees"].shape == (0,) and empty["n_nan"] == 0
    status = np.full(1, 7, np.int32)
    assert db.lib.suo_pose_nees(db._h, 0, None, None, None, None, None, None, None, None, status.ctypes.data) == 0 and status[0] == 0
    assert db.lib.suo_keypoint_nees(db._h, 0, None, None, None, None, None, None, None, None) == 0
    # the one argument rule that needs a live database: an index at or past n_models
    it = designed[0]
    idx, Te, Tg, cv, out = np.array([5], np.int32), it["T_est"][:3].copy(), it["T_gt"][:3].copy(), it["cov"].copy(), np.zeros(1)
    assert db.lib.suo_pose_nees(db._h, 1, idx.ctypes.data, Te.ctypes.data, Tg.ctypes.data, cv.ctypes.data, out.ctypes.data, None, None, None, None) == 1
    assert b"model_index[0]=5 out of range" in db.lib.suo_last_error()


def test_keypoints(db):
    """n_pts = 0, 1, 41, 7 in one call, K the K_bbox of a crop (NDC); noise 0.05 of the crop, so that the rounding of uv - projection (eps |uv|) stays a small part
    of the error it leaves."""
    rng = np.random.default_rng(14)
    sigma, dets, T_ref = 0.05, [], []
    for k in (0, 1, 41, 7):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R._rot(rng), [rng.uniform(-0.1, 0.1), rng.uniform(-0.08, 0.08), rng.uniform(0.5, 0.7)]
        p = rng.uniform(-1, 1, (k, 3)) * [0.05, 0.035, 0.06]
        pc = (T @ np.c_[p, np.ones(k)].T).T[:, :3]
        xy = pc[:, :2] / pc[:, 2:3] if k else np.zeros((0, 2))
        half, mid = (0.6 * (xy.max(0) - xy.min(0)) + 0.01, 0.5 * (xy.max(0) + xy.min(0))) if k else (np.ones(2), np.zeros(2))
        kk = np.array([1 / half[0], 1 / half[1], -mid[0] / half[0], -mid[1] / half[1]])
        A = rng.normal(0, 0.3, (k, 2, 2)) + np.eye(2)
        cov = A @ A.transpose(0, 2, 1) * sigma * sigma
        uv = xy * kk[:2] + kk[2:] + sigma * np.einsum("nij,nj->ni", A, rng.normal(size=(k, 2)))
        dets.append({"model_kp": p, "uv_pred": uv, "cov_pred": cov, "K": R.keypoint_K(kk)})
        T_ref.append(T)
    d41 = dets[2]
    d41["cov_pred"][3] = np.outer([1.0, 2.0], [1.0, 2.0]) * sigma ** 2                          # singular
    d41["cov_pred"][4] = np.array([[1.0, 2.0], [2.0, 1.0]]) * sigma ** 2                        # indefinite, positive diagonal
    d41["cov_pred"][5] = np.array([[-1.0, 0.0], [0.0, -1.0]]) * sigma ** 2                      # positive determinant, negative diagonal
    d41["cov_pred"][6, 0, 1] = np.nan
    d41["model_kp"][7] = np.linalg.inv(T_ref[2])[:3, :3] @ (np.array([0.01, 0.02, -0.4]) - T_ref[2][:3, 3])      # behind the camera: z = -0.4
    nan_at = [3, 4, 5, 6]
    dets.append({"model_kp": np.zeros((3, 3)), "uv_pred": np.zeros((3, 2)), "cov_pred": None, "K": np.eye(3)})  # no covariance: skipped and counted
    T_ref.append(np.eye(4))
    got = consistency.keypoint_nees(db, dets, np.stack(T_ref))
    assert got["n_skipped"] == 1 and got["chi2"][4] is None and got["chi2"][0].shape == (0,)
    worst = 0.0
    for i in (1, 2, 3):
        keep = [j for j in range(len(dets[i]["uv_pred"])) if not (i == 2 and j in nan_at)]
        chi2, err = R.keypoint_chi2(dets[i]["model_kp"][keep], dets[i]["uv_pred"][keep], dets[i]["cov_pred"][keep], dets[i]["K"], T_ref[i])
        cond = np.linalg.cond(dets[i]["cov_pred"][keep])
        assert np.isfinite(got["chi2"][i][keep]).all()
        assert (np.abs(got["chi2"][i][keep] - chi2) <= 1e3 * EPS * cond * chi2).all()
        assert (np.abs(got["err"][i][keep] - err) <= 1e3 * EPS * (1 + np.abs(err))).all()
        worst = max(worst, float((np.abs(got["chi2"][i][keep] - chi2) / (EPS * cond * chi2)).max()))
    print(f"keypoints: worst |chi2 - ref| = {worst:.3f} eps cond chi2 (bound 1e3)")
    assert np.isnan(got["chi2"][2][nan_at]).all()
    assert np.isfinite(got["chi2"][2][7]) and got["chi2"][2][7] > 100                            # the point behind the camera keeps its finite value


# ---- Monte Carlo ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def monte_carlo_on_device():
    mc = R.monte_carlo()
    N, n_kp = mc["p"].shape[:2]
    cam_T, zeros = np.eye(4)[None, :3], np.zeros(n_kp, np.int32)
    problems = [ba.Problem(cam_T, [1], mc["T_init"][i][None, :3], [0], zeros, zeros, np.tile(mc["k"][i], (n_kp, 1)), mc["p"][i], mc["uv"][i], mc["info"][i],
                           np.ones(n_kp, np.uint8), its=(10, 10), chi2_thr=1e12, huber_delta=1e6) for i in range(N)]
    ba.optimize_batch(problems)
    assert all(p.inlier.all() for p in problems)
    cov = ba.pose_covariances_batch(problems)
    assert sum(int(c[2].sum()) for c in cov) == 0
    T_est = np.stack([p.obj_T.reshape(3, 4) for p in problems])
    Sigma = np.stack([c[1][0] for c in cov])
    d = Db([np.random.default_rng(15).uniform(-0.05, 0.05, (8, 3))], [np.eye(3, 4)[None]])
    yield d, mc, T_est, Sigma
    d.close()


def test_monte_carlo_covariances_are_consistent(monte_carlo_on_device):
    """Measured on an MI355X (profiles/consistency.txt): mean NEES 6.0356, share <= 16.8119 0.9873, mean keypoint chi2 1.9972, share <= 9.210 0.9900 -- the
    figures of the numpy chain on the same inputs (tests/test_nees_ref.py) to the digits shown."""
    d, mc, T_est, Sigma = monte_carlo_on_device
    N, n_kp = mc["p"].shape[:2]
    got = consistency.pose_nees(d, [0] * N, T_est, mc["T_gt"], Sigma)
    assert got["n_nan"] == 0 and (got["sym_index"] == 0).all()
    print(f"Monte Carlo on the device, {N} frames: mean NEES {np.mean(got['nees']):.4f}, share <= {R.CHI2_6_99}: {np.mean(got['nees'] <= R.CHI2_6_99):.4f}, "
          f"share <= {R.CHI2_6_95}: {np.mean(got['nees'] <= R.CHI2_6_95):.4f}")
    R.check_pose_gates(got["nees"])
    dets = [{"model_kp": mc["p"][i], "uv_pred": mc["uv"][i], "cov_pred": mc["cov"][i], "K": R.keypoint_K(mc["k"][i])} for i in range(N)]
    kp = consistency.keypoint_nees(d, dets, mc["T_gt"])
    chi2 = np.concatenate(kp["chi2"])
    assert kp["n_skipped"] == 0 and chi2.shape == (N * n_kp,)
    print(f"Monte Carlo keypoints, {len(chi2)}: mean chi2 {np.mean(chi2):.4f}, share <= {R.CHI2_2_99}: {np.mean(chi2 <= R.CHI2_2_99):.4f}")
    R.check_keypoint_gates(chi2)


def test_the_gate_tells_a_swapped_convention(monte_carlo_on_device):
    d, mc, T_est, Sigma = monte_carlo_on_device
    perm = [3, 4, 5, 0, 1, 2]
    swapped = np.ascontiguousarray(Sigma[:512][:, perm][:, :, perm])
    got = consistency.pose_nees(d, [0] * 512, T_est[:512], mc["T_gt"][:512], swapped)
    print(f"[upsilon, omega] order on 512 frames: mean NEES {np.nanmean(got['nees']):.3f}")
    with pytest.raises(AssertionError):
        R.check_pose_gates(got["nees"])
