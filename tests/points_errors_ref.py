"""Yardsticks of the point-set and mask pose errors of row N4 (include/suo_hip.h: suo_pose_errors_points, suo_pose_errors_masks); a helper, not a test.

    add / adi / proj       float64 numpy, written from the header's definitions (each coordinate ((r0 x + r1 y) + r2 z) + t, a squared distance
                           (dx^2 + dy^2) + dz^2, the exact nearest neighbour by brute force, np.mean): tests/test_siso_host.py ties them to the toolkit's
                           pose_error.add / adi / proj, recorded in tests/golden/siso_golden.npz
    mp_errors              the same three definitions in mpmath at 40 digits with the error scale of the pair: the yardstick of
                           tests/test_gpu_points_errors.py
    mask_counts            union, intersection and the two boxes of a pair's renders by the numpy rasteriser of tests/vsd_ref.py
    RefSisoErrors          stands in for bop_eval.BopErrors under a LocalizationMeter: the above + the numpy VSD of tests/vsd_ref.py
"""
import numpy as np

from tests import vsd_ref as VR

# The largest |toolkit float64 - mp| / (2^-52 s) over siso_cases.point_pairs(), s the pair's error scale (mp_errors), measured by tests/test_siso_host.py, which
# holds it: a measurement above TOOLKIT_RATIO fails there.  C = 8 TOOLKIT_RATIO is the tolerance factor of the GPU test (the margin is for the different
# summation order of a P-term mean).  No figure here comes from a GPU run.
TOOLKIT_RATIO = {"add": 0.11, "adi": 0.05, "proj": 0.8}        # measured: 0.105, 0.0487, 0.773 (the numpy restatement here: 0.105, 0.029, 0.723)
C = {k: 8.0 * v for k, v in TOOLKIT_RATIO.items()}
EPS = 2.0 ** -52


def transform(points, T):
    P = np.asarray(points, np.float32).astype(np.float64)
    T = np.asarray(T, np.float64).reshape(-1, 4)[:3]
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    return np.stack([((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)], 1)


def project(points, K, T):
    """misc.project_pts: M = K [R|t] formed first, (M [p;1])_xy / (M [p;1])_z."""
    K, T = np.asarray(K, np.float64).reshape(3, 3), np.asarray(T, np.float64).reshape(-1, 4)[:3]
    M = np.array([[(K[i, 0] * T[0, j] + K[i, 1] * T[1, j]) + K[i, 2] * T[2, j] for j in range(4)] for i in range(3)])
    h = transform(points, M)
    with np.errstate(all="ignore"):
        return h[:, :2] / h[:, 2:]


def _norm_rows(d):
    s = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    return np.sqrt(s + d[:, 2] * d[:, 2] if d.shape[1] == 3 else s)


def add(points, T_est, T_gt):
    return float(np.mean(_norm_rows(transform(points, T_est) - transform(points, T_gt))))


def adi(points, T_est, T_gt):
    """mean over the GROUND-TRUTH points of the distance to the nearest ESTIMATED-pose point."""
    e, g = transform(points, T_est), transform(points, T_gt)
    best = np.full(len(g), np.inf)
    for b in range(0, len(e), 512):
        d = g[:, None, :] - e[None, b:b + 512, :]
        best = np.minimum(best, ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).min(1))
    return float(np.mean(np.sqrt(best)))


def proj(points, T_est, T_gt, K):
    return float(np.mean(_norm_rows(project(points, K, T_est) - project(points, K, T_gt))))


def mp_errors(points, T_est, T_gt, K, dps=40):
    """``({"add", "adi", "proj"}, {the same: error scale s})`` in mpmath: s = the largest |coordinate| over both transformed point sets (add, adi), the
    largest |projected coordinate| (proj).  The float64 inputs are taken exactly; the nearest neighbour is chosen in float64 among the candidates within
    1e-9 relative of the float64 minimum, each evaluated in mp."""
    import mpmath as mp
    with mp.workdps(dps):
        P = np.asarray(points, np.float32).astype(np.float64)
        Te, Tg, Km = (np.asarray(a, np.float64) for a in (T_est, T_gt, K))

        def xf(T, p):
            return [mp.fsum([mp.mpf(float(T[i, j])) * mp.mpf(float(p[j])) for j in range(3)] + [mp.mpf(float(T[i, 3]))]) for i in range(3)]

        def pj(T, p):
            X = xf(T, p)
            h = [mp.fsum([mp.mpf(float(Km[i, j])) * X[j] for j in range(3)]) for i in range(3)]
            return [h[0] / h[2], h[1] / h[2]]
        E, G = [xf(Te, p) for p in P], [xf(Tg, p) for p in P]
        n = len(P)
        s_add = mp.fsum([mp.sqrt(mp.fsum([(a - b) ** 2 for a, b in zip(e, g)])) for e, g in zip(E, G)]) / n
        e64, g64 = transform(P, Te), transform(P, Tg)
        s_adi = mp.mpf(0)
        for i in range(n):
            d2 = ((g64[i] - e64) ** 2).sum(1)
            cand = np.nonzero(d2 <= d2.min() * (1 + 1e-9) + 1e-300)[0]
            s_adi += mp.sqrt(min(mp.fsum([(a - b) ** 2 for a, b in zip(E[j], G[i])]) for j in cand))
        s_adi /= n
        ue, ug = [pj(Te, p) for p in P], [pj(Tg, p) for p in P]
        s_proj = mp.fsum([mp.sqrt(mp.fsum([(a - b) ** 2 for a, b in zip(e, g)])) for e, g in zip(ue, ug)]) / n
        s3 = float(max(np.abs(e64).max(), np.abs(g64).max()))
        s2 = float(max(max(abs(c) for u in ue for c in u), max(abs(c) for u in ug for c in u)))
        return {"add": s_add, "adi": s_adi, "proj": s_proj}, {"add": s3, "adi": s3, "proj": s2}


def ratio(value, mp_value, scale):
    """|value - mp_value| / (2^-52 scale) as a float."""
    import mpmath as mp
    with mp.workdps(40):
        return float(abs(mp.mpf(float(value)) - mp_value) / (mp.mpf(EPS) * mp.mpf(scale)))


def _box(mask):
    ys, xs = mask.nonzero()
    return [-1, -1, -1, -1] if xs.size == 0 else [int(xs.min()), int(ys.min()), int(xs.max() - xs.min()), int(ys.max() - ys.min())]


def mask_counts(points, faces, T_est, T_gt, K, width, height, renders=None):
    """``(union, intersection, box_est, box_gt)`` of the masks depth > 0 of the two renders (boxes as misc.calc_2d_bbox, [-1] * 4 for an empty mask)."""
    ren = renders if renders is not None else (lambda T: VR.render_depth(points, faces, T, K, width, height))
    me, mg = ren(T_est) > 0, ren(T_gt) > 0
    return int((me | mg).sum()), int((me & mg).sum()), _box(me), _box(mg)


class RefSisoErrors(VR.RefVsdErrors):
    """The numpy counterpart of bop_eval.BopErrors for a LocalizationMeter: ``.errors`` and ``.vsd`` of tests/vsd_ref.RefVsdErrors, ``.point_errors`` and
    ``.mask_errors`` of this module.  Renders are cached per (object, pose, camera, size)."""

    def __init__(self, mesh_db, models_info, max_sym_disc_step=0.01):
        super().__init__(mesh_db, models_info, max_sym_disc_step)
        self._renders = {}

    def point_errors(self, obj_ids, T_est, T_gt, K=None, which=("add", "adi", "proj")):
        fn = {"add": lambda p, e, g, k: add(p, e, g), "adi": lambda p, e, g, k: adi(p, e, g), "proj": lambda p, e, g, k: proj(p, e, g, k)}
        Ks = [None] * len(obj_ids) if K is None else np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 3, 3), (len(obj_ids), 3, 3))
        return {w: np.array([fn[w](self.mesh_db[int(o)]["points"], e, g, k) for o, e, g, k in zip(obj_ids, T_est, T_gt, Ks)], np.float64) for w in which}

    def _render(self, o, T, K, hw):
        key = (int(o), np.asarray(T, np.float64).tobytes(), np.asarray(K, np.float64).tobytes(), tuple(hw))
        if key not in self._renders:
            self._renders[key] = VR.render_depth(self.mesh_db[int(o)]["points"], self.mesh_db[int(o)]["faces"], T, K, hw[1], hw[0])
        return self._renders[key]

    def mask_errors(self, obj_ids, T_est, T_gt, K, hw):
        from suo_slam_amd import bop_eval
        Ks = np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 3, 3), (len(obj_ids), 3, 3))
        rows = [mask_counts(None, None, e, g, k, hw[1], hw[0], renders=lambda T, o=o, k=k: self._render(o, T, k, hw)) for o, e, g, k in zip(obj_ids, T_est, T_gt, Ks)]
        return {"cus": np.array([bop_eval.cus_from_counts(u, i) for u, i, _, _ in rows], np.float64),
                "cou_bb_proj": np.array([bop_eval.cou_bb_from_boxes(a, b) for _, _, a, b in rows], np.float64),
                "union": np.array([r[0] for r in rows], np.int64), "inter": np.array([r[1] for r in rows], np.int64),
                "box_est": np.array([r[2] for r in rows], np.int32).reshape(-1, 4), "box_gt": np.array([r[3] for r in rows], np.int32).reshape(-1, 4)}
