"""Seeded inputs of the BOP-19 goldens (row N5), shared by tests/golden/make_bop19_golden.py (which runs the REFERENCE's vendored bop_toolkit on them, build
container only) and by the tests (which regenerate them, so tests/golden/bop19_golden.npz holds results only).  Nothing here comes from the toolkit.

Ranges the tolerance of tests/test_gpu_bop_errors.py is derived for: |p| <= 200 mm, |t| <= 2000 mm, |z| >= 200 mm for every transformed point, f <= 1100 px."""
import numpy as np

_ROT_Z = np.diag([-1.0, -1.0, 1.0, 1.0])
_ROT_X = np.diag([1.0, -1.0, -1.0, 1.0])
_ROT_Y = np.diag([-1.0, 1.0, -1.0, 1.0])
_ROT_X_SHIFTED = _ROT_X.copy()
_ROT_X_SHIFTED[:3, 3] = [0.0, 4.0, -6.0]              # a half turn about an axis that misses the origin

# model infos in models_info.json's form; S at max_sym_disc_step 0.01: 1, 2, 4, 314, 314, 628, 1256
SYM_INFOS = {
    "none": {"diameter": 210.0},
    "disc1": {"diameter": 180.0, "symmetries_discrete": [_ROT_Z.ravel().tolist()]},
    "disc3": {"diameter": 250.0, "symmetries_discrete": [_ROT_Z.ravel().tolist(), _ROT_X_SHIFTED.ravel().tolist(), _ROT_Y.ravel().tolist()]},
    "cont0": {"diameter": 160.0, "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]},
    "cont_off": {"diameter": 230.0, "symmetries_continuous": [{"axis": [0.3, -0.2, 1.0], "offset": [5.0, -3.0, 12.0]}]},
    "both1": {"diameter": 200.0, "symmetries_discrete": [_ROT_X.ravel().tolist()], "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]},
    "both3": {"diameter": 240.0, "symmetries_discrete": [_ROT_Z.ravel().tolist(), _ROT_X.ravel().tolist(), _ROT_Y.ravel().tolist()],
              "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0.0, 0.0, 7.5]}]},
}
SYM_STEPS = (0.01, 0.1)

# (points, symmetry set) of the models of the error pairs: every P of the parity list, every S of it (1, 2, 314, 628, 1256)
MODELS = ((1, "none"), (63, "disc1"), (64, "cont0"), (65, "both1"), (255, "both3"), (257, "none"), (1000, "disc1"), (4099, "cont_off"), (1000, "both1"),
          (4099, "both3"), (257, "disc3"))
N_PAIRS = 40
N_BEHIND = 3                                          # further pairs with the object behind the camera (z <= -200): finite, equal to the toolkit


def model_points(m, seed=1905):
    """[P,3] float32, |p| <= 200 mm."""
    rng = np.random.default_rng(seed + m)
    ext = rng.uniform(30, 110, 3)
    return (rng.uniform(-1, 1, (MODELS[m][0], 3)) * ext).astype(np.float32)


def random_rotation(rng):
    Q, R = np.linalg.qr(rng.standard_normal((3, 3)))
    Q = Q @ np.diag(np.sign(np.diag(R)))
    if np.linalg.det(Q) < 0:
        Q[:, 0] *= -1
    return Q


def rotvec(v):
    """Rodrigues: the rotation by |v| radians about v."""
    th = float(np.linalg.norm(v))
    if th == 0:
        return np.eye(3)
    k = np.asarray(v, np.float64) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def compose(T, S):
    """T S for 3x4 [R|t] blocks."""
    return np.hstack((T[:, :3] @ S[:, :3], T[:, :3] @ S[:, 3:] + T[:, 3:]))


def pairs(syms_of, seed=77):
    """N_PAIRS + N_BEHIND (model index, T_est [3,4], T_gt [3,4], K [3,3]) items.  ``syms_of(name)`` -> [S,3,4]: the symmetry set of a SYM_INFOS entry (the
    caller's own, at step 0.01); estimates are small and large perturbations of the ground truth and of its symmetric counterparts, and exact counterparts."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(N_PAIRS + N_BEHIND):
        m = i % len(MODELS)
        Tg = np.hstack((random_rotation(rng), np.array([[rng.uniform(-300, 300)], [rng.uniform(-200, 200)], [rng.uniform(500, 1500)]])))
        if i >= N_PAIRS:
            Tg[2, 3] = -rng.uniform(500, 1000)
        S = syms_of(MODELS[m][1])
        Sk = S[int(rng.integers(0, len(S)))]
        kind = i % 4
        if kind == 0:
            d = np.hstack((rotvec(rng.standard_normal(3) * 0.03), rng.standard_normal((3, 1)) * 3.0))
            Te = compose(Tg, d)
        elif kind == 1:
            d = np.hstack((rotvec(rng.standard_normal(3) * 0.02), rng.standard_normal((3, 1)) * 2.0))
            Te = compose(compose(Tg, Sk), d)
        elif kind == 2:
            d = np.hstack((rotvec(rng.standard_normal(3) * 0.6), rng.standard_normal((3, 1)) * 30.0))
            Te = compose(Tg, d)
        else:
            Te = compose(Tg, Sk)
        K = np.array([[rng.uniform(500, 1100), 0.5 if i % 5 == 0 else 0.0, rng.uniform(300, 400)], [0.0, rng.uniform(500, 1100), rng.uniform(200, 300)], [0.0, 0.0, 1.0]])
        out.append((m, Te, Tg, K))
    return out


def match_case(seed=5):
    """A synthetic error table for the matching and recall goldens: one scene, six images, classes with up to three instances, ties in score, invalid ground
    truths, infinite errors and more estimates than ``inst_count``.  Returns ``(gt_obj_ids {im: [obj]}, gt_valid {im: [bool]}, inst_count {(im, obj): k},
    ests {(im, obj): [{"score", "errors": {gt_id: e}}]})`` with errors in [0, 0.8] (normalised-MSSD-like; times 100 they are MSPD-like)."""
    rng = np.random.default_rng(seed)
    gt_obj_ids, gt_valid, inst_count, ests = {}, {}, {}, {}
    for im in (3, 8, 15, 16, 42, 77):
        objs = []
        for o in rng.choice(np.arange(1, 8), 3, replace=False).tolist():
            objs += [int(o)] * int(rng.integers(1, 4))
        objs = [objs[j] for j in rng.permutation(len(objs))]
        gt_obj_ids[im] = objs
        gt_valid[im] = [bool(rng.random() < 0.8) for _ in objs]
        for o in sorted(set(objs)):
            gts = [g for g, oo in enumerate(objs) if oo == o]
            inst_count[(im, o)] = len(gts) if rng.random() < 0.7 else max(1, len(gts) - 1)
            if rng.random() < 0.1:
                continue                                              # a target without estimates
            n_est = int(rng.integers(1, len(gts) + 3))
            rows = []
            for _ in range(n_est):
                errors = {}
                for g in gts:
                    e = float(np.round(rng.uniform(0, 0.8), 3))       # three decimals: several errors fall on thresholds' neighbours, none relies on 1 ulp
                    errors[g] = float("inf") if rng.random() < 0.1 else e
                rows.append({"score": float(rng.integers(1, 4)), "errors": errors})      # scores 1..3: ties are the rule
            ests[(im, o)] = rows
    return gt_obj_ids, gt_valid, inst_count, ests
