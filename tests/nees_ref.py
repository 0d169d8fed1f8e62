"""Test-only fp64 numpy reference of the consistency figures (include/suo_hip.h: suo_pose_nees, suo_keypoint_nees), sharing no code with the library:
the SE(3) exponential and its logarithm (rotation from the antisymmetric part of R and its trace, upsilon by np.linalg.solve against V -- not the kernels'
quaternion route and closed V^-1), a brute-force symmetry pick over all points, NEES by np.linalg.solve, the keypoint chi2 as err @ inv(cov) @ err.

It also holds the Monte-Carlo generator of the one test that says the covariances mean something (tests/test_gpu_nees.py, tests/test_nees_ref.py) and a batched
numpy Gauss-Newton for it.  Lengths are METRES here (objects of 4-10 cm at 0.5-1.5 m): the bounds of the tests are absolute in xi, and a translation of ~1 keeps
the rounding of t_est - R t_ref (eps |t|) well inside them; the library only asks that all lengths share one unit."""
import functools

import numpy as np

EPS = np.finfo(np.float64).eps
CHI2_6_95, CHI2_6_99 = 12.5916, 16.8119          # chi2 quantiles, 6 degrees of freedom
CHI2_2_95, CHI2_2_99 = 5.9915, 9.210             # 2 degrees of freedom


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def _abc(th):
    """a = sin th / th, b = (1 - cos th) / th^2, c = (th - sin th) / th^3 without cancellation."""
    if th < 1e-2:
        t = th * th
        return (1 - t / 6 + t * t / 120 - t ** 3 / 5040, 0.5 - t / 24 + t * t / 720 - t ** 3 / 40320, 1 / 6 - t / 120 + t * t / 5040 - t ** 3 / 362880)
    return np.sin(th) / th, 2 * np.sin(th / 2) ** 2 / th ** 2, (th - np.sin(th)) / th ** 3


def exp_se3(u):
    """[omega, upsilon] -> 4x4: R = exp([omega]x), t = V upsilon."""
    w, v = np.asarray(u[:3], float), np.asarray(u[3:], float)
    a, b, c = _abc(float(np.linalg.norm(w)))
    Om = skew(w)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + a * Om + b * Om @ Om
    T[:3, 3] = (np.eye(3) + b * Om + c * Om @ Om) @ v
    return T


def log_se3(T):
    """4x4 -> [omega, upsilon], theta in [0, pi): omega from (R - R^T) / 2 = sin(theta) [axis]x and cos(theta) = (tr R - 1) / 2, upsilon = solve(V, t)."""
    R, t = np.asarray(T, float)[:3, :3], np.asarray(T, float)[:3, 3]
    s = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    ns = float(np.linalg.norm(s))
    th = float(np.arctan2(ns, 0.5 * (np.trace(R) - 1.0)))
    w = s * (th / ns) if ns > 1e-6 else s * (1 + ns * ns / 6 + 3 * ns ** 4 / 40)        # asin(x) / x
    _, b, c = _abc(float(np.linalg.norm(w)))
    Om = skew(w)
    V = np.eye(3) + b * Om + c * Om @ Om
    return np.r_[w, np.linalg.solve(V, t)]


def to4(T):
    T = np.asarray(T, float)
    if T.shape == (4, 4):
        return T
    out = np.eye(4)
    out[:3] = T.reshape(3, 4)
    return out


def symmetry_pick(points, syms, T_est, T_gt):
    """Index of the symmetry with the smallest max_i |T_est p_i - T_gt S_s p_i| over ALL points (first on ties), and the maxima."""
    P = np.c_[np.asarray(points, float), np.ones(len(points))].T
    est = (to4(T_est) @ P)[:3]
    d = np.array([np.sqrt((((to4(T_gt) @ to4(S) @ P)[:3] - est) ** 2).sum(0)).max() for S in syms])
    return int(np.argmin(d)), d


def pose_nees(points, syms, T_est, T_gt, cov):
    """dict(sym_index, T_ref 4x4, xi [6], nees) of one triple."""
    j, _ = symmetry_pick(points, syms, T_est, T_gt)
    T_ref = to4(T_gt) @ to4(syms[j])
    xi = log_se3(to4(T_est) @ np.linalg.inv(T_ref))
    return {"sym_index": j, "T_ref": T_ref, "xi": xi, "nees": float(xi @ np.linalg.solve(np.asarray(cov, float).reshape(6, 6), xi))}


def keypoint_chi2(model_kp, uv, cov, K, T_ref):
    """(chi2 [n], err [n,2]) of one detection: err = uv - pi(K, T_ref x); chi2 = err @ inv(cov) @ err, keypoint by keypoint."""
    X = (to4(T_ref) @ np.c_[np.asarray(model_kp, float).reshape(-1, 3), np.ones(len(model_kp))].T)[:3]
    h = np.asarray(K, float).reshape(3, 3) @ X
    err = np.asarray(uv, float).reshape(-1, 2) - (h[:2] / h[2]).T
    chi2 = np.einsum("ni,nij,nj->n", err, np.linalg.inv(np.asarray(cov, float).reshape(-1, 2, 2)), err) if len(err) else np.zeros(0)
    return chi2, err


# ---- Monte Carlo -----------------------------------------------------------------------------------------------------------------------------------
SIGMA = 0.001
N_KP = 16


def _rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


@functools.lru_cache(maxsize=None)
def monte_carlo(n_frames=4096, seed=0, n_kp=N_KP, sigma=SIGMA):
    """n_frames independent single-view frames: one fixed camera at the identity, one free object each (extent 4-10 cm at 0.5-1.5 m, the NDC intrinsics of its
    crop), n_kp keypoints with a random covariance C = A A^T sigma^2 each, THE NOISE DRAWN FROM THAT C (sigma A N(0, I)), information C^-1.
    A = Rot(phi) diag(a, b) with phi uniform and a, b uniform in [0.5, 1.5]: every orientation and an axis ratio up to 3, cond(C) <= 9.  (A = I + N(0, 0.3), the
    draw of tests/pose_cov_cases.py, comes within 1e-4 of singular somewhere in 65536 draws: that keypoint's information C^-1 is then a hard constraint, the
    pose Hessian's condition goes from a median of 1e4 to 6e11, and neither twenty LM iterations -- of the library or of the C oracle, which agree to 3e-12
    there -- nor a first-order covariance describe such a frame.  This test is about the covariances of well-posed frames.)
    dict of arrays: T_gt [N,4,4], T_init [N,4,4] (the truth moved by a small left update), k [N,4] (fx, fy, cx, cy), p [N,n_kp,3], uv [N,n_kp,2], cov [N,n_kp,2,2],
    info [N,n_kp,3] (xx, xy, yy).  Cached and read-only: tests take copies."""
    rng = np.random.default_rng(seed)
    out = {k: [] for k in ("T_gt", "T_init", "k", "p", "uv", "cov", "info")}
    for _ in range(n_frames):
        T = np.eye(4)
        T[:3, :3] = _rot(rng)
        z = rng.uniform(0.5, 1.5)
        T[:3, 3] = [rng.uniform(-0.2, 0.2) * z, rng.uniform(-0.15, 0.15) * z, z]
        p = rng.uniform(-1, 1, (n_kp, 3)) * rng.uniform(0.04, 0.1, 3)
        pc = (T @ np.c_[p, np.ones(n_kp)].T).T[:, :3]
        xy = pc[:, :2] / pc[:, 2:3]
        half = 0.6 * (xy.max(0) - xy.min(0))
        mid = 0.5 * (xy.max(0) + xy.min(0))
        k = np.array([1 / half[0], 1 / half[1], -mid[0] / half[0], -mid[1] / half[1]])
        phi, ax = rng.uniform(0, np.pi, n_kp), rng.uniform(0.5, 1.5, (n_kp, 2))
        A = np.stack([np.stack([np.cos(phi), -np.sin(phi)], -1), np.stack([np.sin(phi), np.cos(phi)], -1)], -2) * ax[:, None, :]
        C = A @ A.transpose(0, 2, 1) * sigma * sigma
        noise = sigma * np.einsum("nij,nj->ni", A, rng.normal(size=(n_kp, 2)))
        uv = xy * k[:2] + k[2:] + noise
        Om = np.linalg.inv(C)
        out["T_gt"].append(T)
        out["T_init"].append(exp_se3(np.r_[rng.normal(0, 2e-3, 3), rng.normal(0, 1e-3, 3)]) @ T)
        out["k"].append(k); out["p"].append(p); out["uv"].append(uv); out["cov"].append(C)
        out["info"].append(np.stack([Om[:, 0, 0], Om[:, 0, 1], Om[:, 1, 1]], -1))
    out = {k: np.stack(v) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


def _exp_batch(d):
    return np.stack([exp_se3(u) for u in d])


def _linearise(T, mc):
    """residuals r [N,n,2] = uv - projection and their Jacobians J [N,n,2,6] under the left update exp(delta) T, columns [omega, upsilon]."""
    pc = np.einsum("nij,nkj->nki", T[:, :3, :3], mc["p"]) + T[:, None, :3, 3]
    x, y, z = pc[..., 0], pc[..., 1], pc[..., 2]
    fx, fy, cx, cy = (mc["k"][:, None, i] for i in range(4))
    r = mc["uv"] - np.stack([fx * x / z + cx, fy * y / z + cy], -1)
    zero = np.zeros_like(x)
    Jp = np.stack([np.stack([fx / z, zero, -fx * x / z ** 2], -1), np.stack([zero, fy / z, -fy * y / z ** 2], -1)], -2)      # d proj / d pc [N,n,2,3]
    # d pc / d delta = [-[pc]x | I]
    D = np.zeros(pc.shape[:2] + (3, 6))
    D[..., 0, 1], D[..., 0, 2], D[..., 1, 0], D[..., 1, 2], D[..., 2, 0], D[..., 2, 1] = z, -y, -z, x, y, -x
    D[..., 0, 3] = D[..., 1, 4] = D[..., 2, 5] = 1.0
    return r, -Jp @ D


def gauss_newton(mc, iters=12):
    """Batched Gauss-Newton from T_init on the whole generator (no robust kernel, no gate): (T [N,4,4], Sigma [N,6,6] = H^-1 at T)."""
    T = mc["T_init"].copy()
    Om = np.zeros(mc["info"].shape[:2] + (2, 2))
    Om[..., 0, 0], Om[..., 0, 1], Om[..., 1, 0], Om[..., 1, 1] = mc["info"][..., 0], mc["info"][..., 1], mc["info"][..., 1], mc["info"][..., 2]
    for _ in range(iters):
        r, J = _linearise(T, mc)
        H = np.einsum("nkai,nkab,nkbj->nij", J, Om, J)
        g = np.einsum("nkai,nkab,nkb->ni", J, Om, r)
        T = _exp_batch(np.linalg.solve(H, -g[..., None])[..., 0]) @ T
    _, J = _linearise(T, mc)
    return T, np.linalg.inv(np.einsum("nkai,nkab,nkbj->nij", J, Om, J))


@functools.lru_cache(maxsize=None)
def monte_carlo_chain():
    """(T, Sigma) of gauss_newton on the default generator: computed once, read-only."""
    T, Sigma = gauss_newton(monte_carlo())
    T.setflags(write=False)
    Sigma.setflags(write=False)
    return T, Sigma


def keypoint_K(k):
    """3x3 camera matrix of the four intrinsics (fx, fy, cx, cy)."""
    return np.array([[k[0], 0.0, k[2]], [0.0, k[1], k[3]], [0.0, 0.0, 1.0]])


def mc_pose_nees(mc, T, Sigma):
    """NEES [N] of the poses T under Sigma against the generator's truth (identity symmetry)."""
    out = np.zeros(len(T))
    for i in range(len(T)):
        xi = log_se3(T[i] @ np.linalg.inv(mc["T_gt"][i]))
        out[i] = xi @ np.linalg.solve(Sigma[i], xi)
    return out


def mc_keypoint_chi2(mc):
    """chi2 [N * n_kp] of the generator's keypoints at the TRUE poses."""
    return np.concatenate([keypoint_chi2(mc["p"][i], mc["uv"][i], mc["cov"][i], keypoint_K(mc["k"][i]), mc["T_gt"][i])[0] for i in range(len(mc["p"]))])


def check_pose_gates(nees, n_se=6.0):
    """The gates of the exact chi2_6 distribution at n_se standard errors: mean 6 (variance 12), share <= 16.8119 is 0.99.  Derived, not measured."""
    n = len(nees)
    assert not np.isnan(nees).any(), "no case may be left out"
    mean, frac = float(np.mean(nees)), float(np.mean(nees <= CHI2_6_99))
    assert abs(mean - 6.0) <= n_se * np.sqrt(12.0 / n), f"mean NEES {mean:.4f} outside 6 +- {n_se * np.sqrt(12.0 / n):.3f}"
    assert abs(frac - 0.99) <= n_se * np.sqrt(0.0099 / n), f"share of NEES <= {CHI2_6_99}: {frac:.4f} outside 0.99 +- {n_se * np.sqrt(0.0099 / n):.4f}"
    return mean, frac


def check_keypoint_gates(chi2, n_se=6.0):
    """The gates of the exact chi2_2 distribution: mean 2 (variance 4), share <= 9.210 is 0.99."""
    n = len(chi2)
    assert not np.isnan(chi2).any(), "no case may be left out"
    mean, frac = float(np.mean(chi2)), float(np.mean(chi2 <= CHI2_2_99))
    assert abs(mean - 2.0) <= n_se * np.sqrt(4.0 / n), f"mean keypoint chi2 {mean:.4f} outside 2 +- {n_se * np.sqrt(4.0 / n):.4f}"
    assert abs(frac - 0.99) <= n_se * np.sqrt(0.0099 / n), f"share of keypoint chi2 <= {CHI2_2_99}: {frac:.4f} outside 0.99 +- {n_se * np.sqrt(0.0099 / n):.4f}"
    return mean, frac
