"""Test-only fp64 numpy reference of the pose covariances (include/suo_hip.h: suo_pose_covariances), sharing no code with the library:
residuals from 4x4 poses, Jacobians by CENTRAL DIFFERENCES of the residual under the left update exp(delta) T (step 1e-6; columns [omega, upsilon]) -- not the
kernels' analytic formulas --, the dense Gauss-Newton Hessian over the free vertices that a counted edge reaches, np.linalg.inv.

A graph is a dict with the arguments of suo_slam_amd.ba.optimize: cam_T [C,3,4], cam_fixed [C], obj_T [O,3,4], obj_fixed [O], edge_cam / edge_obj [E],
edge_camk [E,4] (fx, fy, cx, cy), edge_p [E,3], edge_uv [E,2], edge_info [E,3] (xx, xy, yy), edge_inlier [E]."""
import numpy as np

STEP = 1e-6


def _skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def exp_se3(u):
    """[omega, upsilon] -> 4x4: R = exp([omega]x), t = V upsilon (the SE(3) exponential)."""
    w, v = np.asarray(u[:3], float), np.asarray(u[3:], float)
    th = float(np.linalg.norm(w))
    Om = _skew(w)
    if th < 1e-12:
        R, V = np.eye(3) + Om, np.eye(3) + 0.5 * Om
    else:
        a, b, c = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
        R = np.eye(3) + a * Om + b * Om @ Om
        V = np.eye(3) + b * Om + c * Om @ Om
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, V @ v
    return T


def to4(T34):
    T = np.eye(4)
    T[:3] = np.asarray(T34, float).reshape(3, 4)
    return T


def residual(Tc, To, k, p, uv):
    """measured uv minus the projection of model point p through object pose To (object -> world) and camera pose Tc (world -> camera)."""
    pc = (Tc @ To @ np.append(p, 1.0))[:3]
    return np.asarray(uv, float) - np.array([k[0] * pc[0] / pc[2] + k[2], k[1] * pc[1] / pc[2] + k[3]])


def edge_jacobians(g, e):
    """(J_cam [2,6], J_obj [2,6]) of edge e by central differences."""
    Tc, To = to4(g["cam_T"][g["edge_cam"][e]]), to4(g["obj_T"][g["edge_obj"][e]])
    k, p, uv = g["edge_camk"][e], g["edge_p"][e], g["edge_uv"][e]
    Jc, Jo = np.zeros((2, 6)), np.zeros((2, 6))
    for i in range(6):
        d = np.zeros(6)
        d[i] = STEP
        Jc[:, i] = (residual(exp_se3(d) @ Tc, To, k, p, uv) - residual(exp_se3(-d) @ Tc, To, k, p, uv)) / (2 * STEP)
        Jo[:, i] = (residual(Tc, exp_se3(d) @ To, k, p, uv) - residual(Tc, exp_se3(-d) @ To, k, p, uv)) / (2 * STEP)
    return Jc, Jo


def covariances(g):
    """dict: cam_cov [C,6,6], obj_cov [O,6,6] (zeros: fixed, NaN: free without a counted edge), status [2] = NaN blocks, H (dense, over the vertices in the
    system), Sigma = inv(H), cond = cond(H)."""
    C, O, E = len(g["cam_T"]), len(g["obj_T"]), len(g["edge_cam"])
    cfix, ofix = np.asarray(g["cam_fixed"]).astype(bool), np.asarray(g["obj_fixed"]).astype(bool)
    counted = [e for e in range(E) if g["edge_inlier"][e] and not (cfix[g["edge_cam"][e]] and ofix[g["edge_obj"][e]])]
    cam_n, obj_n = np.zeros(C, int), np.zeros(O, int)
    for e in counted:
        cam_n[g["edge_cam"][e]] += 1
        obj_n[g["edge_obj"][e]] += 1
    col, n = {}, 0
    for c in range(C):
        if not cfix[c] and cam_n[c] > 0:
            col[("c", c)] = n
            n += 6
    for o in range(O):
        if not ofix[o] and obj_n[o] > 0:
            col[("o", o)] = n
            n += 6
    H = np.zeros((n, n))
    for e in counted:
        Jc, Jo = edge_jacobians(g, e)
        i = g["edge_info"][e]
        Om = np.array([[i[0], i[1]], [i[1], i[2]]])
        J = np.zeros((2, n))
        if ("c", int(g["edge_cam"][e])) in col:
            a = col[("c", int(g["edge_cam"][e]))]
            J[:, a:a + 6] = Jc
        if ("o", int(g["edge_obj"][e])) in col:
            a = col[("o", int(g["edge_obj"][e]))]
            J[:, a:a + 6] = Jo
        H += J.T @ Om @ J
    Sigma = np.linalg.inv(H) if n else np.zeros((0, 0))
    cam_cov, obj_cov = np.zeros((C, 6, 6)), np.zeros((O, 6, 6))
    for c in range(C):
        if not cfix[c]:
            a = col.get(("c", c))
            cam_cov[c] = np.nan if a is None else Sigma[a:a + 6, a:a + 6]
    for o in range(O):
        if not ofix[o]:
            a = col.get(("o", o))
            obj_cov[o] = np.nan if a is None else Sigma[a:a + 6, a:a + 6]
    status = np.array([int(np.isnan(cam_cov[:, 0, 0]).sum()), int(np.isnan(obj_cov[:, 0, 0]).sum())])
    return {"cam_cov": cam_cov, "obj_cov": obj_cov, "status": status, "H": H, "Sigma": Sigma, "cond": float(np.linalg.cond(H)) if n else 1.0}


def bound(ref):
    """|Sigma_hip - Sigma_ref| <= 1e3 eps cond(H_ref) max|Sigma_ref|: the forward-error bound of an inverse through Cholesky (constant for n <= 200)."""
    return 1e3 * np.finfo(np.float64).eps * ref["cond"] * float(np.abs(ref["Sigma"]).max())
