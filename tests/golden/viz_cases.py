"""The designed views of the visualisation fixture (tests/golden/make_viz_golden.py -> viz_golden.npz; tests/test_viz_ref.py and tests/test_gpu_viz.py rebuild
them from here).  Pure numpy: a case is the ObjectSLAM state collect_results(no_viz=False) reads for ONE view, plus the frame and the meshes.

Each case is the smallest view at which a rule can go wrong; what it is for stands at its builder.  Canvases are 150 x 117 and 160 x 120: no side is a multiple
of 64 or of the kernel's 64 x 4 tile.  Every K and every pose is exactly representable in float32, so that the reference (which casts both to float32) and the
product (fp64) start from the same numbers; mesh points whose projection lies within 1e-3 px of a pixel boundary are dropped (drop_boundary_points), so that
the reference's float32 projection and the fp64 rule pick the same pixels."""
import numpy as np

from tests import viz_ref

NUM_KP = 41
VIEW = 7                                            # the view id of every case


def camera(W, H):
    return np.array([[150.5, 0.0, W / 2 - 0.75], [0.0, 149.25, H / 2 + 0.25], [0.0, 0.0, 1.0]], np.float32).astype(np.float64)


def fix_K_for_bbox_ndc(K_, bbox):                   # lib/utils/utils.py:416-429
    x1, y1, x2, y2 = bbox
    x, y, w, h = x1, y1, x2 - x1, y2 - y1
    T = np.eye(3)
    T[:2, 2] = -np.array([x, y], dtype=np.float64)
    S = np.eye(3)
    S[0, :] *= 2.0 / w
    S[1, :] *= -2.0 / h
    S[0, 2] -= 1
    S[1, 2] += 1
    return S @ T @ np.copy(K_)


def frame(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def detection(K, bbox, pixels, channels, cov_pix=None, prior_pixels=None, prior_channels=None):
    """A detection whose keypoints of ``channels`` land at ``pixels`` [n,2] of the full image (up to rounding: the targets sit a quarter pixel off the centres),
    with pixel-space covariances ``cov_pix`` [n,2,2] and prior keypoints of ``prior_channels`` at ``prior_pixels``."""
    bbox = np.asarray(bbox, np.float64)
    Kb = fix_K_for_bbox_ndc(K, bbox).astype(np.float32).astype(np.float64)
    w, h = bbox[2] - bbox[0], bbox[3] - bbox[1]

    def ndc(px):
        px = np.asarray(px, np.float64).reshape(-1, 2)
        return np.stack((2 * (px[:, 0] - bbox[0]) / w - 1, 1 - 2 * (px[:, 1] - bbox[1]) / h), axis=1)
    order = np.argsort(channels, kind="stable")
    kp_mask = np.zeros(NUM_KP, bool)
    kp_mask[list(channels)] = True
    det = {"pose": None, "inliers": np.ones(len(channels), bool), "model_kp": np.zeros((len(channels), 3)), "uv_pred": ndc(pixels)[order],
           "cov_pred": None, "K": Kb, "bbox": bbox, "kp_mask": kp_mask, "model_kp_mask": np.zeros(NUM_KP, bool), "prior_uv": None, "uv_gt": None, "score": 1.0}
    if cov_pix is not None:
        a = np.array([w / 2, -h / 2])
        det["cov_pred"] = (np.asarray(cov_pix, np.float64)[order] / (a[:, None] * a[None, :])).astype(np.float32)
    if prior_pixels is not None:
        pu = np.zeros((NUM_KP, 2))
        pu[list(prior_channels)] = ndc(prior_pixels)
        det["prior_uv"] = pu
        det["model_kp_mask"][list(prior_channels)] = True
    return det


def cov_with(axis_a, axis_b, angle_deg):
    """A pixel-space covariance whose ellipse has about those half-axes: axis = round((2 / 3) sqrt(5.991 lambda))."""
    lam = [(1.5 * axis_a) ** 2 / 5.991, (1.5 * axis_b) ** 2 / 5.991]
    c, s = np.cos(np.deg2rad(angle_deg)), np.sin(np.deg2rad(angle_deg))
    R = np.array([[c, -s], [s, c]])
    return R @ np.diag(lam) @ R.T


def pose(t, rz_deg=0.0):
    c, s = np.cos(np.deg2rad(rz_deg)), np.sin(np.deg2rad(rz_deg))
    T = np.eye(4)
    T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    T[:3, 3] = t
    return T.astype(np.float32).astype(np.float64)


def patch(n, step, extra=()):
    """An n x n grid of points on the object's z = 0 plane, ``step`` mm apart, plus ``extra`` points."""
    g = (np.arange(n) - (n - 1) / 2) * step
    p = np.stack(list(np.meshgrid(g, g, indexing="xy")) + [np.zeros((n, n))], axis=-1).reshape(-1, 3)
    return np.concatenate((p, np.asarray(extra, np.float64).reshape(-1, 3))).astype(np.float32)


def drop_boundary_points(points, T, K, H, W, margin=1e-3):
    """The points whose projected u + 0.5 and v + 0.5 stay ``margin`` away from every integer (the others dropped, in order)."""
    uh, vh = viz_ref.project(points, T, K)
    far = lambda a: ~np.isfinite(a) | (np.abs(a - np.rint(a)) >= margin)        # noqa: E731
    return np.ascontiguousarray(points[far(uh) & far(vh)])


def _case(name, H, W, seed, detections, obj_poses, meshes, viz_cov=False, no_network_cov=True, cam_pose=None):
    K = camera(W, H)
    cam_pose = np.eye(4) if cam_pose is None else cam_pose
    to4 = lambda T: np.concatenate((T, np.eye(4)[3:4, :]), axis=0) if T.shape[0] == 3 else T        # noqa: E731
    meshes = {o: drop_boundary_points(p, to4(cam_pose) @ to4(obj_poses[o]), K, H, W) if o in obj_poses else p for o, p in meshes.items()}
    return {"name": name, "H": H, "W": W, "frame": frame(H, W, seed), "K": K, "cam_pose": cam_pose, "detections": detections, "obj_poses": obj_poses,
            "meshes": meshes, "viz_cov": viz_cov, "no_network_cov": no_network_cov}


def case_empty():
    """A view with no objects at all: three copies of the frame."""
    return _case("empty", 117, 150, 1, {}, {}, {})


def case_keypoints():
    """Discs crossing each of the four borders; centres one pixel off the canvas on each side (nothing is drawn, not even the visible part); two and three
    overlapping keypoints, within one object (channel order decides) and across objects (obj_ids order decides); a box partly outside, one with a negative
    x1 (its prior window is then whatever Python's slice yields), one wholly outside."""
    W, H = 150, 117
    K = camera(W, H)
    q = 0.25
    d = {
        3: detection(K, [20.4, 15.2, 90.7, 80.1], [[3 + q, 50 + q], [146 + q, 60 + q], [70 + q, 2 + q], [75 + q, 114 + q], [40 + q, 40 + q], [46 + q, 43 + q], [43 + q, 47 + q]],
                     [0, 5, 9, 12, 20, 21, 40]),
        1: detection(K, [-12.3, 60.0, 60.2, 130.9], [[-1 + q, 30 + q], [150 + q, 30 + q], [30 + q, -1 + q], [30 + q, 117 + q], [0 + q, 0 + q], [149 + q, 116 + q], [44 + q, 45 + q]],
                     [1, 2, 3, 4, 6, 7, 30]),
        5: detection(K, [100.0, -20.0, 170.0, 50.0], [[120 + q, 20 + q], [126 + q, 22 + q]], [8, 10]),
        9: detection(K, [200.0, 30.0, 260.0, 90.0], [[100 + q, 100 + q]], [11]),
    }
    return _case("keypoints", H, W, 2, d, {}, {})


def case_ellipses():
    """viz_cov: half-axes 0, 1, 2 and large, at several angles (0 and 90 degrees among the constructions), ellipses crossing the borders, and an ellipse
    painted over a neighbour's discs."""
    W, H = 160, 120
    K = camera(W, H)
    q = 0.25
    px = [[20 + q, 20 + q], [50 + q, 20 + q], [80 + q, 20 + q], [110 + q, 20 + q], [140 + q, 20 + q], [30 + q, 70 + q], [80 + q, 70 + q], [88 + q, 74 + q], [150 + q, 100 + q],
          [5 + q, 110 + q]]
    cov = [cov_with(0.0, 0.0, 0), cov_with(1, 0.0, 0), cov_with(1, 2, 90), cov_with(2, 2, 30), cov_with(3, 9, 0), cov_with(25, 6, 90), cov_with(14, 5, 37), cov_with(5, 14, 135),
           cov_with(40, 12, 60), cov_with(18, 1, 10)]
    d = {2: detection(K, [10.0, 8.0, 155.0, 115.0], px, [0, 3, 6, 9, 12, 15, 18, 21, 24, 27], cov_pix=cov)}
    return _case("ellipses", H, W, 3, d, {}, {}, viz_cov=True, no_network_cov=False)


def case_priors():
    """Prior heat: windows clipped by the canvas (a stamp centred near a corner) and by the object's box; two objects sharing channels at the same place, so
    that the clip at 1 acts; several channels on one pixel, so that the sum of colours exceeds 255; a box with negative x1, whose window Python's slice
    leaves empty; boxes drawn before the blend."""
    W, H = 150, 117
    K = camera(W, H)
    q = 0.25
    d = {
        3: detection(K, [30.2, 20.3, 120.6, 100.4], [[60 + q, 50 + q]], [0], prior_pixels=[[70 + q, 60 + q], [72 + q, 58 + q], [74 + q, 62 + q], [35 + q, 95 + q]], prior_channels=[0, 2, 5, 7]),
        6: detection(K, [50.0, 40.0, 149.4, 116.4], [[100 + q, 80 + q]], [1], prior_pixels=[[70 + q, 60 + q], [73 + q, 61 + q], [145 + q, 112 + q]], prior_channels=[0, 2, 9]),
        4: detection(K, [-8.6, 5.0, 40.0, 45.0], [[10 + q, 10 + q]], [4], prior_pixels=[[12 + q, 14 + q]], prior_channels=[11]),
        8: detection(K, [0.4, 60.2, 48.0, 116.7], [[20 + q, 90 + q]], [6], prior_pixels=[[2 + q, 114 + q], [30 + q, 70 + q]], prior_channels=[13, 12]),
    }
    return _case("priors", H, W, 4, d, {}, {})


def case_overlay():
    """Meshes: pairs overlapping in both depth orders against the obj_ids order, a pair of equal depth (the stable sort decides), a mesh crossing the canvas
    border (the dilation does not wrap), points behind the camera (they project, and are painted: no depth test), a point with z = 0 and a point projecting
    into (-1, 0)."""
    W, H = 160, 120
    K = camera(W, H)
    obj_poses = {
        1: pose([-60.0, -40.0, 600.0]), 2: pose([-40.0, -30.0, 500.0], 20),           # 2 nearer than 1: painted over it
        3: pose([70.0, -40.0, 450.0]), 4: pose([85.0, -25.0, 640.0], -15),            # 4 farther than 3: 3 stays on top
        5: pose([-30.0, 70.0, 550.0]), 6: pose([-10.0, 80.0, 550.0], 45),             # equal depth: obj_ids order
        7: pose([300.0, 200.0, 560.0]),                                               # across the right and bottom borders
        10: pose([0.0, 0.0, 500.0]),
    }
    meshes = {o: patch(36, 3.0) for o in (1, 2, 3, 4, 5, 6)}
    meshes[7] = patch(30, 6.0)
    Kx, Ky = K[0, 2], K[1, 2]
    # object 10: a few points in front; behind the camera (z = -900 -> Z = -400: projects mirrored onto the canvas); Z = 0 exactly; into (-1, 0): u + 0.5 = -0.4
    into = [(-0.9 - Kx) * 500.0 / K[0, 0], (30.3 - Ky) * 500.0 / K[1, 1], 0.0]
    meshes[10] = np.concatenate((patch(5, 2.0), np.array([[40.0, 30.0, -900.0], [-55.0, 20.0, -900.0], [10.0, 10.0, -500.0], into], np.float32)))
    return _case("overlay", H, W, 5, {}, obj_poses, meshes)


def case_all():
    """Everything at once, as a SLAM view has it: detected objects with and without a map pose, a map object that is not detected (its zero box row is drawn
    at the corner in the table's last colour), priors, ellipses, a camera pose that is not the identity and is stored as 3 x 4."""
    W, H = 150, 117
    K = camera(W, H)
    q = 0.25
    cam = pose([5.0, -3.0, 10.0], 3)
    d = {
        2: detection(K, [15.5, 12.5, 80.5, 70.5], [[30 + q, 30 + q], [50 + q, 44 + q], [36 + q, 33 + q]], [2, 17, 33], cov_pix=[cov_with(9, 4, 20), cov_with(2, 1, 70), cov_with(12, 12, 0)],
                     prior_pixels=[[40 + q, 40 + q], [60 + q, 50 + q]], prior_channels=[2, 17]),
        12: detection(K, [70.2, 50.9, 148.7, 115.1], [[100 + q, 80 + q], [140 + q, 110 + q]], [0, 40], cov_pix=[cov_with(6, 3, 100), cov_with(20, 2, 45)]),
    }
    obj_poses = {12: pose([40.0, 30.0, 520.0], 10)[:3], 30: pose([-50.0, -20.0, 480.0], -30), 2: pose([-20.0, -10.0, 700.0])}
    meshes = {12: patch(30, 3.0), 30: patch(30, 3.0), 2: patch(40, 4.0)}
    return _case("all", H, W, 6, d, obj_poses, meshes, viz_cov=True, no_network_cov=False, cam_pose=cam[:3])


def all_cases():
    return [case_empty(), case_keypoints(), case_ellipses(), case_priors(), case_overlay(), case_all()]


def install(slam, case):
    """Put the case into an ObjectSLAM-shaped object (the reference's class or the product's) as its only view; ``points`` become what that class reads."""
    import copy
    c = copy.deepcopy(case)
    slam.detections = {VIEW: c["detections"]}
    slam.cam_poses = {VIEW: c["cam_pose"]}
    slam.obj_poses = c["obj_poses"]
    slam.view_ids = [VIEW]
    slam.cam_K = {VIEW: c["K"]}
    slam.images = {VIEW: c["frame"]}
    slam.needs_opt = False
    slam.no_network_cov = c["no_network_cov"]
    slam.viz_cov = c["viz_cov"]
    return slam
