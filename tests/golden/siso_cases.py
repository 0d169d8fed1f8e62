"""Seeded inputs of the SISO goldens and tests (row N4), shared by tests/golden/make_siso_golden.py (which runs the REFERENCE's vendored bop_toolkit scripts
on them, build container only) and by the tests (which regenerate them, so tests/golden/siso_golden.npz holds results only).  Nothing here comes from the
toolkit.

The tree: two scenes of 160 x 96 images under K0 with the two small meshes of tests/golden/vsd_cases.py (object id = model index + 1: 1 the box, 2 the
icosphere).  What it was designed to hold:
    scene 1, image 0    two instances of object 1, the second behind a slab (visib_fract below 0.1, above 0), inst_count 2; three estimates of object 1 --
                        the best-scored one the worse pose of the first instance, so that n_top = 1 takes the worse one, the third one on the hidden
                        instance; object 2 with est == gt
    scene 1, image 4    object 1 with an estimate whose spheres (and sphere projections) do not overlap the ground truth's; object 2 a target without an
                        estimate
    scene 5, image 2    object 1 with an estimate that fails the translation element of rete only; object 2 with a near estimate
    scene 5, image 3    object 2 half a radian off (ADD large, ADI small: the icosphere is the symmetric object of ``ad``); an estimate of object 1, which
                        is no target of the image
"""
import numpy as np

from tests import gt_info_ref as GR
from tests import vsd_ref as VR
from tests.golden import bop19_cases as BC
from tests.golden import vsd_cases as VC

W, H = VC.W, VC.H
K0 = VC.K0
DELTA = 15
DEPTH_SCALE = 0.1
SYMMETRIC_OBJ_IDS = (2,)
SCENE_IDS = (1, 5)
OBJ_IDS = (1, 2)
RESULT_NAME = "suo_tless-test"                    # <method>_<dataset>-<split>: the results file is RESULT_NAME + ".csv"
TARGETS_FILENAME = "all_target_tless.json"

# the runs of the two scripts that are recorded: (error type, n_top, visib_gt_min, correct_th or None for the script's default)
VSD = dict(vsd_delta=DELTA, vsd_taus=[20.0], vsd_normalized_by_diameter=False)
RUNS = [(et, n_top, vmin, None) for et in ("vsd", "add", "adi", "ad", "proj", "cus", "rete") for n_top, vmin in ((1, 0.1), (1, -1), (-1, 0.1), (-1, -1), (0, 0.1))]
RUNS += [("rete", 1, 0.1, [5.0, 10.0]), ("vsd", 1, 0.1, [0.6]), ("proj", 0, -1, [2.0])]


def models():
    return VC.models()[:2]


def models_info():
    return {i + 1: {"diameter": m[3]} for i, m in enumerate(models())}


def mesh_db():
    return {i + 1: {"points": m[1], "faces": m[2]} for i, m in enumerate(models())}


def _perturb(rng, T, rot, trans):
    return BC.compose(T, np.hstack((BC.rotvec(rng.standard_normal(3) * rot), rng.standard_normal((3, 1)) * trans)))


def tree(seed=61):
    """``{"scenes": {scene_id: {im_id: {"K", "gts": [(obj_id, T [3,4])], "raw" uint16 [H,W]}}}, "targets": [...], "ests": [{"scene_id", "im_id", "obj_id",
    "score", "T"}] in the order of the results file}``."""
    rng = np.random.default_rng(seed)
    ms = models()

    def raw_of(gts, slab=None):
        depth = np.full((H, W), VC.BACKGROUND, np.float32)
        for o, T in gts:
            d = VR.render_depth(ms[o - 1][1], ms[o - 1][2], T, K0, W, H)
            depth = np.where((d > 0) & (d < depth), d, depth)
        if slab is not None:
            depth[:, slab[0]:slab[1]] = 180.0
        return np.round(depth / np.float32(DEPTH_SCALE)).astype(np.uint16)

    scenes, ests, targets = {1: {}, 5: {}}, [], []

    def est(s, im, o, score, T):
        ests.append({"scene_id": s, "im_id": im, "obj_id": o, "score": score, "T": T})

    a, b, c = VC.pose(rng, (38.0, 30.0), 350.0), VC.pose(rng, (112.0, 62.0), 380.0), VC.pose(rng, (72.0, 66.0), 400.0)
    gts = [(1, a), (2, c), (1, b)]
    scenes[1][0] = {"K": K0.copy(), "gts": gts, "raw": raw_of(gts, slab=(97, 140))}
    targets += [{"scene_id": 1, "im_id": 0, "obj_id": 1, "inst_count": 2}, {"scene_id": 1, "im_id": 0, "obj_id": 2, "inst_count": 1}]
    est(1, 0, 1, 0.5, _perturb(rng, a, 0.02, 1.0))                            # the better pose, scored lower
    est(1, 0, 2, 0.8, c.copy())                                               # est == gt
    est(1, 0, 1, 0.9, _perturb(rng, a, 0.35, 9.0))                            # the worse pose, scored best
    est(1, 0, 1, 0.3, _perturb(rng, b, 0.02, 1.0))                            # on the hidden instance

    a, c = VC.pose(rng, (50.0, 48.0), 340.0), VC.pose(rng, (115.0, 45.0), 370.0)
    gts = [(2, c), (1, a)]
    scenes[1][4] = {"K": K0.copy(), "gts": gts, "raw": raw_of(gts)}
    targets += [{"scene_id": 1, "im_id": 4, "obj_id": 1, "inst_count": 1}, {"scene_id": 1, "im_id": 4, "obj_id": 2, "inst_count": 1}]
    far = a.copy()
    far[0, 3] += 150.0                                                        # more than the box's diameter (107.7) to the side
    est(1, 4, 1, 0.6, far)

    a, c = VC.pose(rng, (45.0, 50.0), 360.0), VC.pose(rng, (110.0, 40.0), 350.0)
    gts = [(1, a), (2, c)]
    scenes[5][2] = {"K": K0.copy(), "gts": gts, "raw": raw_of(gts)}
    targets += [{"scene_id": 5, "im_id": 2, "obj_id": 2, "inst_count": 1}, {"scene_id": 5, "im_id": 2, "obj_id": 1, "inst_count": 1}]
    t_only = BC.compose(a, np.hstack((BC.rotvec(np.array([0.02, -0.02, 0.02])), np.array([[0.0], [0.0], [8.0]]))))      # 2 degrees, 8 mm
    est(5, 2, 1, 0.7, t_only)
    est(5, 2, 2, 0.4, _perturb(rng, c, 0.02, 2.0))

    c = VC.pose(rng, (80.0, 48.0), 380.0)
    gts = [(2, c)]
    scenes[5][3] = {"K": K0.copy(), "gts": gts, "raw": raw_of(gts)}
    targets += [{"scene_id": 5, "im_id": 3, "obj_id": 2, "inst_count": 1}]
    est(5, 3, 2, 0.2, BC.compose(c, np.hstack((BC.rotvec(np.array([0.3, 0.3, 0.25])), np.array([[1.0], [-1.0], [2.0]])))))
    est(5, 3, 1, 0.9, VC.pose(rng, (60.0, 40.0), 350.0))                      # object 1 is no target here
    return {"scenes": scenes, "targets": targets, "ests": ests}


def read_raw(raw):
    return np.asarray(raw).astype(np.float32) * np.float32(DEPTH_SCALE)


def scene_gt(t):
    """``{scene_id: {im_id: [scene_gt.json entries]}}``."""
    return {s: {im: [{"cam_R_m2c": T[:, :3].ravel().tolist(), "cam_t_m2c": T[:, 3].tolist(), "obj_id": int(o)} for o, T in v["gts"]] for im, v in ims.items()}
            for s, ims in t["scenes"].items()}


def scene_gt_info(t):
    """``{scene_id: {im_id: [scene_gt_info.json entries]}}`` by the numpy restatement of calc_gt_info.py (tests/gt_info_ref.py)."""
    ms = models()
    return {s: {im: [GR.gt_info(ms[o - 1][1], ms[o - 1][2], T, v["K"], read_raw(v["raw"]), DELTA) for o, T in v["gts"]] for im, v in ims.items()}
            for s, ims in t["scenes"].items()}


def results_text(t):
    """The results CSV in the form inout.save_bop_results writes (str() of every float: it reads back to the same bits)."""
    lines = ["scene_id,im_id,obj_id,score,R,t,time"]
    for e in t["ests"]:
        lines.append("{},{},{},{},{},{},{}".format(e["scene_id"], e["im_id"], e["obj_id"], e["score"], " ".join(map(str, e["T"][:, :3].flatten().tolist())),
                                                   " ".join(map(str, e["T"][:, 3].flatten().tolist())), -1))
    return "\n".join(lines)


def write_tree(root, t):
    """Writes the tree under ``root``: ``ds/tless/test/<scene>/{scene_camera,scene_gt,scene_gt_info}.json`` and ``depth/``, the targets file,
    ``models_eval/models_info.json`` (no PLY files: the readers of the models are the caller's) and ``results/RESULT_NAME.csv``.  Returns ``ds/tless``."""
    import json
    import os

    from PIL import Image
    base = os.path.join(root, "ds", "tless")
    gt, info = scene_gt(t), scene_gt_info(t)
    for s, ims in t["scenes"].items():
        sdir = os.path.join(base, "test", f"{s:06d}")
        os.makedirs(os.path.join(sdir, "depth"))
        cam = {str(im): {"cam_K": v["K"].ravel().tolist(), "depth_scale": DEPTH_SCALE} for im, v in ims.items()}
        for name, obj in (("scene_camera.json", cam), ("scene_gt.json", gt[s]), ("scene_gt_info.json", info[s])):
            with open(os.path.join(sdir, name), "w") as f:
                json.dump({str(k): v for k, v in obj.items()}, f)
        for im, v in ims.items():
            Image.fromarray(v["raw"]).save(os.path.join(sdir, "depth", f"{im:06d}.png"))
    with open(os.path.join(base, TARGETS_FILENAME), "w") as f:
        json.dump(t["targets"], f)
    os.makedirs(os.path.join(base, "models_eval"))
    with open(os.path.join(base, "models_eval", "models_info.json"), "w") as f:
        json.dump({str(k): v for k, v in models_info().items()}, f)
    os.makedirs(os.path.join(root, "results"))
    with open(os.path.join(root, "results", RESULT_NAME + ".csv"), "w") as f:
        f.write(results_text(t))
    return base


def tree_pairs(t):
    """Every (estimate, ground truth of the same object and image) of the tree: ``[(model index, T_est, T_gt, K)]``."""
    out = []
    for e in t["ests"]:
        v = t["scenes"][e["scene_id"]][e["im_id"]]
        out += [(o - 1, e["T"], T, v["K"]) for o, T in v["gts"] if o == e["obj_id"]]
    return out


def mask_pairs(seed=67):
    """``[(label, model index, T_est, T_gt, K)]`` for cus / cou_bb_proj: the tree's pairs, then renders that miss each other, an estimate off the image,
    both off the image, a near object whose renders cross the 64-pixel tile boundaries in both directions, and est == gt."""
    rng = np.random.default_rng(seed)
    out = [(f"tree{i}", m, Te, Tg, K) for i, (m, Te, Tg, K) in enumerate(tree_pairs(tree()))]
    out.append(("apart", 0, VC.pose(rng, (30.0, 30.0), 360.0), VC.pose(rng, (125.0, 66.0), 360.0), K0))
    out.append(("est_off_image", 1, VC.pose(rng, (420.0, -300.0), 350.0), VC.pose(rng, (70.0, 50.0), 350.0), K0))
    out.append(("both_off_image", 0, VC.pose(rng, (420.0, -300.0), 350.0), VC.pose(rng, (-300.0, 400.0), 350.0), K0))
    g = VC.pose(rng, (66.0, 62.0), 110.0)
    out.append(("across_tiles", 1, _perturb(rng, g, 0.1, 3.0), g, K0))
    g = VC.pose(rng, (128.0, 64.0), 200.0)
    out.append(("across_tiles_border", 0, _perturb(rng, g, 0.2, 4.0), g, K0))
    g = VC.pose(rng, (90.0, 40.0), 300.0)
    out.append(("same", 1, g.copy(), g, K0))
    return out


# ---- point sets for add / adi / proj: either side of every lane and tile boundary of the kernel ----------------
POINT_COUNTS = (1, 63, 64, 65, 1023, 1025, 3001)
PAIRS_PER_MODEL = 3


def point_models(seed=71):
    """``[float32 [P,3]]`` for P in POINT_COUNTS, |p| <= 110 mm."""
    out = []
    for k, P in enumerate(POINT_COUNTS):
        rng = np.random.default_rng(seed + k)
        out.append((rng.uniform(-1, 1, (P, 3)) * rng.uniform(30, 110, 3)).astype(np.float32))
    return out


def point_pairs(seed=73):
    """``[(model index, T_est, T_gt, K)]``, PAIRS_PER_MODEL per model: a small and a large perturbation and est == gt.  Every pose keeps the object in front
    of the camera with z >= 0.3 |X| for all its points (depth 400 .. 600 mm, points within 191 mm of the origin, centres within 100 px of the principal
    point)."""
    rng = np.random.default_rng(seed)
    out = []
    for m in range(len(POINT_COUNTS)):
        for kind in range(PAIRS_PER_MODEL):
            Tg = VC.pose(rng, (rng.uniform(20, 140), rng.uniform(10, 86)), rng.uniform(400, 600))
            Te = Tg.copy() if kind == 2 else _perturb(rng, Tg, (0.03, 0.6)[kind], (2.0, 25.0)[kind])
            out.append((m, Te, Tg, K0))
    return out
