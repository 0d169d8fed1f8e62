"""Pin the host side and the error arithmetic of the BOP-19 VSD chain (row N6) against the REFERENCE's vendored bop_toolkit (imported from /root/reference in
the build container).  The toolkit's renderer needs OpenGL; ``pose_error.vsd`` is therefore run with a stub renderer whose ``render_object`` returns the
depth images of the numpy rasteriser of tests/vsd_ref.py -- what is pinned is everything after the renderer.  Recorded (tests/golden/vsd_golden.npz,
results and two small meshes only):

    inout.load_ply                          points and faces of an ascii and a binary file of the synthetic tree of tests/bop_tree.py
    misc.overlapping_sphere_projections     on the designed cases of tests/golden/vsd_cases.py
    pose_error.vsd                          on its seeded pairs (occluded scenes, missing depth, empty union, est == gt; both normalisations)
    pose_matching.match_poses_scene + score.calc_localization_scores     on a VSD error table, per tau and threshold

    python tests/golden/make_vsd_golden.py
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference/thirdparty/bop_toolkit")
np.float = float                                  # the vendored toolkit predates numpy 1.24
import types  # noqa: E402
for _absent in ("imageio", "png"):                # image codecs imported at the top of inout.py; nothing here touches them
    sys.modules.setdefault(_absent, types.ModuleType(_absent))

from bop_toolkit_lib import inout, misc, pose_error, pose_matching, score  # noqa: E402

from tests import bop_tree  # noqa: E402
from tests import vsd_ref as VR  # noqa: E402
from tests.golden import vsd_cases as VC  # noqa: E402


class StubRenderer:
    """``render_object`` of renderer.Renderer for pose_error.vsd: depth from the numpy rasteriser."""

    def __init__(self, models):
        self.models = models

    def render_object(self, obj_id, R, t, fx, fy, cx, cy):
        _, p, f, _ = self.models[obj_id]
        K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
        return {"depth": VR.render_depth(p, f, np.hstack((R, np.reshape(t, (3, 1)))), K, VC.W, VC.H)}


if __name__ == "__main__":
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        desc = bop_tree.build(tmp, **VC.PLY_TREE)
        for oid in (1, 2):
            model = inout.load_ply(os.path.join(desc["data_root"], "models_eval", f"obj_{oid:06d}.ply"))
            out[f"ply{oid}_pts"], out[f"ply{oid}_faces"] = np.asarray(model["pts"], np.float64), np.asarray(model["faces"], np.float64)
    out["sphere"] = np.array([bool(misc.overlapping_sphere_projections(r, np.array(p1), np.array(p2))) for r, p1, p2 in VC.SPHERE_CASES])

    models = VC.models()
    ren = StubRenderer(models)
    errs = []
    for p in VC.vsd_pairs():
        diam = models[p["m"]][3]
        e = pose_error.vsd(p["Te"][:, :3], p["Te"][:, 3:], p["Tg"][:, :3], p["Tg"][:, 3:], p["test"], p["K"], VC.DELTA, list(VC.TAUS), p["normalized"], diam, ren,
                           p["m"], "step")
        errs.append(e)
        de, dg = (ren.render_object(p["m"], T[:, :3], T[:, 3:], 150.0, 150.0, 80.0, 48.0)["depth"] for T in (p["Te"], p["Tg"]))
        m_delta, m_tau = VR.decision_margins(de, dg, p["test"], p["K"], VC.DELTA, VC.TAUS, p["normalized"], diam)
        assert m_delta > 1e-6 and m_tau > 1e-9, (p["label"], m_delta, m_tau)          # no recorded pixel decides on a rounding
        mine = VR.vsd_from_depth(de, dg, p["test"], p["K"], VC.DELTA, VC.TAUS, p["normalized"], diam)[0]
        print(p["label"], "margins", m_delta, m_tau, "toolkit", np.round(e, 4)[[0, 4, 9]], "equal to tests/vsd_ref.py:", list(e) == list(mine))
    out["vsd_errors"] = np.array(errs, np.float64)

    gt_obj_ids, gt_valid, inst_count, ests = VC.vsd_match_case()
    scene_gt = {im: [{"obj_id": o} for o in objs] for im, objs in gt_obj_ids.items()}
    ths = np.arange(0.05, 0.51, 0.05)
    est_of_gt, recalls = [], []
    for t in range(len(VC.TAUS)):
        scene_errs = []
        for (im, o), rows in ests.items():
            kept = sorted(enumerate(rows), key=lambda x: x[1]["score"], reverse=True)[slice(0, inst_count[(im, o)])]      # eval_calc_errors.py:258-262
            for est_id, r in kept:
                scene_errs.append({"im_id": im, "obj_id": o, "est_id": est_id, "score": r["score"], "errors": {g: [e[t]] for g, e in r["errors"].items()}})
        for th in ths:
            matches = pose_matching.match_poses_scene(1, scene_gt, gt_valid, scene_errs, [th], -1)
            sc = score.calc_localization_scores([1], list(range(1, 8)), matches, -1, do_print=False)
            est_of_gt.append([mt["est_id"] for mt in matches])
            recalls.append(sc["recall"])
    out["match_vsd_est"] = np.array(est_of_gt, np.int64).reshape(len(VC.TAUS), len(ths), -1)
    out["match_vsd_recall"] = np.array(recalls, np.float64).reshape(len(VC.TAUS), len(ths))
    path = os.path.join(ROOT, "tests", "golden", "vsd_golden.npz")
    np.savez_compressed(path, **out)
    print("recorded", {k: v.shape for k, v in out.items()}, os.path.getsize(path), "bytes; sphere", out["sphere"], "mean recall", out["match_vsd_recall"].mean())
