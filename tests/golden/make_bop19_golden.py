"""Pin the BOP-19 MSSD / MSPD chain (row N5) against the REFERENCE's vendored bop_toolkit (imported from /root/reference in the build container): runs
``misc.get_symmetry_transformations``, ``pose_error.mssd`` / ``mspd`` and ``pose_matching.match_poses_scene`` + ``score.calc_localization_scores`` on the
seeded inputs of tests/golden/bop19_cases.py and stores what the toolkit returned (tests/golden/bop19_golden.npz: results only, a few KB).

    python tests/golden/make_bop19_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference/thirdparty/bop_toolkit")
np.float = float                                  # the vendored toolkit predates numpy 1.24
import types  # noqa: E402
for _absent in ("imageio", "png"):                # image codecs imported at the top of inout.py; nothing here touches them
    sys.modules.setdefault(_absent, types.ModuleType(_absent))

from bop_toolkit_lib import misc, pose_error, pose_matching, score  # noqa: E402

from tests.golden import bop19_cases as BC  # noqa: E402


def toolkit_syms(name, step):
    return misc.get_symmetry_transformations(BC.SYM_INFOS[name], step)


if __name__ == "__main__":
    out = {}
    for name in BC.SYM_INFOS:
        for step in BC.SYM_STEPS:
            tr = toolkit_syms(name, step)
            out[f"sym_{name}_{step}"] = np.stack([np.hstack((t["R"], t["t"])) for t in tr]).astype(np.float64)
    sets = {name: toolkit_syms(name, 0.01) for name in BC.SYM_INFOS}
    pairs = BC.pairs(lambda name: out[f"sym_{name}_0.01"])
    pts = {m: BC.model_points(m).astype(np.float64) for m in range(len(BC.MODELS))}
    mssd, mspd = [], []
    for m, Te, Tg, K in pairs:
        syms = sets[BC.MODELS[m][1]]
        mssd.append(pose_error.mssd(Te[:, :3], Te[:, 3:], Tg[:, :3], Tg[:, 3:], pts[m], syms))
        mspd.append(pose_error.mspd(Te[:, :3], Te[:, 3:], Tg[:, :3], Tg[:, 3:], K, pts[m], syms))
    out["mssd"], out["mspd"] = np.array(mssd, np.float64), np.array(mspd, np.float64)

    gt_obj_ids, gt_valid, inst_count, ests = BC.match_case()
    scene_gt = {im: [{"obj_id": o} for o in objs] for im, objs in gt_obj_ids.items()}
    for scale, ths, tag in ((1.0, np.arange(0.05, 0.51, 0.05), "mssd"), (100.0, np.arange(5, 51, 5), "mspd")):
        scene_errs = []
        for (im, o), rows in ests.items():
            kept = sorted(enumerate(rows), key=lambda x: x[1]["score"], reverse=True)[slice(0, inst_count[(im, o)])]      # eval_calc_errors.py:258-262
            for est_id, r in kept:
                scene_errs.append({"im_id": im, "obj_id": o, "est_id": est_id, "score": r["score"], "errors": {g: [scale * e] for g, e in r["errors"].items()}})
        est_of_gt, recalls = [], []
        for th in ths:
            matches = pose_matching.match_poses_scene(1, scene_gt, gt_valid, scene_errs, [th], -1)
            sc = score.calc_localization_scores([1], list(range(1, 8)), matches, -1, do_print=False)
            est_of_gt.append([mt["est_id"] for mt in matches])
            recalls.append(sc["recall"])
        out[f"match_{tag}_est"] = np.array(est_of_gt, np.int64)
        out[f"match_{tag}_recall"] = np.array(recalls, np.float64)
        out[f"match_{tag}_targets"] = np.array(sc["targets_count"], np.int64)
    path = os.path.join(ROOT, "tests", "golden", "bop19_golden.npz")
    np.savez_compressed(path, **out)
    print("recorded", len(mssd), "pairs;", {k: v.shape for k, v in out.items() if k.startswith("sym_")}, os.path.getsize(path), "bytes")
    print("mssd", out["mssd"][:8], "mspd", out["mspd"][:8], "recall", out["match_mssd_recall"], out["match_mspd_recall"])
