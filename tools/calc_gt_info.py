"""scene_gt_info.json (and, with --masks, mask/ and mask_visib/) for the scenes of a BOP-format split, computed on the device (row N7): a thin command line
over suo_slam_amd.bop_gt_info.calc_scene_gt_info, in place of bop_toolkit's scripts/calc_gt_info.py and scripts/calc_gt_masks.py.

    python tools/calc_gt_info.py <dataset dir> <split> <model dir> [--delta 15] [--masks] [--scenes 1 2 ...]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from suo_slam_amd import bop, bop_eval, bop_gt_info  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("dataset_dir", help="the dataset's folder, e.g. <bop root>/tless")
    ap.add_argument("split", help="the split's folder name under it, e.g. test_primesense")
    ap.add_argument("model_dir", help="folder with models_info.json and obj_%%06d.ply, absolute or under the dataset's folder (e.g. models_cad)")
    ap.add_argument("--delta", type=float, default=15.0, help="tolerance of the visibility test in mm (5 for ITODD)")
    ap.add_argument("--masks", action="store_true", help="also write mask/ and mask_visib/")
    ap.add_argument("--scenes", type=int, nargs="*", default=None, help="scene ids; default: all")
    a = ap.parse_args(argv)
    model_dir = a.model_dir if os.path.isabs(a.model_dir) else os.path.join(a.dataset_dir, a.model_dir)
    errors = bop_eval.BopErrors(bop.load_mesh_db(model_dir, faces=True), bop_eval.load_models_info(model_dir))
    delta = int(a.delta) if float(a.delta).is_integer() else a.delta
    out = bop_gt_info.calc_scene_gt_info(errors, os.path.join(a.dataset_dir, a.split), scene_ids=a.scenes, delta=delta, masks=a.masks, write=True)
    errors.close()
    for scene_id, info in out.items():
        print(f"scene {scene_id}: {len(info)} images, {sum(len(v) for v in info.values())} instances")


if __name__ == "__main__":
    main()
