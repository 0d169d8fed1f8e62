"""models_info.json (3-D bounding box and diameter of every obj_%06d.ply) of a BOP-format model folder, computed on the device (row N8): a thin command
line over suo_slam_amd.bop_model_info.calc_models_info, in place of bop_toolkit's scripts/calc_model_info.py.  What an existing models_info.json holds
besides the seven computed keys (symmetries_discrete, symmetries_continuous, ...) is kept unless --no-keep asks for exactly the toolkit's file.

    python tools/calc_model_info.py <model dir> [--objects 1 2 ...] [--no-keep] [--dry-run]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from suo_slam_amd import bop_model_info  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("model_dir", help="folder with obj_%%06d.ply, e.g. <bop root>/tless/models_cad")
    ap.add_argument("--objects", type=int, nargs="*", default=None, help="object ids; default: every obj_%%06d.ply there")
    ap.add_argument("--no-keep", action="store_true", help="drop what an existing models_info.json holds besides the computed keys, as the toolkit's script does")
    ap.add_argument("--dry-run", action="store_true", help="compute and print, write nothing")
    a = ap.parse_args(argv)
    out = bop_model_info.calc_models_info(a.model_dir, obj_ids=a.objects, keep=not a.no_keep, write=not a.dry_run)
    for obj_id in sorted(out):
        e = out[obj_id]
        if "diameter" in e and "size_x" in e:
            print(f"object {obj_id}: diameter {e['diameter']:.6f}, box {e['size_x']:.6f} x {e['size_y']:.6f} x {e['size_z']:.6f}")
    if not a.dry_run:
        print("wrote", os.path.join(a.model_dir, "models_info.json"))


if __name__ == "__main__":
    main()
