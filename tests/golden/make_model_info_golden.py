"""Pin the model-statistics row (N8) against the REFERENCE's vendored bop_toolkit (imported from /root/reference in the build container, the way
tests/golden/make_gt_info_golden.py imports it: the ``np.float`` shim and the absent codec modules stubbed).

scripts/calc_model_info.py itself cannot be run with runpy under Python 3 -- it subscripts a ``map`` object -- so its steps are followed here, one by one,
with the toolkit's OWN functions instead: ``inout.load_ply`` on the PLY files of tests/golden/model_info_cases.py (binary little-endian float files and one
ascii file printed with %.9g), the per-axis minimum, the per-axis maximum minus that minimum taken as Python floats, ``misc.calc_pts_diameter``, and
``inout.save_json`` for the file.

Recorded (tests/golden/model_info_golden.npz): the text of models_info.json as save_json wrote it and the seven numbers per model as float64.  As a sanity
check of the fixture, ``calc_pts_diameter2`` (scipy's cdist) must agree with the recorded diameter to 1 ulp on every case; without scipy the same
N x N matrix of Euclidean distances is formed with numpy.

    python tests/golden/make_model_info_golden.py
"""
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TOOLKIT = "/root/reference/thirdparty/bop_toolkit"
sys.path.insert(0, ROOT)
sys.path.insert(0, TOOLKIT)
np.float = float                                  # the vendored toolkit predates numpy 1.24
for _absent in ("imageio", "png"):                # image codecs imported at the top of inout.py; not used here
    sys.modules.setdefault(_absent, types.ModuleType(_absent))

from bop_toolkit_lib import inout, misc  # noqa: E402

from tests.golden import model_info_cases as MC  # noqa: E402

KEYS = ("min_x", "min_y", "min_z", "size_x", "size_y", "size_z", "diameter")


def diameter2(pts):
    try:
        return float(misc.calc_pts_diameter2(pts))
    except (NameError, AttributeError, ImportError):              # no scipy: cdist(pts, pts, 'euclidean').max() by hand
        best = 0.0
        for i0 in range(0, len(pts), 256):
            d = pts[i0:i0 + 256, None, :] - pts[None, :, :]
            best = max(best, float(np.sqrt((d * d).sum(axis=2)).max()))
        return best


if __name__ == "__main__":
    cases = MC.models()
    models_info = {}
    with tempfile.TemporaryDirectory() as tmp:
        MC.write_models(tmp)
        for obj_id in range(1, len(cases) + 1):
            model = inout.load_ply(os.path.join(tmp, f"obj_{obj_id:06d}.ply"))
            assert model["pts"].dtype == np.float64 and np.array_equal(model["pts"], cases[obj_id - 1][1].astype(np.float64)), obj_id
            # The script's steps (calc_model_info.py:37-48): the box's corner, its extent, the diameter.  The script subtracts the corner as a sequence
            # of Python floats from the fp64 array of maxima; numpy converts such a sequence to an fp64 array first, so array - array is that subtraction.
            pts = model["pts"]
            lo, hi = pts.min(axis=0), pts.max(axis=0)
            values = [float(v) for v in lo] + [float(v) for v in hi - np.array(lo.tolist(), np.float64)] + [misc.calc_pts_diameter(pts)]
            models_info[obj_id] = dict(zip(KEYS, values))
            diameter, d2 = values[6], diameter2(pts)
            assert abs(d2 - diameter) <= np.spacing(diameter), (obj_id, d2, diameter)
            print(f"{obj_id:2d} {cases[obj_id - 1][0]:18s} n={len(model['pts']):5d}", models_info[obj_id])
        path = os.path.join(tmp, "models_info.json")
        inout.save_json(path, models_info)
        with open(path, "r") as f:
            text = f.read()
    out = {"text": np.frombuffer(text.encode(), np.uint8), "info": np.array([[models_info[o][k] for k in KEYS] for o in sorted(models_info)], np.float64)}
    path = os.path.join(ROOT, "tests", "golden", "model_info_golden.npz")
    np.savez_compressed(path, **out)
    print("recorded", {k: v.shape for k, v in out.items()}, os.path.getsize(path), "bytes")
