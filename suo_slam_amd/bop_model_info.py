"""models_info.json -- the 3-D bounding box and the diameter of each object model -- from the raw meshes.

Stands in for bop_toolkit's ``scripts/calc_model_info.py`` (with ``misc.calc_pts_diameter``, an O(N^2) scan on the host), the last file of a BOP-format tree
that bop.load_mesh_db, bop_eval.load_models_info and every threshold of the evaluation (fractions of the diameter) needed another tool for:

    model_info(errors_or_db, obj_ids, pairs)        {obj_id: {"min_x", ..., "size_z", "diameter"[, "pair"]}}   -> HIP, csrc/model_info.hip (suo_model_info)
    format_models_info(info)                        the text inout.save_json writes for {obj_id: entry}
    calc_models_info(model_dir, ...)                obj_%06d.ply -> entries -> models_info.json

Input rule.  The result is computed on float32 points (what the mesh database holds), widened exactly to fp64, with the toolkit's arithmetic.  It therefore
equals the toolkit's bit for bit for binary PLY files with float coordinates and for ascii files whose numbers are float32-representable.  For other ascii
files (and double-precision binary ones) the toolkit works on the float64 parse; the inputs then differ by their float32 rounding, and so may the results.

Signed zero.  -0 orders below +0 on the device: where an axis's minimum is zero and the axis holds both zeros, ``min_*`` is -0.0, while the toolkit's numpy
reports whichever zero it meets first (``size_*`` and ``diameter`` are the same either way; with one kind of zero the two agree).

Deviation.  ``calc_model_info.py`` overwrites models_info.json and so drops hand-annotated ``symmetries_discrete`` / ``symmetries_continuous``, which
silently breaks MSSD / MSPD; ``calc_models_info(keep=True)``, the default, carries the keys of an existing file other than the seven computed ones over
(and the entries of objects it was not asked to compute).  ``keep=False`` writes exactly the toolkit's file.  tools/calc_model_info.py is the command line."""
from __future__ import annotations

import ctypes as C
import json
import os
import re

import numpy as np

from . import _lib

KEYS = ("min_x", "min_y", "min_z", "size_x", "size_y", "size_z", "diameter")


def tiles():
    """``(TILE, ITILE)``: the j-tile and the i-tile of the device's tile pass, in points (csrc/model_info.h)."""
    t, i = C.c_int(0), C.c_int(0)
    _lib.lib().suo_model_info_tiles(C.byref(t), C.byref(i))
    return t.value, i.value


def _points(p):
    if hasattr(p, "detach"):
        p = p.detach().cpu().numpy()
    return np.ascontiguousarray(p, np.float32).reshape(-1, 3)


def model_info_raw(lib, handle, index, pairs=False):
    """The C entry over a live database handle: ``(info float64 [n,7], pair int32 [n,2] or None, flags int32 [n])`` of the database's models ``index``."""
    idx = np.ascontiguousarray(index, np.int32).reshape(-1)
    n = idx.shape[0]
    info = np.zeros((n, 7), np.float64)
    pair = np.zeros((n, 2), np.int32) if pairs else None
    flags = np.zeros(n, np.int32)
    _lib.check(lib.suo_model_info(handle, n, idx.ctypes.data, info.ctypes.data, None if pair is None else pair.ctypes.data, flags.ctypes.data), "suo_model_info")
    return info, pair, flags


class PointDb:
    """A mesh database of bare point clouds (no symmetries, no faces) and the raw entry over it: ``clouds`` is a list of [P,3] arrays, model k is
    ``clouds[k]`` as float32.  What ``model_info`` uploads a dictionary into; a context manager."""

    def __init__(self, clouds):
        self.lib = _lib.lib()
        _lib.require_gpu()
        self.clouds = [_points(c) for c in clouds]
        n_pts = np.array([c.shape[0] for c in self.clouds], np.int32)
        allpts = np.ascontiguousarray(np.concatenate(self.clouds, 0))
        self.h = C.c_void_p()
        _lib.check(self.lib.suo_mesh_db_create(len(self.clouds), n_pts.ctypes.data, allpts.ctypes.data, C.byref(self.h)), "suo_mesh_db_create")

    def run(self, index, pairs=True):
        return model_info_raw(self.lib, self.h, index, pairs)

    def close(self):
        if self.h is not None:
            self.lib.suo_mesh_db_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def model_info(errors_or_db, obj_ids=None, pairs=False):
    """``{obj_id: {"min_x", "min_y", "min_z", "size_x", "size_y", "size_z", "diameter"}}`` (Python floats, the toolkit's keys) of the objects ``obj_ids``
    (default: all), in one device call.  ``errors_or_db``: a bop_eval.BopErrors or eval_meter.EvalMeter -- its mesh database is used as it stands (an
    EvalMeter built with ``sample_n_points`` holds the sampled points) -- or a mesh_db dictionary ``{obj_id: {"points": [P,3]}}``, whose points are uploaded
    for the call.  ``pairs``: also ``"pair"``, the point indices ``(i, j)``, i <= j, of the diametral pair with the lowest i, then the lowest j.  A model with
    a NaN or Inf coordinate has NaN in all seven (and the pair (-1, -1)); the others are unaffected."""
    if isinstance(errors_or_db, dict):
        want = list(errors_or_db.keys()) if obj_ids is None else list(obj_ids)
        if not want:
            return {}
        ids = list(dict.fromkeys(want))
        with PointDb([errors_or_db[o]["points"] for o in ids]) as db:
            info, pair, _ = db.run([ids.index(o) for o in want], pairs)
    else:
        assert errors_or_db._h is not None, "the mesh database is closed"
        want = list(errors_or_db._index.keys()) if obj_ids is None else list(obj_ids)
        if not want:
            return {}
        info, pair, _ = model_info_raw(errors_or_db.lib, errors_or_db._h, [errors_or_db._index[o] for o in want], pairs)
    out = {}
    for k, o in enumerate(want):
        e = {name: float(info[k, c]) for c, name in enumerate(KEYS)}
        if pairs:
            e["pair"] = (int(pair[k, 0]), int(pair[k, 1]))
        out[o] = e
    return out


def format_models_info(info):
    """The text ``inout.save_json(path, info)`` writes for a dictionary (inout.py:86-102): ``{``, one ``  "<id>": <json.dumps(v, sort_keys=True)>`` line per
    object in ascending order of the integer keys, ``}``, no trailing newline."""
    items = sorted(info.items(), key=lambda kv: kv[0])
    lines = ['  "{}": {}'.format(k, json.dumps(v, sort_keys=True)) + ("," if i != len(items) - 1 else "") for i, (k, v) in enumerate(items)]
    return "{\n" + "".join(ln + "\n" for ln in lines) + "}"


def model_ids(model_dir):
    """The ids of the ``obj_%06d.ply`` files of ``model_dir``, ascending."""
    return sorted(int(m.group(1)) for m in (re.fullmatch(r"obj_(\d{6})\.ply", f) for f in os.listdir(model_dir)) if m)


def calc_models_info(model_dir, obj_ids=None, keep=True, write=True):
    """``{obj_id: entry}`` for the models ``obj_%06d.ply`` of ``model_dir`` (``obj_ids``: which; default all there), as ``calc_model_info.py`` computes
    them; with ``write`` saved as ``models_info.json`` in the toolkit's text.  ``keep``: the stated deviation of the module doc -- what an existing
    models_info.json holds besides the seven computed keys stays."""
    return _calc_models_info(model_dir, obj_ids, keep, write, model_info)


def _calc_models_info(model_dir, obj_ids, keep, write, compute):
    """calc_models_info with what maps the mesh_db dictionary to the entries as an argument: ``model_info`` on the device, or, in the host tests of the
    file handling, their numpy restatement."""
    from . import bop
    ids = model_ids(model_dir) if obj_ids is None else [int(o) for o in obj_ids]
    db = {o: {"points": bop.load_ply_points(os.path.join(model_dir, f"obj_{o:06d}.ply")).astype(np.float32)} for o in ids}
    out = compute(db)
    path = os.path.join(model_dir, "models_info.json")
    if keep and os.path.exists(path):
        with open(path, "r") as f:
            old = {int(k): v for k, v in json.load(f).items()}
        for o, e in old.items():
            if o in out:
                out[o].update({k: v for k, v in e.items() if k not in KEYS})
            else:
                out[o] = e
    if write:
        with open(path, "w") as f:
            f.write(format_models_info(out))
    return out
