"""The rule of suo_model_info (include/suo_hip.h, row N8) in chunked numpy fp64, pair rule included: the yardstick of tests/test_gpu_model_info.py at the
sizes the toolkit was not run on.  tests/test_model_info_ref.py ties it to the toolkit's own functions (tests/golden/model_info_golden.npz) with ``==``.

    box       min_c = min_i p_ic,  size_c = max_i p_ic - min_c; a zero minimum with both zeros present is -0.0 (-0 orders below +0; numpy's own min
              reports whichever zero it meets first: the one case in which the rule is not the toolkit's).  The sign of a zero maximum never shows:
              max - min is the same number with either zero
    diameter  sqrt(max_{i <= j} ((dx dx + dy dy) + dz dz)) on the float32 points widened to fp64
    pair      the i <= j with that maximum, lowest i, then lowest j

numpy forms each product and sum as one correctly rounded fp64 operation, in the order written: no contraction."""
import math

import numpy as np

ROWS = 128                # i-points of one chunk: 128 x n doubles per temporary
KEYS = ("min_x", "min_y", "min_z", "size_x", "size_y", "size_z", "diameter")


def _d2(p, i0, i1):
    """d^2 of the points i0..i1-1 against the points i0..n-1 (the columns j < i they also hold equal their mirror images exactly)."""
    a, b = p[i0:i1], p[i0:]
    dx = a[:, 0:1] - b[None, :, 0]
    dy = a[:, 1:2] - b[None, :, 1]
    dz = a[:, 2:3] - b[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def model_info(pts32, pair=False):
    """``(info float64 [7], (i, j) or None, flag)`` of one float32 cloud [n,3]; a non-finite coordinate: seven NaN, (-1, -1), flag 1."""
    pts32 = np.asarray(pts32)
    assert pts32.dtype == np.float32 and pts32.ndim == 2 and pts32.shape[1] == 3 and len(pts32) > 0
    if not np.isfinite(pts32).all():
        return np.full(7, np.nan), ((-1, -1) if pair else None), 1
    p = pts32.astype(np.float64)
    n = len(p)
    lo, hi = p.min(axis=0), p.max(axis=0)
    for c in range(3):                                            # -0 orders below +0
        if lo[c] == 0.0:
            lo[c] = -0.0 if np.signbit(p[p[:, c] == 0.0, c]).any() else 0.0
    tops = [float(_d2(p, i0, min(i0 + ROWS, n)).max()) for i0 in range(0, n, ROWS)]
    top = max(tops)
    found = None
    if pair:
        for c, i0 in enumerate(range(0, n, ROWS)):
            if tops[c] != top:
                continue
            d = _d2(p, i0, min(i0 + ROWS, n))
            hit = (d == top) & (np.arange(d.shape[1])[None, :] >= np.arange(d.shape[0])[:, None])         # j >= i
            rows = hit.any(axis=1)
            if rows.any():
                r = int(np.argmax(rows))
                found = (i0 + r, i0 + int(np.argmax(hit[r])))
                break
        assert found is not None
    return np.array([lo[0], lo[1], lo[2], hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2], math.sqrt(top)], np.float64), found, 0


def entry(pts32):
    """The models_info.json entry of one cloud: Python floats under the toolkit's keys."""
    info, _, _ = model_info(pts32)
    return {k: float(v) for k, v in zip(KEYS, info)}


def models_info(db):
    """``{obj_id: entry}`` of a mesh_db dictionary: what bop_model_info.model_info computes on the device."""
    return {o: entry(np.ascontiguousarray(e["points"], np.float32)) for o, e in db.items()}
