"""Graphs placed on the lane-group shapes of the phase kernels (csrc/lm_dist.hip), for tests/test_ba_phases_ref.py and tests/test_gpu_ba_phases.py.  All of them come
from tests/ba_route_cases.graph: anisotropic information with xy of both signs, outliers a few Huber deltas out as well as gross ones.

small    3 cameras (camera 0 fixed), 2 free objects, 6 edges per pair: every property runs on it.
slices   86 free cameras (0 .. 85) and one fixed (86, last, so that it ends the one list it is in); 10 free objects whose lists hold exactly 7, 8, 9, 31, 32, 33, 41, 42,
         43 and 85 FREE cameras (object j sees cameras 0 .. n_j - 1; the object of 85 cameras 1 .. 85 and the fixed one): 8 +- 1 for the eight lanes of ba_gather_kernel, 32 +- 1 for
         the 32 lanes per r_g row, 42 +- 1 and 2 * 42 + 1 for the 42 camera slices of ba_schur_s_kernel; 100 blocks of S over 64 workgroups; the cameras' own lists have
         10, 9, .., 1 objects (1, 3, 4, 5 and 8 among them: the four slices of ba_update_kernel at 4 +- 1 and at 8).  2 edges per pair.
slots    6 objects of which 1 and 4 are fixed (obj_slot is not the identity); cameras 0 and 1 fixed, camera 1 with edges to free objects (Hoo / bo, not S); one edge
         between fixed camera 0 and fixed object 1 (never active); free object 5 without an edge; free camera 5 all of whose measurements lie 150 px off, so that the
         classification casts every one of its edges out and Hcc = 0.
ns102    5 cameras, 17 free objects (ba_solve_big_kernel); ns96 is ns102 without its last object (16: the LDS solve of ba_solve_kernel), edge for edge.
weak     a small global graph plus a camera that sees one keypoint: Hcc of rank 2.
ranks    7 cameras, 2 objects, 6 edges per pair; dealt to three ranks by ba_dist.split_problem."""
from __future__ import annotations

import zlib

import numpy as np

from tests import ba_route_cases as RC

SLICE_LISTS = (7, 8, 9, 31, 32, 33, 41, 42, 43, 85)
NAMES = ("small", "slices", "slots", "ns96", "ns102", "weak", "ranks")
SLOTS_CAST_OUT_CAMERA, SLOTS_EDGELESS_OBJECT = 5, 5


def _rng(name):
    return np.random.default_rng(zlib.crc32(f"phases/{name}".encode()))


def _gauge(n_cam, fixed=(0,)):
    cf = np.zeros(n_cam, np.uint8)
    cf[list(fixed)] = 1
    return cf


def _small():
    return RC.graph(_rng("small"), np.full((3, 2), 6), _gauge(3), np.zeros(2), outlier_frac=0.25)


def _slices_counts():
    counts = np.zeros((87, 10), int)
    for j, n in enumerate(SLICE_LISTS):
        counts[:n, j] = 2
    counts[:, 9] = 0
    counts[1:87, 9] = 2                                # (cameras 1 .. 85 and the fixed one: every free camera sees something)
    return counts


def _slices():
    return RC.graph(_rng("slices"), _slices_counts(), _gauge(87, (86,)), np.zeros(10))


def _slots():
    counts = np.zeros((6, 6), int)
    counts[0, [0, 2]] = 4
    counts[0, 1] = 1                                   # fixed camera, fixed object
    counts[1, [0, 2, 3]] = 4                           # the second fixed camera sees free objects
    counts[2:5, :5] = 4                                # free cameras see fixed and free objects alike
    counts[5, [0, 3, 4]] = 4
    of = np.zeros(6, np.uint8)
    of[[1, 4]] = 1
    P = RC.graph(_rng("slots"), counts, _gauge(6, (0, 1)), of, outlier_frac=0.2)
    P["edge_uv"][P["edge_cam"] == SLOTS_CAST_OUT_CAMERA] += 150.0
    return P


def _ns102():
    return RC.graph(_rng("ns102"), np.full((5, 17), 3), _gauge(5), np.zeros(17))


def without_last_object(P):
    last = len(P["obj_T"]) - 1
    keep = P["edge_obj"] != last
    Q = {k: np.array(v) for k, v in P.items()}
    for k in ("edge_cam", "edge_obj", "edge_camk", "edge_p", "edge_uv", "edge_info", "edge_inlier"):
        Q[k] = np.ascontiguousarray(P[k][keep])
    for k in ("obj_T", "obj_fixed", "obj_gt"):
        Q[k] = np.ascontiguousarray(P[k][:last])
    return Q


def _weak():
    r = _rng("weak")
    return RC.with_weak_camera(r, RC.global_graph(r, 90, 4, 3, miss=0.0), 1)


def _ranks():
    return RC.graph(_rng("ranks"), np.full((7, 2), 6), _gauge(7), np.zeros(2), outlier_frac=0.25)


_BUILD = {"small": _small, "slices": _slices, "slots": _slots, "ns102": _ns102, "ns96": lambda: without_last_object(_ns102()), "weak": _weak, "ranks": _ranks}


def graph(name):
    """The case's arrays (tests/ba_route_cases.KEYS), rebuilt from its fixed seed."""
    return _BUILD[name]()


def problem(name, **kw):
    """A fresh ba.Problem of the case: contexts write into the one they are given."""
    from suo_slam_amd import ba
    P = graph(name)
    return ba.Problem(*[P[k] for k in RC.KEYS], **kw)


def weak_camera(P=None):
    return len((graph("weak") if P is None else P)["cam_T"]) - 1


# ---- the sizes the cases stand for, stated where a change of the builders would move them ---------------------------------------------------------------------
def _list_lengths(counts, cam_fixed):
    free = ~np.asarray(cam_fixed, bool)
    return [int(((counts[:, o] > 0) & free).sum()) for o in range(counts.shape[1])], [int((counts[c] > 0).sum()) for c in range(len(counts))]


_c = _slices_counts()
_per_obj, _per_cam = _list_lengths(_c, _gauge(87, (86,)))
assert tuple(_per_obj) == SLICE_LISTS == (8 - 1, 8, 8 + 1, 32 - 1, 32, 32 + 1, 42 - 1, 42, 42 + 1, 2 * 42 + 1)
assert {1, 3, 4, 5, 8} <= set(_per_cam[:86]) and min(_per_cam) >= 1
assert all(np.flatnonzero(_c[:, o] > 0).max() == (86 if o == 9 else SLICE_LISTS[o] - 1) for o in range(10))      # the fixed camera ends the one list it is in
assert len(SLICE_LISTS) ** 2 > 64 and int(_c.sum()) < 1000
del _c, _per_obj, _per_cam
