"""Graphs for the tests of suo_pose_covariances_graph (tests/test_gpu_pose_cov_graph.py, tests/test_pose_cov_graph_ref.py), from pose_cov_cases.coupled, the same
metre-scale generator.  They are the smallest sizes at which the device-memory form can go wrong: the first object past the 16 of the LDS form, reduced systems that
are no multiple of 64, 32 or 16 rows (102, 174), cameras that miss objects, and the largest system (n = 198) the constant of pose_cov_ref.bound covers.  Every graph
is cached with its reference, computed once and never modified: tests take copies."""
import functools

import numpy as np

from tests import pose_cov_cases as K
from tests import pose_cov_ref as R

CASES = {
    "2x17": lambda: K.case("2x17")[0],                       # the graph the old entries refuse
    "3x17m": lambda: K.coupled(21, 3, 17, miss=0.3, kp=(5, 7)),
    "6x20m": lambda: K.coupled(23, 6, 20, miss=0.3, kp=(5, 7)),
    "4x29m": lambda: K.coupled(24, 4, 29, miss=0.3, kp=(4, 6)),
    "2x32": lambda: K.coupled(22, 2, 32, kp=(4, 6)),
}
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def _case(name):
    g = CASES[name]()
    return g, R.covariances(g)


def case(name):
    """(graph, reference of pose_cov_ref): the graph a deep copy, the reference shared and read-only"""
    g, ref = _case(name)
    return {k: v.copy() for k, v in g.items()}, ref


def unseen_pair(g):
    """the first (free camera, object) pair without an edge between the two, as (camera, object), or None (pose_cov_pair_cases.unseen_pair's search)"""
    seen = set(zip(g["edge_cam"].tolist(), g["edge_obj"].tolist()))
    for c in range(len(g["cam_T"])):
        for o in range(len(g["obj_T"])):
            if not g["cam_fixed"][c] and (c, o) not in seen:
                return c, o
    return None


def camera_pairs(g):
    """every ordered (camera, camera) pair, the gauge included, and every (c, c)"""
    C = len(g["cam_T"])
    return [(a, b) for a in range(C) for b in range(C)]


def pairs_of(g):
    """The pair set of the large-map tests, as vertex codes [P,2]: every (camera, object) pair; a free camera with an object it does not see, named object first (where
    the graph has one); the object pairs (0, 1), (15, 16) -- straddling the old limit -- and (0, last) in both orders; every ordered (camera, camera) pair and (c, c)."""
    C, O = len(g["cam_T"]), len(g["obj_T"])
    pairs = [(c, C + o) for c in range(C) for o in range(O)]
    un = unseen_pair(g)
    if un is not None:
        pairs.append((C + un[1], un[0]))
    for a, b in ((0, 1), (15, 16), (0, O - 1)):
        pairs += [(C + a, C + b), (C + b, C + a)]
    return np.array(pairs + camera_pairs(g), np.int32)
