"""Graphs and pair lists for the pair-covariance tests (tests/test_gpu_pose_cov_pairs.py, tests/test_pose_cov_pairs_ref.py), built with pose_cov_cases._graph, the
same metre-scale generator.  The fixed camera of pose_cov_cases' frames sits at the identity, where Ad(T_c) = I would leave the propagation untested, so the
frames here hold their fixed camera at MOVED, a pose away from the identity, with 8, 9 and 17 objects (8 lanes per object, 4 lanes per object, two passes); the
curr-only graph holds its free camera there.  "3x2" and "5x16" are pose_cov_cases' graphs (their references are shared).  Every graph is cached with its two
references, computed once and never modified: tests take copies."""
import functools

import numpy as np

from tests import pose_cov_cases as K
from tests import pose_cov_pairs_ref as PR
from tests import pose_cov_ref as R

# world -> camera: 0.3 rad about y, 0.1 rad about x, the camera 10-20 cm off the origin; the objects (0.5-1.5 m down the world's z) stay in front of it
MOVED = R.exp_se3(np.array([0.1, 0.3, -0.05, 0.12, -0.06, 0.2]))


def moved_frame(seed, n_obj):
    rng = np.random.default_rng(seed)
    return K._graph(rng, [MOVED], [1], n_obj, lambda c, o: True)


def moved_cam_only(seed):
    rng = np.random.default_rng(seed)
    return K._graph(rng, [MOVED], [0], 2, lambda c, o: True, (4, 4), obj_fixed=[1, 1])


CASES = {
    "moved_1x8": lambda: moved_frame(31, 8),
    "moved_1x9": lambda: moved_frame(32, 9),
    "moved_1x17": lambda: moved_frame(33, 17),
    "moved_cam_only": lambda: moved_cam_only(34),
    "3x2": lambda: K.case("3x2")[0],
    "5x16": lambda: K.case("5x16")[0],          # seed 12, miss = 0.3: UNSEEN below asserts that a free camera misses an object
}
OBJ_PAIRS = {"moved_1x17": [(0, 1), (3, 16)], "5x16": [(0, 1), (0, 15)]}      # (3, 16) straddles the two passes of 16 objects


def pairs_of(g, obj_pairs=((0, 1),)):
    """every (camera, object) pair, then the (object, object) pairs, as vertex codes [P,2]"""
    C, O = len(g["cam_T"]), len(g["obj_T"])
    return np.array([(c, C + o) for c in range(C) for o in range(O)] + [(C + a, C + b) for a, b in obj_pairs], np.int32)


def unseen_pair(g):
    """the first (free camera, object) pair without an edge between the two, as (camera, object), or None"""
    seen = set(zip(g["edge_cam"].tolist(), g["edge_obj"].tolist()))
    for c in range(len(g["cam_T"])):
        for o in range(len(g["obj_T"])):
            if not g["cam_fixed"][c] and (c, o) not in seen:
                return c, o
    return None


def with_refs(g, pairs):
    ref = R.covariances(g)
    return ref, PR.relative(g, ref, pairs)


@functools.lru_cache(maxsize=None)
def _case(name):
    g = CASES[name]()
    pairs = pairs_of(g, OBJ_PAIRS.get(name, [(0, 1)]))
    return (g, pairs) + with_refs(g, pairs)


def case(name):
    """(graph, pairs [P,2], reference of pose_cov_ref, (cross, rel, NaN pairs) of pose_cov_pairs_ref): the graph a deep copy, the rest shared and read-only"""
    g, pairs, ref, rel = _case(name)
    return {k: v.copy() for k, v in g.items()}, pairs.copy(), ref, rel


UNSEEN = unseen_pair(K.case("5x16")[0])
assert UNSEEN is not None, "5x16: every free camera sees every object -- pick a seed with a missing (camera, object) edge"
