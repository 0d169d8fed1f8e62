"""Graphs for the tests of suo_residual_statistics (tests/test_gpu_resid_stats.py, tests/test_resid_stats_ref.py): the smallest graphs at which its kernels can go
wrong.  From tests/pose_cov_cases.py and tests/pose_cov_graph_cases.py: every cov_form (0: 1x1_4edges with 2 degrees of freedom and 1x17 with its second pass of 16
objects; 1: cam_only; 2: 3x2 and 5x16, the LDS form at its cap, with misses; 3: 3x17m and 6x20m, cameras that miss objects, edge counts that are no multiple of 256
and, in 6x20m, more than one workgroup of edges).  Designed variants, each a copy of a small case:
  three_edges     one object of a single-view frame cut to exactly three counted edges: no redundancy, t NaN, status[3] == 3 (DESIGNED names those edges)
  flagged_3x2     every fifth edge flagged edge_inlier = 0: the s = +1 branch next to counted edges of the same pairs
  object_out_*    an object all of whose edges are flagged out: a NaN vertex, its edges counted in status[2] (forms 0, 2 and 3)
  fixed_pair_3x2  a fixed object seen by the fixed camera: P = 0 and t == chi2 on those edges
  shuffled_3x2    the edges of 3x2 in a random order: the caller's order is not the pair order the kernels sort into
  no_edges        n_edge == 0
Every graph is cached with its references (tests/pose_cov_ref.py, tests/resid_stats_ref.py), computed once and never modified: tests take copies."""
import functools

import numpy as np

from tests import pose_cov_cases as K
from tests import pose_cov_graph_cases as GK
from tests import pose_cov_ref as R
from tests import resid_stats_ref as RS

EDGE_KEYS = ("edge_cam", "edge_obj", "edge_camk", "edge_p", "edge_uv", "edge_info", "edge_inlier")


def _three_edges():
    g = K.frame(67, 3, (8, 12))      # (a seed at which the three ill-held edges leave cond(H), and with it every tolerance, moderate)
    keep = np.ones(len(g["edge_obj"]), bool)
    keep[np.flatnonzero(g["edge_obj"] == 1)[3:]] = False        # (removed, not flagged out: beside three counted edges an uncounted one is all but undetermined)
    for k in EDGE_KEYS:
        g[k] = g[k][keep]
    return g


def _flagged(g, step=5):
    g["edge_inlier"][2::step] = 0
    return g


def _object_out(g, o):
    g["edge_inlier"][g["edge_obj"] == o] = 0
    return g


def _fixed_pair():
    g = K.CASES["3x2"]()
    g["obj_fixed"][1] = 1
    return g


def _shuffled():
    g = K.CASES["3x2"]()
    order = np.random.default_rng(62).permutation(len(g["edge_cam"]))
    for k in EDGE_KEYS:
        g[k] = g[k][order]
    g["edge_inlier"][::7] = 0
    return g


def _no_edges():
    g = K.frame(63, 2)
    for k in EDGE_KEYS:
        g[k] = g[k][:0]
    return g


CASES = {
    "1x1_4edges": K.CASES["1x1_4edges"],
    "1x17": K.CASES["1x17"],
    "cam_only": K.CASES["cam_only"],
    "3x2": K.CASES["3x2"],
    "5x16": K.CASES["5x16"],
    "3x17m": GK.CASES["3x17m"],
    "6x20m": GK.CASES["6x20m"],
    "three_edges": _three_edges,
    "flagged_3x2": lambda: _flagged(K.CASES["3x2"]()),
    "object_out_frame": lambda: _object_out(K.frame(64, 3), 2),
    "object_out_3x2": lambda: _object_out(K.CASES["3x2"](), 1),
    "object_out_3x17m": lambda: _object_out(GK.CASES["3x17m"](), 16),
    "fixed_pair_3x2": _fixed_pair,
    "shuffled_3x2": _shuffled,
    "no_edges": _no_edges,
}
NAMES = list(CASES)


def designed(name, g):
    """the edges whose reference det R must sit far BELOW the rule's threshold: the three counted edges of the cut object"""
    if name != "three_edges":
        return np.zeros(len(g["edge_cam"]), bool)
    return (g["edge_obj"] == 1) & (g["edge_inlier"] == 1)


FAR = 1e3           # every input sits this factor away from the rule's threshold, on its side


def far_from_the_threshold(name, g, st):
    """the condition on the inputs (asserted by tests/test_resid_stats_ref.py and again by the GPU test): every counted edge outside the designed three-edge object has reference det R at least
    FAR x the threshold, the designed edges at most threshold / FAR; uncounted edges have det R = det(I + P Omega) >= 1"""
    cut = designed(name, g)
    ok = ~np.isnan(st["det"])
    assert (st["det"][ok & st["counted"] & ~cut] >= FAR * RS.MIN_DET).all(), (name, st["det"][ok & st["counted"] & ~cut].min())
    assert (st["det"][ok & ~st["counted"]] >= 1.0 - 1e-9).all(), name
    assert (np.abs(st["det"][cut]) <= RS.MIN_DET / FAR).all(), (name, st["det"][cut])
    return int(cut.sum())


@functools.lru_cache(maxsize=None)
def _case(name):
    g = CASES[name]()
    ref = R.covariances(g)
    return g, ref, RS.statistics(g, ref)


def case(name):
    """(graph, reference of pose_cov_ref, reference of resid_stats_ref): the graph a deep copy, the references shared and read-only"""
    g, ref, stats = _case(name)
    return {k: v.copy() for k, v in g.items()}, ref, stats
