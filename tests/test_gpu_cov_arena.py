"""The covariance entries share one arena (csrc/cov_stage.hip stages all of them through the arena of suo_optimize_batch): an entry must not read what an earlier
entry left there, nor rely on memory that happened to be zero.  Each of the five batch entries is called on its smallest cases, the arena is then grown and
dirtied by a larger graph call and an LM run, and the entries are called again in reverse order: every output keeps its bytes (tobytes(), so NaN positions count),
and the Problem arrays handed to the entries are unchanged.

The graphs: pose_cov_cases "3x2" and "1x17", pose_cov_pair_cases "moved_cam_only", the smallest of track_cov_cases.SIZES, resid_stats_cases "three_edges" and
"no_edges".  The dirtying call is pose_covariances_graph_batch on "1x33" -- the graph of that name is pose_cov_cases', pose_cov_graph_cases has none; its pairs
are pose_cov_graph_cases.pairs_of -- together with pose_cov_graph_cases "2x32", so that the device-memory form's scratch is written too, then optimize_batch on
a copy of "3x2"."""
import numpy as np
import pytest

from suo_slam_amd import ba
from tests import pose_cov_cases as K
from tests import pose_cov_graph_cases as GK
from tests import pose_cov_pair_cases as PK
from tests import resid_stats_cases as RK
from tests import track_cov_cases as TC

pytestmark = pytest.mark.gpu

PROBLEM_ARRAYS = ("cam_T", "obj_T", "cam_fixed", "obj_fixed", "edge_cam", "edge_obj", "edge_camk", "edge_p", "edge_uv", "edge_info", "inlier")


def _problem(g):
    return ba.Problem(*K.args(g))


def _flat(results):
    """every array of a batch entry's return value, in a fixed order"""
    out = []
    for r in results:
        out += [r[k] for k in sorted(r)] if isinstance(r, dict) else list(r)
    return out


@pytest.fixture(scope="module")
def entries():
    """name -> (call, problems): the five batch entries on their smallest cases, the problems built once"""
    small = [_problem(K.CASES[n]()) for n in ("3x2", "1x17")]
    small_lists = [PK.pairs_of(K.CASES[n]()) for n in ("3x2", "1x17")]
    g_pair = PK.CASES["moved_cam_only"]()
    pair, pair_lists = [_problem(g_pair)] + small, [PK.pairs_of(g_pair)] + small_lists
    g_track, Sigma, _ = TC.case(min(TC.SIZES))
    track = [_problem(g_track)]
    resid = [_problem(RK.CASES[n]()) for n in ("three_edges", "no_edges")]
    return {
        "pose_covariances_batch": (lambda: ba.pose_covariances_batch(small), small),
        "pose_covariances_pairs_batch": (lambda: ba.pose_covariances_pairs_batch(pair, pair_lists), pair),
        "pose_covariances_graph_batch": (lambda: ba.pose_covariances_graph_batch(pair, pair_lists), pair),
        "tracking_covariances_batch": (lambda: ba.tracking_covariances_batch(track, [Sigma]), track),
        "residual_statistics_batch": (lambda: ba.residual_statistics_batch(resid), resid),
    }


def test_every_entry_keeps_its_bytes_after_the_arena_was_grown_and_dirtied(entries):
    first = {name: [a.tobytes() for a in _flat(call())] for name, (call, _) in entries.items()}
    assert all(first.values())

    big = [K.CASES["1x33"](), GK.CASES["2x32"]()]
    got = ba.pose_covariances_graph_batch([_problem(g) for g in big], [GK.pairs_of(g) for g in big])
    assert not np.isnan(got[1][0]).any() and not np.isnan(got[1][1]).any(), "2x32: every vertex carries edges"
    ba.optimize_batch([_problem(K.CASES["3x2"]())])

    for name in reversed(list(entries)):
        again = [a.tobytes() for a in _flat(entries[name][0]())]
        assert len(again) == len(first[name]), name
        for j, (x, y) in enumerate(zip(first[name], again)):
            assert x == y, (name, "output", j, "changed its bytes after the arena was grown and dirtied")


def test_the_entries_leave_their_problems_as_they_were(entries):
    for name, (call, probs) in entries.items():
        before = [{k: getattr(p, k).copy() for k in PROBLEM_ARRAYS} for p in probs]
        call()
        for p, b in zip(probs, before):
            for k in PROBLEM_ARRAYS:
                assert getattr(p, k).dtype == b[k].dtype and getattr(p, k).tobytes() == b[k].tobytes(), (name, k, "the entry modified its Problem")
