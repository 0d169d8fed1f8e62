"""Every case of tests/ba_route_cases.py on the GPU: its route asserted first (suo_debug_lm_routes), then each problem against the C oracle
(oracle/lm_oracle.c) at the gates of tests/test_gpu_geometry.py: _compare_ba.  In a batch, each problem is also run alone; where that is the same
route it must be bit-identical to its batch result (across different kernels only the oracle gates apply)."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import geometry as G  # noqa: E402
from tests import ba_route_cases as RC  # noqa: E402
from tests.test_gpu_geometry import _compare_ba  # noqa: E402

CHI2_THR = 5.991


@pytest.fixture(scope="module")
def ba():
    from suo_slam_amd import _lib, ba
    _lib.require_gpu()
    return ba


def _args(P):
    return [P[k] for k in RC.KEYS]


def _flag_report(P, got, kw):
    """The edges whose inlier flag differs from the oracle's, with both chi2 values, and every edge whose oracle chi2 lies within 1e-9 relative of the
    threshold (a flag there is decided by rounding, not by the kernel)."""
    ref = G.optimize(*_args(P), **kw)
    diff = np.flatnonzero(got[2] != ref[2])
    near = np.flatnonzero(np.abs(ref[3] - CHI2_THR) <= 1e-9 * CHI2_THR)
    return (f"flags differ at edges {diff[:20].tolist()} (kernel chi2 {got[3][diff[:20]].tolist()}, oracle chi2 {ref[3][diff[:20]].tolist()}); "
            f"edges within 1e-9 of the threshold: {[(int(e), float(ref[3][e])) for e in near]}")


def _check(ba_like, P, **kw):
    """_compare_ba (oracle gates, unchanged) on what ba_like.optimize returns; nothing may be NaN."""
    got = ba_like.optimize(*_args(P), **kw)
    fixed = types.SimpleNamespace(optimize=lambda *a, **k: got)
    try:
        _, ref = _compare_ba(fixed, P, **kw)
    except AssertionError as e:
        raise AssertionError(f"{e}\n{_flag_report(P, got, kw)}") from e
    for a in (got[0], got[1], got[3]):
        assert np.isfinite(a).all()
    return got, ref


def _kws(case):
    base = {} if case.its is None else {"its": case.its}
    return [dict(base, init_with_outliers=iwo) for iwo in ((False, True) if case.tracking else (False,))]


@pytest.mark.parametrize("name", RC.CASE_IDS)
def test_case_matches_the_oracle_on_its_route(ba, name):
    case = RC.BY_NAME[name]
    probs = case.problems()
    for kw in _kws(case):
        routes, _ = RC.routes_of(probs, **kw)
        assert routes == case.routes, (name, routes)
        if len(probs) == 1:
            got, ref = _check(ba, probs[0], **kw)
            results = [(got, ref)]
        else:
            batch = ba.optimize_batch([ba.Problem(*_args(P), **kw) for P in probs])
            results = []
            for P, p, route in zip(probs, batch, routes):
                out = (p.cam_T.reshape(-1, 3, 4), p.obj_T.reshape(-1, 3, 4), p.inlier, p.chi2, p.stats)
                results.append(_check(types.SimpleNamespace(optimize=lambda *a, _o=out, **k: _o), P, **kw))
                alone, _ = _check(ba, P, **kw)                          # alone: on the route it takes alone, against the oracle too
                if RC.routes_of([P], **kw)[0] == [route]:
                    for a, b in zip(out, alone):
                        assert np.array_equal(a, b), (name, route)
        for P, (got, ref) in zip(probs, results):
            assert got[4][0] >= 1 and ref[4][3] >= 4, (got[4], ref[4])             # the rounds ran: not a no-op comparison
            if name == "tracking_rejected_trials_cam":
                assert got[4][2] > got[4][1], got[4]                               # the kernel itself rejected trials: pop() and lambda * ni ran
            if name.startswith("degenerate_outlier_object"):
                # the object all of whose measurements are gross outliers keeps no inlier: its block is lambda I from round 1 on
                cut = [o for o in range(len(P["obj_T"])) if not ref[2][P["edge_obj"] == o].any()]
                assert len(cut) == 1, cut
            if name.startswith("degenerate_weak_camera"):
                c = len(P["cam_T"]) - 1
                assert (P["edge_cam"] == c).sum() <= 2 and not P["cam_fixed"][c]
