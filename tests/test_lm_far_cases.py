"""The far-start cases of tests/lm_far_cases.py admitted by the oracle alone, on the CPU: every route has an admitted case at both levels and both iteration counts, on
the route it is meant for; the rejected-trial cases and the recovery cases likewise.  tests/test_gpu_lm_far_starts.py runs the kernels on exactly these."""
import numpy as np
import pytest

from tests import ba_route_cases as RC
from tests import lm_far_cases as F


@pytest.fixture(scope="module")
def built():
    from suo_slam_amd import build
    return build.build(verbose=False)


def test_existing_cases_rebuild_the_same_arrays():
    """perturb= defaults are the values the builders had: the rng is consumed identically."""
    r = lambda: np.random.default_rng(3)                                             # noqa: E731
    for a, b in ((RC.frame(r(), [5, 6]), RC.frame(r(), [5, 6], perturb=(3e-4, 0.2))), (RC.tracking(r(), [5, 6], 1), RC.tracking(r(), [5, 6], 1, perturb=(2e-4, 0.1))),
                 (RC.global_graph(r(), 40, 3, 2), RC.global_graph(r(), 40, 3, 2, perturb=(5e-4, 0.3)))):
        for k in RC.KEYS:
            assert np.array_equal(a[k], b[k]), k
    near, far = RC.frame(r(), [5, 6]), RC.frame(r(), [5, 6], perturb=(0.3, 30.0))
    for k in RC.KEYS:
        assert np.array_equal(near[k], far[k]) == (k != "obj_T"), k                  # only the start of the free vertices moves


@pytest.mark.parametrize("level", list(F.LEVELS))
@pytest.mark.parametrize("route", F.ROUTES)
def test_route_case_is_admitted(built, route, level):
    probs = F.build(route, level)
    assert max(len(P["edge_cam"]) for P in probs) <= 529
    for its in F.ITS:
        routes, _ = RC.routes_of(probs, its=its, init_with_outliers=True)
        assert routes == [route] * len(probs), (route, routes)
        for P in probs:
            ok, why, info = F.admit(P, its, level)
            assert ok, (route, level, its, why)
            if its == (1,):
                a = info["angles"]
                print(f"{route:9s} {level:4s} first-step angles: min {a.min():.3f}  median {np.median(a):.3f}  max {a.max():.3f}  ({len(a)} free vertices); "
                      f"chi2 margin {info['margin']:.1e}, reorder {info['reorder'][0]:.1e} / {info['reorder'][1]:.1e}")


@pytest.mark.parametrize("family", list(F.REJECT))
def test_rejected_trial_case_is_admitted(built, family):
    from oracle import geometry as G
    seed, its = F.REJECT[family]
    probs = F.build_reject(family)
    ref = G.optimize(*F.args(probs[0]), its=its, init_with_outliers=True)
    assert ref[4][2] > ref[4][1], ref[4]                                            # the oracle rejected a trial
    ok, why, info = F.admit(probs[0], its, "high", need_single_trial=False)
    assert ok, why
    print(f"{family}: its {its}, oracle stats {ref[4].tolist()}, accepted first-step angles {np.round(info['angles'], 3).tolist()}, route "
          f"{RC.routes_of(probs, its=its, init_with_outliers=True)[0]}")


@pytest.mark.parametrize("rot", F.RECOVERY_ROT)
@pytest.mark.parametrize("route", list(F.RECOVERY_BUILDERS))
def test_recovery_case_is_admitted(built, route, rot):
    P = F.build_recovery(route, rot)
    assert RC.routes_of([P], **F.RECOVERY_KW)[0] == [route]
    start = F.turn_angles(np.r_[P["cam_T"], P["obj_T"]], np.r_[P["cam_gt"], P["obj_gt"]])
    assert start.max() > 0.5 * rot
    ok, why, ref = F.admit_recovery(P)
    print(f"{route} from {rot} rad (largest start angle {start.max():.3f}): {why}")
    assert ok, why
