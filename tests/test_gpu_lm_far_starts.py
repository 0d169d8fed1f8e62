"""Every LM route from far starts (tests/lm_far_cases.py): updates of 0.03-0.8 rad go through pose_oplus' Taylor series and closed forms and R_to_q's other forms
inside the LM kernels themselves, where the route table's near starts (< 1e-3 rad) reach the shortcut only.

a. ONE and TWO LM iterations against the C oracle at the unchanged gates of tests/test_gpu_geometry.py: _compare_ba, on cases the oracle alone admitted (distance of
   every chi2 from the threshold, stability under edge reordering, where the first step lands) -- checked here before the kernel's result is looked at.
b. The truth of noise-free graphs recovered from 0.1 / 0.3 rad out in 40 iterations: judged by the ground truth at the project's gates, not by the oracle (which
   only has to get there itself for the case to count).  Iteration and trial counts are not compared.

Measured (oracle's first-step angles in rad, low | high level): FRAME2 0.04-0.16 | 0.22-0.63, FRAME8 0.06-0.16 | 0.17-0.38, FRAME16 0.03-0.14 | 0.23-0.69,
CAM2 0.10 | 0.63, CAM 0.13 | 0.54, LM 0.03-0.11 | 0.15-0.54, LM_BIG 0.05-0.14 | 0.13-0.82, PHASES 0.04-0.12 | 0.06-0.63, PHASEWISE 0.03-0.21 | 0.11-1.11; smallest
chi2 margin 2.8e-4, reordering at most 6.4e-12 (poses) / 4.8e-12 (chi2).  On an MI355X the kernels' poses lie within 1.4e-11 of the oracle's after one and two
iterations on all 36 cases (8.7e-10 on the rejected-trial cases).  Recovery, kernel's distance from the truth (dR / dt relative): FRAME2 1.1e-15 / 2.2e-16 and
1.4e-15 / 4.1e-16, CAM2 4.1e-16 / 4.3e-16 and 5.2e-16 / 5.8e-16, LM 7.5e-16 / 2.1e-14 and 8.3e-16 / 2.7e-14, PHASES 1.2e-15 / 1.1e-14 and 8.7e-16 / 7.4e-15 (from
0.1 and 0.3 rad; 16-28 iterations)."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import ba_route_cases as RC  # noqa: E402
from tests import lm_far_cases as F  # noqa: E402
from tests.test_gpu_geometry import _compare_ba, _pose_close  # noqa: E402


@pytest.fixture(scope="module")
def ba():
    from suo_slam_amd import _lib, ba
    _lib.require_gpu()
    return ba


def _run(ba, probs, kw):
    """Each problem's (cam_T, obj_T, inlier, chi2, stats): alone through optimize, several as ONE batch."""
    if len(probs) == 1:
        return [ba.optimize(*F.args(probs[0]), **kw)]
    batch = ba.optimize_batch([ba.Problem(*F.args(P), **kw) for P in probs])
    return [(p.cam_T.reshape(-1, 3, 4), p.obj_T.reshape(-1, 3, 4), p.inlier, p.chi2, p.stats) for p in batch]


def _against_oracle(ba, probs, route, its, level, need_single_trial=True):
    kw = dict(its=its, init_with_outliers=True)
    routes, _ = RC.routes_of(probs, **kw)
    assert routes == [route] * len(probs), routes
    for P in probs:                                                   # admitted by the oracle alone, before any kernel result exists
        ok, why, _ = F.admit(P, its, level, need_single_trial)
        assert ok, why
    for P, got in zip(probs, _run(ba, probs, kw)):
        for a in (got[0], got[1], got[3]):
            assert np.isfinite(a).all()
        assert got[4][0] >= 1 and got[4][1] >= 1, got[4]              # a round ran and iterated: not two no-ops compared
        _, ref = _compare_ba(types.SimpleNamespace(optimize=lambda *a, _g=got, **k: _g), P, **kw)
        moved = F.first_step_angles(P, got)
        print(f"{route} {level} its {its}: kernel stats {np.asarray(got[4]).tolist()}, oracle {ref[4].tolist()}, turned {moved.min():.3f} .. {moved.max():.3f} rad, "
              f"max pose diff {max(np.abs(got[0] - ref[0]).max(), np.abs(got[1] - ref[1]).max()):.2e}")
    return got, ref


@pytest.mark.parametrize("its", F.ITS, ids=lambda i: f"its{i[0]}")
@pytest.mark.parametrize("level", list(F.LEVELS))
@pytest.mark.parametrize("route", F.ROUTES)
def test_one_and_two_iterations_match_the_oracle(ba, route, level, its):
    _against_oracle(ba, F.build(route, level), route, its, level)


@pytest.mark.parametrize("family", list(F.REJECT))
def test_rejected_trial_after_a_large_step_matches_the_oracle(ba, family):
    _, its = F.REJECT[family]
    probs = F.build_reject(family)
    route = RC.routes_of(probs, its=its, init_with_outliers=True)[0][0]
    got, ref = _against_oracle(ba, probs, route, its, "high", need_single_trial=False)
    assert ref[4][2] > ref[4][1], ref[4]                              # the oracle rejected a trial on the way (the kernel's counts are not compared)


@pytest.mark.parametrize("rot", F.RECOVERY_ROT)
@pytest.mark.parametrize("route", list(F.RECOVERY_BUILDERS))
def test_truth_is_recovered_from_a_far_start(ba, route, rot):
    P = F.build_recovery(route, rot)
    assert RC.routes_of([P], **F.RECOVERY_KW)[0] == [route]
    ok, why, _ = F.admit_recovery(P)
    assert ok, why
    got = ba.optimize(*F.args(P), **F.RECOVERY_KW)
    dR, dt = F.truth_distance(P, got)
    print(f"{route} from {rot} rad: kernel ends dR {dR:.2e}  dt {dt:.2e} from the truth, stats {np.asarray(got[4]).tolist()}; {why}")
    for a, b in zip(np.r_[got[0], got[1]], np.r_[P["cam_gt"], P["obj_gt"]]):
        assert _pose_close(a, b, 1e-6, 1e-6), np.abs(a - b).max()
    assert got[2].all(), np.flatnonzero(got[2] == 0)
