"""suo_pose_errors_points (csrc/eval_points.hip, row N4) on the device, through BopErrors.point_errors: the toolkit's pose_error.add / adi / proj.

Yardstick: the 40-digit mpmath evaluation of the same definitions (tests/points_errors_ref.mp_errors), computed once per module; next to it the toolkit's
own float64 values on the same pairs (tests/golden/siso_golden.npz, recorded by tests/golden/make_siso_golden.py).
Error scale per pair: s = the largest |coordinate| over both transformed point sets (add, adi); the largest |projected coordinate| (proj), the cases
keeping z >= 0.3 |X| (tests/test_siso_host.py asserts it).
Tolerance: C 2^-52 s with C = 8 x the largest ratio the TOOLKIT's float64 result shows against mpmath over these cases -- measured on the CPU by
tests/test_siso_host.py, which holds it: add 0.105 -> C = 0.88, adi 0.0487 -> C = 0.40, proj 0.773 -> C = 6.4 (points_errors_ref.TOOLKIT_RATIO rounds the
ratios up to 0.11, 0.05, 0.8).  The factor 8 is the margin for the different summation order of a P-term mean.  Against the toolkit's recorded value the bound is
(C + TOOLKIT_RATIO) 2^-52 s, the two distances to the mp value added.
The device showed (largest ratio to mp over the cases): add 0.105, adi 0.0333, proj 0.739 (DEVICE_RATIO below).
Point counts: P = 1, 63, 64, 65, 1023, 1025, 3001 -- either side of a wave (64), of a workgroup's 1024 ground-truth points and of the 512-point LDS tile, and
a model of several tiles whose estimated-pose points are split over 1, 2, 3 and 6 workgroups depending on the batch."""
import os

import numpy as np
import pytest

from suo_slam_amd import bop_eval
from tests import points_errors_ref as PR
from tests.golden import siso_cases as SC

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "siso_golden.npz"))
NAMES = ("add", "adi", "proj")
DEVICE_RATIO = {"add": 0.105, "adi": 0.0333, "proj": 0.739}     # the largest ratios an MI355X showed (test_against_mp_and_the_toolkit prints them); a record


@pytest.fixture(scope="module")
def be():
    pm = SC.point_models()
    e = bop_eval.BopErrors({m + 1: {"points": p} for m, p in enumerate(pm)}, {m + 1: {"diameter": 1.0} for m in range(len(pm))})
    yield e
    e.close()


@pytest.fixture(scope="module")
def pairs():
    pp = SC.point_pairs()
    return [m + 1 for m, *_ in pp], np.stack([p[1] for p in pp]), np.stack([p[2] for p in pp]), np.stack([p[3] for p in pp])


@pytest.fixture(scope="module")
def batch(be, pairs):
    return be.point_errors(*pairs)


@pytest.fixture(scope="module")
def mp_ref():
    pm = SC.point_models()
    return [PR.mp_errors(pm[m], Te, Tg, K) for m, Te, Tg, K in SC.point_pairs()]


def test_against_mp_and_the_toolkit(batch, mp_ref):
    worst = {k: 0.0 for k in NAMES}
    for i, (mpv, scale) in enumerate(mp_ref):
        for c, k in enumerate(NAMES):
            r = PR.ratio(batch[k][i], mpv[k], scale[k])
            worst[k] = max(worst[k], r)
            print(f"pair {i:2d} P {SC.POINT_COUNTS[i // SC.PAIRS_PER_MODEL]:5d} {k:4s} device {batch[k][i]!r} toolkit {GOLD['points'][i, c]!r} ratio to mp {r:.4f} (C {PR.C[k]:.2f})")
    print("largest |device - mp| / (2^-52 s):", worst)
    for i, (mpv, scale) in enumerate(mp_ref):
        for c, k in enumerate(NAMES):
            assert PR.ratio(batch[k][i], mpv[k], scale[k]) <= PR.C[k], (i, k)
            assert abs(batch[k][i] - GOLD["points"][i, c]) <= (PR.C[k] + PR.TOOLKIT_RATIO[k]) * PR.EPS * scale[k], (i, k)


def test_a_pair_has_the_same_bits_alone_and_in_any_batch(be, pairs, batch):
    objs, Te, Tg, K = pairs
    n = len(objs)
    for i in range(n):
        one = be.point_errors(objs[i:i + 1], Te[i:i + 1], Tg[i:i + 1], K[i:i + 1])
        for k in NAMES:
            assert one[k].view(np.uint64)[0] == batch[k].view(np.uint64)[i], (i, k)
    rev = be.point_errors(objs[::-1], Te[::-1], Tg[::-1], K[::-1])
    for k in NAMES:
        assert np.array_equal(rev[k][::-1].view(np.uint64), batch[k].view(np.uint64)), k


@pytest.mark.parametrize("copies", (300, 400, 700))
def test_the_split_of_the_estimated_points_does_not_show(be, pairs, batch, copies):
    """The 3001-point model alone has its estimated-pose points split over 6 workgroups per ground-truth tile (2048 workgroups wanted, 3 tiles); in a
    batch of 300 over 3, of 400 over 2, of 700 not at all.  The merged minima are the same."""
    objs, Te, Tg, K = pairs
    i = len(objs) - SC.PAIRS_PER_MODEL + 1                                     # the large perturbation of the largest model
    assert SC.POINT_COUNTS[-1] == 3001 and objs[i] == len(SC.POINT_COUNTS)
    many = be.point_errors([objs[i]] * copies, np.repeat(Te[i:i + 1], copies, 0), np.repeat(Tg[i:i + 1], copies, 0), K[i], which=("adi",))["adi"]
    assert np.all(many.view(np.uint64) == batch["adi"].view(np.uint64)[i])


def test_which_selects_and_does_not_change_the_bits(be, pairs, batch):
    objs, Te, Tg, K = pairs
    for which in (("add",), ("adi",), ("proj",), ("proj", "add")):
        out = be.point_errors(objs, Te, Tg, K, which=which)
        assert tuple(out) == which
        for k in which:
            assert np.array_equal(out[k].view(np.uint64), batch[k].view(np.uint64)), which
    assert np.array_equal(be.point_errors(objs, Te, Tg, which=("add", "adi"))["adi"].view(np.uint64), batch["adi"].view(np.uint64))      # no K without proj
    with pytest.raises(ValueError, match="needs the camera matrix"):
        be.point_errors(objs, Te, Tg, which=("proj",))
    with pytest.raises(ValueError, match="unknown error"):
        be.point_errors(objs, Te, Tg, K, which=("mssd",))
    empty = be.point_errors([], np.zeros((0, 3, 4)), np.zeros((0, 3, 4)), K[0])
    assert tuple(empty) == NAMES and all(v.shape == (0,) for v in empty.values())


def test_est_equal_to_gt_is_exactly_zero(pairs, batch):
    objs, Te, Tg, K = pairs
    same = [i for i in range(len(objs)) if np.array_equal(Te[i], Tg[i])]
    assert len(same) == len(SC.POINT_COUNTS)
    for k in NAMES:
        assert np.all(batch[k][same] == 0.0) and not np.any(np.signbit(batch[k][same])), k


def test_non_finite_distances_give_inf_and_a_clean_return(be, pairs, batch):
    objs, Te, Tg, K = pairs
    Tn = Te.copy()
    Tn[4, 1, 2] = np.nan                                                       # a NaN pose in the middle of the batch
    Tn[10, 0, 3] = np.inf
    out = be.point_errors(objs, Tn, Tg, K)
    for k in NAMES:
        assert out[k][4] == np.inf and out[k][10] == np.inf, k
        keep = [i for i in range(len(objs)) if i not in (4, 10)]
        assert np.array_equal(out[k][keep].view(np.uint64), batch[k][keep].view(np.uint64)), k      # the other pairs of the batch are untouched
    out = be.point_errors(objs[:6], Te[:6], np.full((6, 3, 4), np.nan), K[:6])
    assert all(np.all(out[k] == np.inf) for k in NAMES)
    # z exactly 0 under the estimate: the one point of model 1 moved onto the camera plane.  PROJ is +inf, the 3-D errors stay finite.
    p = SC.point_models()[0][0].astype(np.float64)
    T0 = np.hstack((np.eye(3), -p[:, None] * np.array([[0.0], [0.0], [1.0]])))
    out = be.point_errors([1], T0[None], Tg[:1], K[:1])
    assert out["proj"][0] == np.inf and np.isfinite(out["add"][0]) and out["add"][0] == out["adi"][0] > 0
    again = be.point_errors(objs, Te, Tg, K)                                   # and the database is as it was
    assert all(np.array_equal(again[k].view(np.uint64), batch[k].view(np.uint64)) for k in NAMES)


def test_one_point_models_and_adi_direction(be):
    """With one point ADI == ADD.  The direction: ground-truth points look for estimated-pose points; on a large perturbation the two directions give
    different means, and the device's is the toolkit's."""
    pm = SC.point_models()
    T = np.hstack((np.eye(3), [[10.0], [0.0], [500.0]]))
    I = np.hstack((np.eye(3), [[0.0], [0.0], [500.0]]))
    out = be.point_errors([1], T[None], I[None], SC.K0)
    assert out["add"][0] == out["adi"][0] == 10.0
    m = 4                                                                      # any model: compare with the numpy restatement in both directions
    Te, Tg = SC.point_pairs()[(m - 1) * SC.PAIRS_PER_MODEL + 1][1:3]
    dev = be.point_errors([m], Te[None], Tg[None], which=("adi",))["adi"][0]
    right, wrong = PR.adi(pm[m - 1], Te, Tg), PR.adi(pm[m - 1], Tg, Te)
    assert abs(dev - right) < 1e-9 * right and abs(right - wrong) > 1e-6 * right


def test_a_model_index_outside_the_database_is_refused(be, pairs):
    objs, Te, Tg, K = pairs
    idx = np.array([len(SC.POINT_COUNTS)], np.int32)
    out = np.zeros(1)
    Kn = np.ascontiguousarray(K[:1]).reshape(1, 9)
    rc = be.lib.suo_pose_errors_points(be._h, 1, idx.ctypes.data, np.ascontiguousarray(Te[:1]).ctypes.data, np.ascontiguousarray(Tg[:1]).ctypes.data, Kn.ctypes.data, 7,
                                       out.ctypes.data, out.ctypes.data, out.ctypes.data)
    assert rc == 1 and b"out of range" in be.lib.suo_last_error()
    rc = be.lib.suo_pose_errors_points(be._h, 1, idx.ctypes.data, None, None, None, 8, None, None, None)
    assert rc == 1 and b"bad argument" in be.lib.suo_last_error()
