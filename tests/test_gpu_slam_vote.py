"""csrc/slam_vote.hip (``suo_slam_vote``) called directly, at the edges of the rule it restates (lib/object_slam.py:975-1072 and :486-514): every output buffer
against tests/slam_vote_ref.vote_ref BIT FOR BIT -- the camera pose, the choice, the hypothesis count, the best count, the 16 counts, the NaN flag, the float32
priors and their masks -- and counts / choice / best count against oracle/slam_rules.estimate_camera_pose.  tests/test_slam_vote_ref.py ties the restatement to
the oracle and the reference's prior rule on the CPU and proves that the cases built in tests/slam_vote_ref.build_cases reach every edge.  Each case is one
single-workgroup launch; the output buffers are prefilled with sentinels."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from suo_slam_amd import _lib  # noqa: E402
from tests import slam_vote_ref as V  # noqa: E402
from tests import test_slam_vote_ref as TV  # noqa: E402
from tests.hipops import P, S  # noqa: E402

SUO_ERR_ARG = 1
OUT_SENTINEL, UV_SENTINEL, MASK_SENTINEL = -7.5, -9.25, 0xAB
DTYPES = {"T_pnp": np.float64, "accepted": np.uint8, "uv": np.float32, "cov": np.float32, "mask": np.uint8, "kps_a": np.float32, "blk": np.float64,
          "kps_b": np.float32, "kmask_b": np.uint8}


def upload(case):
    return {k: torch.from_numpy(np.ascontiguousarray(case[k], DTYPES[k])).cuda() for k in V.ARRAYS}


def out_buffers():
    return (torch.full((V.OUT,), OUT_SENTINEL, dtype=torch.float64, device="cuda"), torch.full((V.MAX_CROPS, V.NUM_KP, 2), UV_SENTINEL, device="cuda"),
            torch.full((V.MAX_CROPS, V.NUM_KP), MASK_SENTINEL, dtype=torch.uint8, device="cuda"))


def launch(case, dev, bufs, **over):
    a = dict(n_a=case["n_a"], n_b=case["n_b"], has_cov=case["has_cov"], kp_std2=case["kp_std2"], chi2_max=case["chi2_max"], min_inliers=case["min_inliers"])
    ptr = {k: P(dev[k]) for k in V.ARRAYS}
    ptr.update(out=P(bufs[0]), prior_uv=P(bufs[1]), prior_mask=P(bufs[2]))
    for k, v in over.items():
        (a if k in a else ptr)[k] = v
    return _lib.lib().suo_slam_vote(a["n_a"], ptr["T_pnp"], ptr["accepted"], None, ptr["uv"], ptr["cov"], ptr["mask"], ptr["kps_a"], ptr["blk"], a["n_b"],
                                    ptr["kps_b"], ptr["kmask_b"], a["has_cov"], C.c_double(a["kp_std2"]), C.c_double(a["chi2_max"]), a["min_inliers"],
                                    ptr["prior_uv"], ptr["prior_mask"], ptr["out"], S())


def run(case):
    dev, bufs = upload(case), out_buffers()
    _lib.check(launch(case, dev, bufs), "suo_slam_vote")
    torch.cuda.synchronize()
    return tuple(b.cpu().numpy() for b in bufs)


def check(case, got, want=None):
    """Bit for bit against the restatement; rows >= n_b of the prior buffers untouched; out[15 + i] = -1 for i >= n_a."""
    out, puv, pmk = got
    want = want or V.vote_ref(case)
    n_a, n_b, name = case["n_a"], case["n_b"], case["name"]
    print(f"{name}: best {out[12]:.0f} of {out[13]:.0f} hypotheses, best_n {out[14]:.0f}, counts {out[15:15 + n_a].astype(int).tolist()}, NaN flag {out[31]:.0f}, "
          f"priors on {pmk[:n_b].any(1).astype(int).tolist()}")
    assert np.array_equal(V.bits64(out[:12]), V.bits64(want["out"][:12])), (name, out[:12] - want["out"][:12])
    assert np.array_equal(V.bits64(out[12:15]), V.bits64(want["out"][12:15])), (name, out[12:15], want["out"][12:15])
    assert np.array_equal(V.bits64(out[15:31]), V.bits64(want["out"][15:31])), (name, out[15:31], want["out"][15:31])
    assert np.all(out[15 + n_a:31] == -1.0), name
    assert V.bits64(out[31:]) == V.bits64(want["out"][31:]), (name, out[31])
    assert np.array_equal(pmk[:n_b], want["prior_mask"]), name
    assert np.array_equal(V.bits32(puv[:n_b]), V.bits32(want["prior_uv"])), (name, np.abs(puv[:n_b] - want["prior_uv"]).max())
    assert np.all(puv[n_b:] == UV_SENTINEL) and np.all(pmk[n_b:] == MASK_SENTINEL), name
    return want


def check_oracle(case, out):
    (pose, best_n, counts), _, _ = TV._oracle(case)
    hyp = [i for i in range(case["n_a"]) if out[15 + i] >= 0]
    assert [int(out[15 + i]) for i in hyp] == counts and int(out[13]) == len(counts) and int(out[14]) == best_n, case["name"]
    if pose is None:
        assert out[12] == -1
    else:
        assert counts.index(best_n) == hyp.index(int(out[12])), case["name"]                    # the first maximum
        assert np.all(np.abs(out[:12].reshape(3, 4) - pose[:3]) <= TV._pose_bound(case, int(out[12]))), case["name"]      # a 4-term fp64 dot product's bound


def _named(pred):
    return [c for n, c in TV.cases().items() if pred(n)]


@pytest.mark.parametrize("n_a", [1, 2, 5, 8, 15, 16])
def test_random_tracking_states(n_a):
    """n_a in {1, 2, 5, 8, 15, 16} x n_b in {1, 3, 16} x has_cov in {0, 1}; 4 to 41 keypoints per crop, one crop with all 41; scattered and prefix masks."""
    cs = _named(lambda n: n.startswith(f"random n_a={n_a} "))
    assert len(cs) == 6
    for c in cs:
        got = run(c)
        check(c, got, TV.ref(c["name"]))
        check_oracle(c, got[0])


def test_validity_combinations():
    """accepted and not in the map / in the map and rejected / both / an accepted crop with an empty mask / no hypothesis at all.  An invalid crop neither
    proposes nor is scored: its count is -1, and the same case with OTHER values wherever the kernel must not look gives the same bits."""
    a, b = TV.cases()["validity: rejected / unmapped / both / empty mask"], TV.cases()["validity: the same with other decoys"]
    ga, gb = run(a), run(b)
    check(a, ga)
    check(b, gb)
    check_oracle(a, ga[0])
    assert ga[0][15:21].astype(int).tolist()[1:4] == [-1, -1, -1] and ga[0][13] == 3
    for x, y in zip(ga, gb):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    a, b = TV.cases()["no hypothesis at all"], TV.cases()["no hypothesis at all: other decoys"]
    for c in (a, b):
        out, puv, pmk = run(c)
        check(c, (out, puv, pmk))
        check_oracle(c, out)
        assert out[12] == -1 and out[13] == 0 and out[14] == -1 and not out[:12].any() and not pmk[:c["n_b"]].any() and not puv[:c["n_b"]].any()


def test_count_boundaries_and_min_inliers():
    """A best count of exactly 3 gives none, of exactly 4 a choice (:1068); min_inliers passed as 1 and as 5 is honoured."""
    want = {"best count exactly 3": (-1, 3), "best count exactly 4": (0, 4), "min_inliers=1 takes a count of 3": (0, 3),
            "min_inliers=5 refuses a count of 4": (-1, 4), "min_inliers=1, count 4": (0, 4)}
    for name, (best, count) in want.items():
        c = TV.cases()[name]
        out, puv, pmk = run(c)
        check(c, (out, puv, pmk))
        check_oracle(c, out)
        assert (int(out[12]), int(out[15])) == (best, count), name
        assert pmk[:c["n_b"]].any() == (best >= 0)


def test_ties_take_the_first_maximum():
    for name, best in (("tie of two: the lower index wins", 1), ("tie of three", 1), ("a later hypothesis with strictly more wins", 2)):
        c = TV.cases()[name]
        got = run(c)
        check(c, got)
        check_oracle(c, got[0])
        assert int(got[0][12]) == best, name
    cnt = run(TV.cases()["tie of three"])[0][15:20]
    assert cnt[1] == cnt[3] == cnt[4] == cnt.max()


def test_depth_in_the_vote_and_in_the_priors():
    """Keypoints of a scored crop behind the camera, a third homogeneous coordinate whose sign is not z's, a depth of exactly 0 (not in front); priors switched off
    by a model-mask keypoint at depth <= 0 and NOT by one outside the model mask, a pass-B object that is not in the map, an all-false model mask."""
    for c in _named(lambda n: n.startswith("vote: ") or n.startswith("priors: ") or n == "depth exactly 0"):
        got = run(c)
        check(c, got)
        check_oracle(c, got[0])
    pmk = run(TV.cases()["priors: depth <= 0 in and out of the model mask, unmapped, empty model mask"])[2]
    assert pmk[:6].any(1).astype(int).tolist() == [0, 1, 0, 0, 0, 1]
    out, _, pmk = run(TV.cases()["depth exactly 0"])
    assert int(out[15]) == 6 and pmk[:2].any(1).astype(int).tolist() == [0, 1]


def test_covariances():
    """Variances under the 1e-4 clamp (one or both), tiny_cov states, correlated entries, unequal off-diagonals (the kernel's b + c)."""
    for c in _named(lambda n: "covariances" in n or n == "tiny_cov state"):
        got = run(c)
        check(c, got)
        check_oracle(c, got[0])


def test_nan_flag():
    """Non-finite VALUES only.  A NaN covariance -- the whole matrix, a variance alone (np.maximum keeps it: :1054-1056) or an off-diagonal entry alone -- on a
    valid keypoint of a scored crop sets out[31]; the same NaN on a masked-out keypoint or on an unscored crop does not."""
    for c in _named(lambda n: n.startswith("NaN ")):
        out = check(c, run(c))["out"]
        assert out[31] == (1.0 if "valid keypoint of a scored crop" in c["name"] else 0.0), c["name"]


@pytest.mark.parametrize("alt", sorted(TV.PLACED))
def test_threshold_placed_between_two_readings(alt):
    """chi2_max at the midpoint of one keypoint's chi-square under the intended reading and under the alternative (tests/test_slam_vote_ref.PLACED): the count
    follows the intended reading."""
    pairs = TV.semantic_pairs(alt)
    assert pairs
    for c, (i, j, k) in pairs:
        want, other = V.vote_ref(c), V.vote_ref(c, alt)
        assert want["trace"]["counts"][i] != other["trace"]["counts"][i]
        got = run(c)
        out = got[0]
        check(c, got, want)
        assert int(out[15 + i]) == want["trace"]["counts"][i] != other["trace"]["counts"][i], c["name"]


def test_no_state_survives_a_launch():
    """The same call twice on the same buffers; then a smaller call behind a larger one on one stream, without a wait between them."""
    big, small = TV.cases()["random n_a=16 n_b=16 cov=1"], TV.cases()["best count exactly 3"]
    dev, bufs = upload(big), out_buffers()
    _lib.check(launch(big, dev, bufs), "suo_slam_vote")
    torch.cuda.synchronize()
    first = tuple(b.cpu().numpy() for b in bufs)
    _lib.check(launch(big, dev, bufs), "suo_slam_vote")
    torch.cuda.synchronize()
    for x, y in zip(first, (b.cpu().numpy() for b in bufs)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    check(big, first, TV.ref(big["name"]))
    dev_s, bufs_s = upload(small), out_buffers()
    _lib.check(launch(big, dev, bufs), "suo_slam_vote")
    _lib.check(launch(small, dev_s, bufs_s), "suo_slam_vote")
    torch.cuda.synchronize()
    check(small, tuple(b.cpu().numpy() for b in bufs_s))


def test_argument_errors_launch_nothing():
    c = TV.cases()["random n_a=2 n_b=3 cov=1"]
    dev, bufs = upload(c), out_buffers()
    bad = [dict(n_a=0), dict(n_a=17), dict(n_b=0), dict(n_b=17), dict(n_a=-1)] + [{k: None} for k in V.ARRAYS + ("out", "prior_uv", "prior_mask")]
    for over in bad:
        assert launch(c, dev, bufs, **over) == SUO_ERR_ARG, over
        assert b"suo_slam_vote" in _lib.lib().suo_last_error(), over
        with pytest.raises(_lib.SuoError, match="suo_slam_vote"):
            _lib.check(launch(c, dev, bufs, **over), "suo_slam_vote")
    torch.cuda.synchronize()
    assert torch.all(bufs[0] == OUT_SENTINEL) and torch.all(bufs[1] == UV_SENTINEL) and torch.all(bufs[2] == MASK_SENTINEL)
    _lib.check(launch(c, dev, bufs), "suo_slam_vote")                  # ... and the same buffers are served by a good call
    torch.cuda.synchronize()
    check(c, tuple(b.cpu().numpy() for b in bufs))
