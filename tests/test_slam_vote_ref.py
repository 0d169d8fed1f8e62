"""tests/slam_vote_ref.py -- the exact restatement of csrc/slam_vote.hip that tests/test_gpu_slam_vote.py holds the kernel against -- tied to the reference on
the CPU: against oracle/slam_rules.estimate_camera_pose (pinned to the reference's own recorded outputs by tests/test_slam_golden.py) and the product's
ObjectSLAM._estimate_camera_pose on every built case, its priors against the reference's rule (lib/object_slam.py:486-514, restated in numpy here), the
conditions on the inputs that make exact counts a fair demand, the kernel header's claim about numpy's products, the coverage of the rule's edges by the built
cases, and the route predicate that sends a view to the kernel.  No GPU."""
import functools

import numpy as np
import pytest

from oracle import slam_rules as R
from suo_slam_amd.object_slam import ObjectSLAM
from tests import slam_vote_ref as V

U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def cases():
    return {c["name"]: c for c in V.build_cases()}


@functools.lru_cache(maxsize=None)
def ref(name, alt=()):
    return V.vote_ref(cases()[name], alt)


def oracle_cases():
    return [c for c in cases().values() if c.get("oracle", True)]


def _oracle(case):
    det, poses, view, std = V.reference_state(case)
    if not case["has_cov"]:
        for d in det[view].values():
            d["cov_pred"] = None
    return R.estimate_camera_pose(det, poses, view, std, case["min_inliers"]), det, poses


def _pose_bound(case, i):
    """|H - H'| for two evaluations of T_pnp @ inv(T_OtoG) in fp64, each a 4-term dot product of dot products: every entry is within gamma_4 = 4u/(1-4u) of
    the exact sum of |a||b| terms for either evaluation, the translation of the inverse within gamma_3 |R^T||t| before it enters -- so two evaluations differ
    by at most 2 (gamma_4 |P||inv| + |P_R| gamma_3 |R^T||t|) <= 8u (|P||inv| + |P_R||R^T||t|) entrywise."""
    P = np.abs(case["T_pnp"][i].reshape(4, 4)[:3])
    To = case["blk"][V.A_T + 12 * i:V.A_T + 12 * i + 12].reshape(3, 4)
    inv = np.eye(4)
    inv[:3, :3] = np.abs(To[:, :3].T)
    inv[:3, 3] = np.abs(To[:, :3].T) @ np.abs(To[:, 3])
    b = 8 * U * (P @ inv)
    b[:, 3] += 8 * U * (P[:, :3] @ inv[:3, 3])
    return b


def test_restatement_agrees_with_the_oracle_and_the_product():
    """Hypothesis counts exact, the chosen hypothesis equal, the pose within the bound of a 4-term fp64 dot product (_pose_bound)."""
    n_chosen = 0
    for case in oracle_cases():
        got = ref(case["name"])
        out, tr = got["out"], got["trace"]
        (want, want_n, counts), det, poses = _oracle(case)
        hyp = [i for i in range(case["n_a"]) if tr["valid"][i]]
        assert [int(out[15 + i]) for i in hyp] == counts, case["name"]
        assert int(out[13]) == len(counts) and int(out[14]) == want_n, case["name"]
        slam = ObjectSLAM(None, {o: {"diameter": 120.0, "is_symmetric": False} for o in det[1]}, debug_gt_kp=True, manual_kp_std=np.sqrt(case["kp_std2"]))
        slam.no_network_cov = not case["has_cov"]
        slam.detections, slam.obj_poses = det, poses
        prod = slam._estimate_camera_pose(1, case["min_inliers"])
        if want is None:
            assert out[12] == -1 and prod is None and not out[:12].any(), case["name"]
            assert slam.last_cam_hypotheses is None or slam.last_cam_hypotheses["counts"] == counts
            continue
        n_chosen += 1
        best = int(out[12])
        assert counts[hyp.index(best)] == want_n and all(c < want_n for c in counts[:hyp.index(best)]), case["name"]      # the FIRST maximum
        assert slam.last_cam_hypotheses["counts"] == counts and slam.last_cam_hypotheses["best_num_inliers"] == want_n, case["name"]
        bound = _pose_bound(case, best)
        for other in (want, prod):
            assert np.all(np.abs(out[:12].reshape(3, 4) - np.asarray(other)[:3]) <= bound), case["name"]
    assert n_chosen >= 40


def test_inputs_are_conditioned_for_exact_counts():
    """The reference inverts the clamped float32 covariance in float32, the kernel in fp64 closed form: their chi-squares differ near 1e-7 relative.  Exact
    counts are a fair demand only where no keypoint sits that close to the threshold -- and no depth within rounding of 0, except where a case was built to
    sit there.  Checked per (hypothesis, crop) pair against the oracle's own per-pair count, and on the margins themselves."""
    n_pairs = 0
    for case in oracle_cases():
        tr = ref(case["name"])["trace"]
        det, poses, view, std = V.reference_state(case)
        hyp = [i for i in range(case["n_a"]) if tr["valid"][i]]
        if not hyp:
            continue
        H = np.stack([det[view][i + 1]["pose"] @ R.invert_SE3(poses[i + 1]) for i in hyp])
        for a, i in enumerate(hyp):
            for j in hyp:
                d = det[view][j + 1]
                if len(d["inliers"]) == 0:
                    assert (i, j) not in tr["pairs"]
                    continue
                T32 = np.zeros((4, 4), np.float32)
                T32[:3] = poses[j + 1][:3]
                T32[3, 3] = 1
                n = R._count_chi2_inliers(H[a] @ T32, d["model_kp"], d["uv_pred"], d["cov_pred"] if case["has_cov"] else None, d["K"], std)
                p = tr["pairs"][(i, j)]
                assert n == p["count"], (case["name"], i, j)
                n_pairs += 1
                if case.get("edge_depth"):
                    continue
                scale = np.abs(d["model_kp"]).max() + np.abs(H[a]).max() * 2e3
                assert all(abs(z) > 1e-9 * scale for z in p["depth"]), (case["name"], i, j)
                assert all(c is None or abs(c - case["chi2_max"]) > 1e-6 * case["chi2_max"] for c in p["chi2"]), (case["name"], i, j)
    assert n_pairs > 2000


def test_priors_follow_the_reference_rule():
    """lib/object_slam.py:486-514: for every pass-B object in the map, project its model-mask keypoints under T_GtoC @ T_OtoG with the double bbox K; the prior
    exists where np.all(uvd[:, 2] > 0), as float32 uv.  Masks equal; coordinates within 1 float32 ulp (the double products may differ in their last bit,
    which can cross a float32 rounding boundary)."""
    n_on = n_off = 0
    for case in cases().values():
        got = ref(case["name"])
        if got["out"][12] < 0:
            assert not got["prior_mask"].any() and not got["prior_uv"].any()
            continue
        T_GtoC = np.eye(4)
        T_GtoC[:3] = got["out"][:12].reshape(3, 4)
        for s in range(case["n_b"]):
            want_uv, want_m = np.zeros((V.NUM_KP, 2), np.float32), np.zeros(V.NUM_KP, np.uint8)
            if case["blk"][V.B_IN + s] != 0.0:
                m = case["kmask_b"][s].astype(bool)
                T_OtoG = np.concatenate((case["blk"][V.B_T + 12 * s:V.B_T + 12 * s + 12].reshape(3, 4), np.eye(4)[3:4]), 0)
                T_OtoC = T_GtoC @ T_OtoG
                kps_in_C = case["kps_b"][s][m] @ T_OtoC[:3, :3].T + T_OtoC[:3, 3]
                uvd = kps_in_C @ case["blk"][V.B_K + 9 * s:V.B_K + 9 * s + 9].reshape(3, 3).T
                if not case.get("edge_depth"):
                    assert np.all(np.abs(uvd[:, 2]) > 1e-6), (case["name"], s)
                if np.all(uvd[:, 2] > 0):
                    want_uv[m] = uvd[:, :2] / uvd[:, 2:3]
                    want_m[m] = 1
            assert np.array_equal(got["prior_mask"][s], want_m), (case["name"], s)
            n_on += bool(want_m.any())
            n_off += not want_m.any()
            ulp = np.spacing(np.abs(want_uv))
            assert np.all(np.abs(got["prior_uv"][s].astype(np.float64) - want_uv) <= ulp), (case["name"], s)
    assert n_on > 100 and n_off >= 5


def test_numpy_products_are_the_documented_fma_chain():
    """The kernel header's claim, pinned for THIS numpy build: the 4 x 4 product, the stacked 4 x 4 product, (-R^T) t and n x 3 @ 3 x 3 come out of numpy as
    fma(a3, b3, fma(a2, b2, fma(a1, b1, a0 b0))) in ascending k -- bit for bit.  It is why the device chain's poses and priors equal the host route's
    (tests/test_gpu_slam_chain.py).  A failure on another host (another BLAS, another CPU) is a finding about the HOST ROUTE's rounding there, not about the
    kernel: the kernel is held to the documented chain itself by tests/test_gpu_slam_vote.py, wherever it runs."""
    rng = np.random.default_rng(17)

    def chain(a, b):
        acc = a[0] * b[0]
        for k in range(1, len(a)):
            acc = V.fma(float(a[k]), float(b[k]), acc)
        return acc

    def matmul_ref(A, B):
        return np.array([[chain(A[i], B[:, j]) for j in range(B.shape[1])] for i in range(A.shape[0])])

    bad = total = 0
    for _ in range(60):
        A, B = (np.eye(4) for _ in range(2))
        for T in (A, B):
            T[:3, :3] = V.SS.random_rotation(rng)
            T[:3, 3] = rng.uniform(-1000, 1000, 3)
        bad += np.count_nonzero(V.bits64(A @ B) != V.bits64(matmul_ref(A, B)))                                  # 4 x 4
        S = (np.stack([A, B])[:, None] @ np.stack([B, A]).astype(np.float32).astype(np.float64)[None])           # stacked, as _estimate_camera_pose forms it
        for i, X in enumerate((A, B)):
            for j, Y in enumerate((B, A)):
                bad += np.count_nonzero(V.bits64(S[i, j]) != V.bits64(matmul_ref(X, Y.astype(np.float32).astype(np.float64))))
        t = -A[:3, :3].T @ A[:3, 3]                                                                            # (-R^T) t
        bad += np.count_nonzero(V.bits64(t) != V.bits64(np.array([chain(-A[:3, r], A[:3, 3]) for r in range(3)])))
        n = int(rng.integers(1, 42))
        pts = rng.uniform(-60, 60, (n, 3)).astype(np.float32)
        for M in (A[:3, :3], V.SS.K_YCBV * rng.uniform(0.5, 2)):                                                # n x 3 @ 3 x 3 (float32 points, as the reference has them)
            bad += np.count_nonzero(V.bits64(pts @ M.T) != V.bits64(matmul_ref(pts.astype(np.float64), M.T)))
            total += 3 * n
        total += 16 + 64 + 3
    assert total > 8000 and bad == 0, (bad, total)


# ---- coverage: every situation of the rule is reached by a built case, judged from the restatement's own trace ----------------------------------------------
def _situations(case, res):
    tr, out = res["trace"], res["out"]
    n_a, n_b = case["n_a"], case["n_b"]
    hyp = [i for i in range(n_a) if tr["valid"][i]]
    cnt = [tr["counts"][i] for i in hyp]
    top = max(cnt) if cnt else -1
    acc, inm = case["accepted"] != 0, case["blk"][V.A_IN:V.A_IN + n_a] != 0.0
    s = set()
    if cnt and top == 3 and case["min_inliers"] == 4 and tr["best"] < 0:
        s.add("best count exactly 3: none")
    if cnt and top == 4 and case["min_inliers"] == 4 and tr["best"] >= 0:
        s.add("best count exactly 4: chosen")
    if case["min_inliers"] == 1 and 0 < top < 4 and tr["best"] >= 0:
        s.add("min_inliers=1 honoured")
    if case["min_inliers"] == 5 and top == 4 and tr["best"] < 0:
        s.add("min_inliers=5 honoured")
    if top >= case["min_inliers"] and cnt.count(top) == 2:
        s.add("two hypotheses tied for the maximum")
        i, j = [h for h in hyp if tr["counts"][h] == top]
        if not np.array_equal(case["T_pnp"][i], case["T_pnp"][j]):
            s.add("tie between different poses")
    if top >= case["min_inliers"] and cnt.count(top) >= 3:
        s.add("three-way tie")
    if tr["best"] > 0 and any(tr["counts"][h] >= case["min_inliers"] for h in hyp if h < tr["best"]):
        s.add("a later hypothesis with strictly more wins")
    if np.any(acc & ~inm):
        s.add("accepted, not in the map")
    if np.any(~acc & inm):
        s.add("in the map, rejected")
    if np.any(~acc & ~inm):
        s.add("rejected and not in the map")
    if any(tr["valid"][j] and tr["nrow"][j] == 0 for j in range(n_a)) and len(hyp) > 1:
        s.add("accepted crop with an empty mask")
    if not hyp:
        s.add("no hypothesis at all")
    for p in tr["pairs"].values():
        if any(z <= 0 for z in p["depth"]) and any(z > 0 for z in p["depth"]):
            s.add("vote: some keypoints of a scored crop behind the camera")
        if any(z == 0 for z in p["depth"]):
            s.add("vote: depth exactly 0")
    for sb, dep in tr["prior_depth"].items():
        if any(z <= 0 for z in dep.values()):
            s.add("prior: model-mask keypoint at depth <= 0")
        if any(z == 0 for z in dep.values()):
            s.add("prior: depth exactly 0")
    if tr["best"] >= 0 and np.any(case["blk"][V.B_IN:V.B_IN + n_b] == 0.0):
        s.add("pass-B object not in the map")
    if tr["best"] >= 0 and any(tr["prior_considered"][k] and not case["kmask_b"][k].any() for k in range(n_b)):
        s.add("all-false model mask")
    if case["has_cov"]:
        for j in hyp:
            c = case["cov"][j][case["mask"][j] != 0]
            if len(c):
                lo0, lo3 = c[:, 0] < 1e-4, c[:, 3] < 1e-4
                if np.any(lo0 ^ lo3):
                    s.add("one variance under the clamp")
                if np.any(lo0 & lo3):
                    s.add("both variances under the clamp")
                if np.any(c[:, 1] != c[:, 2]):
                    s.add("unequal off-diagonals")
                if np.any(np.abs(c[:, 1]) > 0.5 * np.sqrt(c[:, 0] * c[:, 3])):
                    s.add("correlated covariance")
    if n_a == 16:
        s.add("n_a = 16")
    if n_b == 16:
        s.add("n_b = 16")
    for j in hyp:
        m = case["mask"][j] != 0
        if m.all():
            s.add("a crop with 41 keypoints")
        if m.any() and not m[:int(m.sum())].all():
            s.add("scattered mask")
        if m[40] and not m.all():
            s.add("lane 40 valid in a partial mask")
    if out[31] == 1.0:
        s.add("NaN flag set")
    if out[31] == 0.0 and np.isnan(case["cov"]).any():
        s.add("NaN that must not set the flag")
    if case["has_cov"] == 0:
        s.add("manual sigma")
    return s


SITUATIONS = (
    "best count exactly 3: none", "best count exactly 4: chosen", "min_inliers=1 honoured", "min_inliers=5 honoured", "two hypotheses tied for the maximum",
    "tie between different poses", "three-way tie", "a later hypothesis with strictly more wins", "accepted, not in the map", "in the map, rejected",
    "rejected and not in the map", "accepted crop with an empty mask", "no hypothesis at all", "vote: some keypoints of a scored crop behind the camera",
    "vote: depth exactly 0", "prior: model-mask keypoint at depth <= 0", "prior: depth exactly 0", "pass-B object not in the map", "all-false model mask",
    "one variance under the clamp", "both variances under the clamp", "unequal off-diagonals", "correlated covariance", "n_a = 16", "n_b = 16",
    "a crop with 41 keypoints", "scattered mask", "lane 40 valid in a partial mask", "NaN flag set", "NaN that must not set the flag", "manual sigma")


def test_every_situation_is_reached_by_a_built_case():
    reached = {}
    for case in cases().values():
        for s in _situations(case, ref(case["name"])):
            reached.setdefault(s, []).append(case["name"])
    missing = [s for s in SITUATIONS if s not in reached]
    assert not missing, missing


@pytest.mark.parametrize("alt", V.ALTERNATIVES)
def test_a_built_case_tells_each_alternative_reading_from_the_intended_one(alt):
    """For every alternative semantic of tests/slam_vote_ref.ALTERNATIVES there is a built case whose results (pose, choice, counts, flag, priors) differ under
    it -- at the ordinary threshold for the discrete ones; the last-bit ones (containers, chain against plain sums) are separated by a placed threshold
    (semantic_pairs).  A kernel implementing the alternative cannot pass tests/test_gpu_slam_vote.py."""
    def differs(c, a, b):
        return (not np.array_equal(V.bits64(a["out"]), V.bits64(b["out"])) or not np.array_equal(V.bits32(a["prior_uv"]), V.bits32(b["prior_uv"]))
                or not np.array_equal(a["prior_mask"], b["prior_mask"]))
    hits = [n for n, c in cases().items() if n.split(" n_a=")[0] != "random" or c["n_a"] <= 5 if differs(c, ref(n), ref(n, alt))]
    if alt in PLACED:
        hits += [c["name"] for c, _ in semantic_pairs(alt)]
    assert hits, alt


# ---- section 4: a threshold placed between two readings of one keypoint -----------------------------------------------------------------------------------
PLACED = {"double_map_pose": "the float32 container of the scored map pose, against the double pose",
          "double_K_a": "pass A's K as the widened float32 container, against the double K",
          "clamp_offdiag": "the clamp at 1e-4 on the diagonal only",
          "fma_points": "the plain-sum point transform, against the FMA chain"}
PLACED_ON = ("random n_a=5 n_b=3 cov=1", "covariances under the clamp, one or both; unequal off-diagonals", "random n_a=2 n_b=1 cov=0")


def semantic_pairs(alt):
    """[(case with chi2_max placed, (i, j, k))]: one keypoint of a built case whose chi-square differs between the intended reading and ``alt``, with chi2_max
    at the midpoint of the two (at the smaller one where they are neighbouring doubles, which chi2 <= chi2_max separates as well)."""
    got = []
    for name in PLACED_ON:
        case = cases()[name]
        if alt == "clamp_offdiag" and not case["has_cov"]:
            continue
        a, b = ref(name)["trace"]["pairs"], ref(name, alt)["trace"]["pairs"]
        cand = []
        for key in sorted(a):
            for k, (x, y) in enumerate(zip(a[key]["chi2"], b[key]["chi2"])):
                if x is not None and y is not None and x != y and np.isfinite(x) and np.isfinite(y):
                    cand.append((abs(x - y) / x, key, k, x, y))
        for _, key, k, x, y in sorted(cand, reverse=True)[:12]:        # the widest gaps first; keep the first whose hypothesis TOTAL tells the readings apart
            mid = 0.5 * (x + y)
            if not (min(x, y) < mid < max(x, y)):
                mid = min(x, y)
            c = V._copy(case, f"{name} | chi2_max between the readings: {alt}")
            c["chi2_max"] = mid
            if V.vote_ref(c)["trace"]["counts"][key[0]] != V.vote_ref(c, alt)["trace"]["counts"][key[0]]:
                got.append((c, key + (k,)))
                break
    return got


@pytest.mark.parametrize("alt", sorted(PLACED))
def test_placed_thresholds_separate_the_readings(alt):
    """No pair is skipped: each of the four has keypoints whose two readings round to different doubles on the built cases."""
    pairs = semantic_pairs(alt)
    assert pairs, alt
    for c, (i, j, k) in pairs:
        a, b = V.vote_ref(c), V.vote_ref(c, alt)
        x, y = a["trace"]["pairs"][(i, j)]["chi2"][k], b["trace"]["pairs"][(i, j)]["chi2"][k]
        assert (x <= c["chi2_max"]) != (y <= c["chi2_max"]), c["name"]
        assert a["trace"]["counts"][i] != b["trace"]["counts"][i], c["name"]


def test_double_K_reading_is_what_the_oracle_scores_with():
    """The reference keeps a detection's K as float32 (:1082) and scores with it: on the placed-threshold case the oracle's count follows the float32 container."""
    for c, (i, j, k) in semantic_pairs("double_K_a"):
        assert not np.array_equal(c["K_a_double"][j].reshape(-1), c["blk"][V.A_K + 9 * j:V.A_K + 9 * j + 9])
        assert np.array_equal(c["K_a_double"][j].astype(np.float32).astype(np.float64).reshape(-1), c["blk"][V.A_K + 9 * j:V.A_K + 9 * j + 9])


# ---- the route predicate ----------------------------------------------------------------------------------------------------------------------------------
def _stub(**kw):
    slam = ObjectSLAM(None, {1: {"diameter": 100.0, "is_symmetric": False}}, debug_gt_kp=True)
    slam.debug_gt_kp = False
    slam.model = object()
    slam.device_chain = True
    slam.cam_poses = {0: np.eye(4)}
    for k, v in kw.items():
        setattr(slam, k, v)
    return slam


def test_route_predicate_at_its_boundaries(monkeypatch):
    monkeypatch.delenv("SUO_SLAM_VOTE_CHAIN", raising=False)
    take = lambda slam, view=5, cam=None, n=3, m=2: bool(slam._slam_view_takes_the_vote_chain(view, cam, n, m))   # noqa: E731
    assert take(_stub())
    for n, want in ((0, False), (1, True), (16, True), (17, False)):
        assert take(_stub(), n=n) is want and take(_stub(), m=n) is want, n
    assert take(_stub(), n=16, m=16) and not take(_stub(), n=17, m=16) and not take(_stub(), n=16, m=17)
    assert not take(_stub(), cam=np.eye(4))                              # cam_pose given
    assert not take(_stub(no_prior_det=True))
    assert not take(_stub(single_view_mode=True))
    assert not take(_stub(cam_poses={}))                                 # first view
    assert not take(_stub(), view=0)                                     # the view already has a pose
    assert not take(_stub(device_chain=False)) and not take(_stub(model=None))
    assert not take(_stub(debug_gt_kp=True, debug_gt_on_device=False)) and take(_stub(debug_gt_kp=True, debug_gt_on_device=True))
    for val, want in (("", False), ("0", False), ("1", True)):
        monkeypatch.setenv("SUO_SLAM_VOTE_CHAIN", val)
        assert take(_stub()) is want, val
