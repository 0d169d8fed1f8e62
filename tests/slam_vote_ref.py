"""An exact restatement of csrc/slam_vote.hip (``suo_slam_vote``) in plain Python, and the builders of the cases it is tested on.

Plain Python + numpy: nothing here imports the product or the oracle.  ``vote_ref`` takes exactly the arrays the kernel takes and follows
the kernel's header step by step; every operation is either a plain Python float operation (an IEEE double operation, never contracted --
what the kernel does under -ffp-contract=off) or ``fma``, which is correctly rounded through exact rational arithmetic.  So its outputs are
what the documented arithmetic gives TO THE BIT, and tests/test_gpu_slam_vote.py compares the kernel's buffers with them as bit patterns.

``alt`` selects alternative semantics, one name each (ALTERNATIVES): the readings a plausible mistake in the kernel would implement.  The
tests use them to prove that a built case tells the intended reading from the alternative, and to place ``chi2_max`` between the two.

A *case* is a dict of the kernel's arguments (``ARRAYS`` + scalars) plus ``name``; ``reference_state`` gives the same numbers as the
reference-shaped ``detections`` / ``obj_poses`` dicts (float32-rounded, every inlier flag set) that oracle/slam_rules.estimate_camera_pose
and ObjectSLAM._estimate_camera_pose read.
"""
import math
from fractions import Fraction

import numpy as np

from tests import slam_states as SS

NUM_KP, MAX_CROPS = 41, 16
# the host block (include/suo_hip.h: SUO_SLAM_VOTE_BLOCK doubles): a_in_map [16] | a_T [16][12] | a_K [16][9] | b_in_map [16] | b_T [16][12] | b_K [16][9]
A_IN, A_T, A_K, B_IN, B_T, B_K, BLOCK = 0, 16, 208, 352, 368, 560, 704
OUT = 32
CHI2_2DOF_95 = 5.991
ARRAYS = ("T_pnp", "accepted", "uv", "cov", "mask", "kps_a", "blk", "kps_b", "kmask_b")

ALTERNATIVES = (
    "vote_ge",             # a later hypothesis with an EQUAL count replaces the earlier one
    "double_map_pose",     # the scored map pose without its float32 container
    "double_K_a",          # pass A's intrinsics as the double K (case["K_a_double"]) instead of the widened float32 container
    "front_on_p",          # the z > 0 test of the vote on the camera-frame point instead of on the third homogeneous coordinate
    "prior_front_on_p",    # ... of the priors
    "ok_all_lanes",        # a prior switched off by ANY of the 41 keypoints at non-positive depth, in the model mask or not
    "clamp_offdiag",       # the 1e-4 clamp also applied to the off-diagonal entry b
    "plain_chain",         # the pose algebra as plain products and sums instead of the FMA chain
    "fma_points",          # the scored point transform as the FMA chain instead of plain sums
)


def fma(a, b, c):
    """a * b + c rounded once (IEEE fusedMultiplyAdd, round to nearest even), signed zeros included."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    if a == 0.0 or b == 0.0:
        return (a * b) + c                       # the product is an exact (signed) zero
    r = Fraction(a) * Fraction(b) + Fraction(c)
    return float(r) if r != 0 else 0.0           # an exact cancellation of non-zero terms is +0 in round-to-nearest


def _chain3(plain):
    if plain:
        return lambda a0, b0, a1, b1, a2, b2: (a0 * b0 + a1 * b1) + a2 * b2
    return lambda a0, b0, a1, b1, a2, b2: fma(a2, b2, fma(a1, b1, a0 * b0))


def _mul34(A, B, chain3):
    """Rows 0-2 of the product of two rigid transforms given as 12 doubles (their fourth rows are 0 0 0 1): sv_mul34."""
    C = [0.0] * 12
    for i in range(3):
        for j in range(4):
            b3 = 1.0 if j == 3 else 0.0
            C[i * 4 + j] = fma(A[i * 4 + 3], b3, chain3(A[i * 4], B[j], A[i * 4 + 1], B[4 + j], A[i * 4 + 2], B[8 + j]))
    return C


def _clamp(v):
    """np.maximum(v, 1e-4): a NaN stays a NaN (:1054)."""
    return 1e-4 if v < 1e-4 else v


def vote_ref(inp, alt=()):
    """-> {"out": [32] float64, "prior_uv": [n_b,41,2] float32, "prior_mask": [n_b,41] uint8, "trace": {...}}.

    trace: "valid" [n_a], "nrow" [n_a], "pairs" {(i, j): {"depth": [...], "chi2": [... or None], "count": n}}, "prior_depth" {s: {lane: q2}},
    "prior_considered" [n_b] (the crop's object is in the map and there is a camera pose)."""
    alt = frozenset([alt] if isinstance(alt, str) else alt)
    assert alt <= set(ALTERNATIVES), alt
    n_a, n_b = int(inp["n_a"]), int(inp["n_b"])
    T_pnp = np.asarray(inp["T_pnp"], np.float64).reshape(-1)
    blk = [float(v) for v in np.asarray(inp["blk"], np.float64)]
    uv, cov, kps_a = (np.asarray(inp[k], np.float32) for k in ("uv", "cov", "kps_a"))
    mask, accepted = np.asarray(inp["mask"], np.uint8), np.asarray(inp["accepted"], np.uint8)
    kps_b, kmask_b = np.asarray(inp["kps_b"], np.float32), np.asarray(inp["kmask_b"], np.uint8)
    has_cov, kp_std2, chi2_max, min_inliers = int(inp["has_cov"]), float(inp["kp_std2"]), float(inp["chi2_max"]), int(inp["min_inliers"])
    chain3 = _chain3("plain_chain" in alt)

    # 1. scoring rows: the valid keypoints of every crop in mask order, widened to double
    rows, valid = [], []
    for j in range(n_a):
        idx = [l for l in range(NUM_KP) if mask[j, l] != 0]
        K = blk[A_K + 9 * j:A_K + 9 * j + 9]
        if "double_K_a" in alt:
            K = [float(v) for v in np.asarray(inp["K_a_double"][j], np.float64).reshape(-1)]
        rows.append({"pts": [[float(kps_a[j, l, c]) for c in range(3)] for l in idx], "uv": [[float(uv[j, l, c]) for c in range(2)] for l in idx],
                     "cov": [[float(cov[j, l].reshape(-1)[c]) for c in range(4)] for l in idx], "K": K, "n": len(idx)})
        valid.append(bool(accepted[j] != 0 and blk[A_IN + j] != 0.0))

    # 2. hypotheses T_pnp[i] @ inv(T_OtoG[i]) and the float32 containers of the map poses
    H, T32 = [None] * n_a, [None] * n_a
    for i in range(n_a):
        if not valid[i]:
            continue
        To = blk[A_T + 12 * i:A_T + 12 * i + 12]
        inv = [0.0] * 12
        for r in range(3):
            for c in range(3):
                inv[r * 4 + c] = To[c * 4 + r]
            inv[r * 4 + 3] = chain3(-To[r], To[3], -To[4 + r], To[7], -To[8 + r], To[11])               # (-R^T) @ t
        P = [float(T_pnp[i * 16 + k]) for k in range(12)]
        H[i] = _mul34(P, inv, chain3)
        T32[i] = list(To) if "double_map_pose" in alt else [float(np.float32(v)) for v in To]

    # 3. counts[i] = sum over the scored crops j of #{k: z > 0, chi2_k <= chi2_max} under H[i] @ T32[j]
    counts, pairs, nan = [0] * n_a, {}, False
    for i in range(n_a):
        if not valid[i]:
            continue
        for j in range(n_a):
            if not valid[j] or rows[j]["n"] <= 0:
                continue
            T = _mul34(H[i], T32[j], chain3)
            row, K = rows[j], rows[j]["K"]
            tr = {"depth": [], "chi2": [], "count": 0}
            for k in range(row["n"]):
                x, y, z = row["pts"][k]
                if "fma_points" in alt:
                    p = [_chain3(False)(x, T[r * 4], y, T[r * 4 + 1], z, T[r * 4 + 2]) + T[r * 4 + 3] for r in range(3)]
                else:
                    p = [((x * T[r * 4] + y * T[r * 4 + 1]) + z * T[r * 4 + 2]) + T[r * 4 + 3] for r in range(3)]
                q = [(p[0] * K[r * 3] + p[1] * K[r * 3 + 1]) + p[2] * K[r * 3 + 2] for r in range(3)]
                depth = p[2] if "front_on_p" in alt else q[2]
                tr["depth"].append(q[2])
                chi2 = None
                if depth > 0.0:
                    rx = row["uv"][k][0] - _div(q[0], q[2])
                    ry = row["uv"][k][1] - _div(q[1], q[2])
                    if has_cov:
                        c = row["cov"][k]
                        aa, d, bb, cc = _clamp(c[0]), _clamp(c[3]), c[1], c[2]
                        if "clamp_offdiag" in alt:
                            bb = _clamp(bb)
                        chi2 = _div((d * rx * rx - (bb + cc) * rx * ry) + aa * ry * ry, aa * d - bb * cc)
                    else:
                        chi2 = _div(rx * rx + ry * ry, kp_std2)
                    nan = nan or chi2 != chi2
                    if chi2 <= chi2_max:
                        tr["count"] += 1
                tr["chi2"].append(chi2)
            counts[i] += tr["count"]
            pairs[(i, j)] = tr

    # 4. the first hypothesis with the most inliers, if it has at least min_inliers
    best, best_n, nh = -1, -1, 0
    for i in range(n_a):
        if not valid[i]:
            continue
        nh += 1
        if counts[i] >= min_inliers and (counts[i] >= best_n if "vote_ge" in alt else counts[i] > best_n):
            best, best_n = i, counts[i]
    out = np.zeros(OUT)
    cam = H[best] if best >= 0 else [0.0] * 12
    out[:12] = cam
    out[12:15] = best, nh, best_n
    for i in range(MAX_CROPS):
        out[15 + i] = counts[i] if (i < n_a and valid[i]) else -1.0
    out[31] = 1.0 if nan else 0.0

    # 5. priors of pass B's crops: float32 NDC of project(K_bbox[s], cam @ T_OtoG[s], model keypoints) where ALL depths are positive
    prior_uv, prior_mask = np.zeros((n_b, NUM_KP, 2), np.float32), np.zeros((n_b, NUM_KP), np.uint8)
    prior_depth, considered = {}, [False] * n_b
    for s in range(n_b):
        if not (best >= 0 and blk[B_IN + s] != 0.0):
            continue
        considered[s] = True
        T = _mul34(cam, blk[B_T + 12 * s:B_T + 12 * s + 12], chain3)
        K = blk[B_K + 9 * s:B_K + 9 * s + 9]
        ok, got, prior_depth[s] = True, {}, {}
        for l in range(NUM_KP):
            m = kmask_b[s, l] != 0
            if not m and "ok_all_lanes" not in alt:
                continue
            x, y, z = (float(kps_b[s, l, c]) for c in range(3))
            p = [chain3(x, T[r * 4], y, T[r * 4 + 1], z, T[r * 4 + 2]) + T[r * 4 + 3] for r in range(3)]      # kps @ R^T, then + t
            q = [chain3(p[0], K[r * 3], p[1], K[r * 3 + 1], p[2], K[r * 3 + 2]) for r in range(3)]            # kps_in_C @ K^T
            if not ((p[2] if "prior_front_on_p" in alt else q[2]) > 0.0):
                ok = False
            if m:
                prior_depth[s][l] = q[2]
                got[l] = (_div(q[0], q[2]), _div(q[1], q[2]))
        if ok:
            for l, (u0, u1) in got.items():
                with np.errstate(over="ignore"):
                    prior_uv[s, l] = np.float32(u0), np.float32(u1)                  # round to nearest
                prior_mask[s, l] = 1
    return {"out": out, "prior_uv": prior_uv, "prior_mask": prior_mask,
            "trace": {"valid": valid, "nrow": [r["n"] for r in rows], "pairs": pairs, "prior_depth": prior_depth, "prior_considered": considered,
                      "counts": counts, "best": best, "best_n": best_n}}


def _div(a, b):
    """IEEE division (Python raises on a zero divisor)."""
    if b == 0.0:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- case builders ---------------------------------------------------------------------------------------------------------------------
def _slots(rng, n, scattered):
    return np.sort(rng.choice(NUM_KP, n, replace=False)) if scattered else np.arange(n)


def empty_case(name, n_a, n_b, has_cov, rng):
    """Every buffer filled with FINITE decoys: whatever a case does not set must not be read into a result (a masked-out keypoint, a rejected crop's pose, an
    absent object's map pose) -- and would change it if it were."""
    c = {"name": name, "n_a": n_a, "n_b": n_b, "has_cov": int(has_cov), "kp_std2": 0.01 ** 2, "chi2_max": CHI2_2DOF_95, "min_inliers": 4}
    c["T_pnp"] = rng.uniform(-3, 3, (n_a, 16))
    c["accepted"] = np.zeros(n_a, np.uint8)
    c["uv"] = rng.uniform(-1, 1, (n_a, NUM_KP, 2)).astype(np.float32)
    c["cov"] = np.tile(np.array([3e-4, 1e-5, 2e-5, 2e-4], np.float32), (n_a, NUM_KP, 1)) * rng.uniform(0.5, 2, (n_a, NUM_KP, 1)).astype(np.float32)
    c["mask"] = np.zeros((n_a, NUM_KP), np.uint8)
    c["kps_a"] = rng.uniform(-60, 60, (n_a, NUM_KP, 3)).astype(np.float32)
    c["blk"] = rng.uniform(-2, 2, BLOCK)
    c["blk"][A_IN:A_IN + 16] = 0.0
    c["blk"][B_IN:B_IN + 16] = 0.0
    c["kps_b"] = rng.uniform(-60, 60, (n_b, NUM_KP, 3)).astype(np.float32)
    c["kmask_b"] = np.zeros((n_b, NUM_KP), np.uint8)
    c["K_a_double"] = np.zeros((n_a, 3, 3))
    return c


def _bbox_K(T_OtoC, pts, margin):
    pc = pts @ T_OtoC[:3, :3].T + T_OtoC[:3, 3]
    px = pc @ SS.K_YCBV.T
    px = px[:, :2] / px[:, 2:3]
    bbox = np.array([px[:, 0].min() - margin, px[:, 1].min() - margin, px[:, 0].max() + margin, px[:, 1].max() + margin])
    return SS.fix_K_for_bbox_ndc(SS.K_YCBV, bbox)


def tracking_case(name, seed, n_a, n_b, has_cov, scattered=True, n_kp=None, reject=(), unmapped=(), b_unmapped=(), **state_kw):
    """A tracking view from tests/slam_states.make_state(seed): its current view's detections as pass A's crops (float32 uv / cov / model keypoints on
    ``n_kp[j]`` slots of the 41, prefix-shaped or scattered), n_b symmetric objects of the map as pass B's.  reject / unmapped: crops whose PnP pose
    was not accepted / whose object is not in the map."""
    rng = np.random.default_rng([seed, 77])
    kw = dict(n_obj=n_a, n_views=2, use_cov=True, kp_range=(NUM_KP, NUM_KP + 1), drop_pose=0.0, drop_map=0.0, miss=0.0)
    kw.update(state_kw)
    st = SS.make_state(seed, **kw)
    view = st["view_ids"][-1]
    c = empty_case(name, n_a, n_b, has_cov, rng)
    c["kp_std2"] = float(st["manual_kp_std"]) ** 2
    if n_kp is None:
        n_kp = [int(v) for v in rng.integers(4, NUM_KP + 1, n_a)]
        n_kp[int(rng.integers(n_a))] = NUM_KP
    for j, o in enumerate(sorted(st["detections"][view])):
        d = st["detections"][view][o]
        n = n_kp[j]
        sl = _slots(rng, n, scattered and j % 3 != 2)                 # (every third crop keeps the network's prefix shape)
        c["mask"][j, sl] = 1
        c["kps_a"][j, sl] = d["model_kp"][:n].astype(np.float32)
        c["uv"][j, sl] = d["uv_pred"][:n].astype(np.float32)
        c["cov"][j, sl] = d["cov_pred"][:n].reshape(n, 4)
        c["K_a_double"][j] = SS.fix_K_for_bbox_ndc(SS.K_YCBV, d["bbox"])
        c["blk"][A_K + 9 * j:A_K + 9 * j + 9] = c["K_a_double"][j].astype(np.float32).astype(np.float64).reshape(-1)      # the float32 container
        if j not in reject:
            c["accepted"][j] = 1
            c["T_pnp"][j] = np.asarray(d["pose"]).reshape(-1)
        if j not in unmapped:
            c["blk"][A_IN + j] = 1.0
            c["blk"][A_T + 12 * j:A_T + 12 * j + 12] = np.asarray(st["obj_poses"][o], np.float64)[:3, :4].reshape(-1)
    for s in range(n_b):
        T = SS._pose(rng)
        c["kps_b"][s] = rng.uniform(-60, 60, (NUM_KP, 3)).astype(np.float32)
        m = _slots(rng, int(rng.integers(4, NUM_KP + 1)) if s else NUM_KP, scattered and s % 2 == 0)
        c["kmask_b"][s, m] = 1
        c["blk"][B_K + 9 * s:B_K + 9 * s + 9] = _bbox_K(T, c["kps_b"][s].astype(np.float64), 10.0).reshape(-1)          # (double, as the reference projects)
        c["blk"][B_T + 12 * s:B_T + 12 * s + 12] = T[:3].reshape(-1)
        if s not in b_unmapped:
            c["blk"][B_IN + s] = 1.0
    return c


def point_behind(case, s, cam, depth=-400.0):
    """Model coordinates (float32) of a point at about ``depth`` on the optical axis of camera ``cam`` ([12]) for pass-B crop s."""
    T = np.eye(4)
    T[:3] = np.asarray(cam).reshape(3, 4)
    To = np.eye(4)
    To[:3] = case["blk"][B_T + 12 * s:B_T + 12 * s + 12].reshape(3, 4)
    p = np.linalg.inv(T @ To) @ np.array([0.0, 0.0, depth, 1.0])
    return p[:3].astype(np.float32)


def reference_state(case):
    """The case's pass A as the reference's bookkeeping: (detections, obj_poses, view_id, manual_kp_std).  Crop j is object j + 1 of view 1."""
    det, poses = {}, {}
    for j in range(case["n_a"]):
        m = case["mask"][j].astype(bool)
        det[j + 1] = {"pose": case["T_pnp"][j].reshape(4, 4).copy() if case["accepted"][j] else None, "inliers": np.ones(int(m.sum()), bool), "kp_mask": m,
                      "model_kp": case["kps_a"][j][m].astype(np.float64), "uv_pred": case["uv"][j][m].astype(np.float64),
                      "cov_pred": case["cov"][j][m].reshape(-1, 2, 2).copy() if case["has_cov"] else None,
                      "K": case["blk"][A_K + 9 * j:A_K + 9 * j + 9].reshape(3, 3).copy()}
        if case["blk"][A_IN + j] != 0.0:
            T = np.eye(4)
            T[:3] = case["blk"][A_T + 12 * j:A_T + 12 * j + 12].reshape(3, 4)
            poses[j + 1] = T if j % 2 else T[:3].copy()               # ([3,4] and [4,4] both occur, as in the reference)
    return {1: det}, poses, 1, math.sqrt(case["kp_std2"])


def _copy(case, name):
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    c["name"] = name
    return c


def copy_crop(c, src, dst):
    """Crop dst becomes crop src: the same detection, PnP pose, map pose and intrinsics."""
    for k in ("T_pnp", "accepted", "uv", "cov", "mask", "kps_a", "K_a_double"):
        c[k][dst] = c[k][src]
    c["blk"][A_IN + dst] = c["blk"][A_IN + src]
    c["blk"][A_T + 12 * dst:A_T + 12 * dst + 12] = c["blk"][A_T + 12 * src:A_T + 12 * src + 12]
    c["blk"][A_K + 9 * dst:A_K + 9 * dst + 9] = c["blk"][A_K + 9 * src:A_K + 9 * src + 9]


def scramble_invalid(case, name, seed=5):
    """The same case with other decoys wherever the kernel must not look: rejected / unmapped crops' poses and detections, masked-out keypoints, rows of
    absent pass-B objects.  Its results must be the first case's, bit for bit."""
    rng = np.random.default_rng(seed)
    c = _copy(case, name)
    for j in range(c["n_a"]):
        ok_pose, in_map = c["accepted"][j] != 0, c["blk"][A_IN + j] != 0.0
        if not ok_pose:
            c["T_pnp"][j] = rng.uniform(-5, 5, 16)
        if not in_map:
            c["blk"][A_T + 12 * j:A_T + 12 * j + 12] = rng.uniform(-5, 5, 12)
        off = c["mask"][j] == 0 if (ok_pose and in_map) else np.ones(NUM_KP, bool)
        c["uv"][j][off] = rng.uniform(-1, 1, (int(off.sum()), 2)).astype(np.float32)
        c["kps_a"][j][off] = rng.uniform(-90, 90, (int(off.sum()), 3)).astype(np.float32)
        c["cov"][j][off] = rng.uniform(1e-6, 1e-3, (int(off.sum()), 4)).astype(np.float32)
        if not (ok_pose and in_map):
            c["blk"][A_K + 9 * j:A_K + 9 * j + 9] = rng.uniform(-5, 5, 9)
    for s in range(c["n_b"]):
        if c["blk"][B_IN + s] == 0.0:
            c["blk"][B_T + 12 * s:B_T + 12 * s + 12] = rng.uniform(-5, 5, 12)
            c["blk"][B_K + 9 * s:B_K + 9 * s + 9] = rng.uniform(-5, 5, 9)
            c["kps_b"][s] = rng.uniform(-90, 90, (NUM_KP, 3)).astype(np.float32)
    return c


def _search(make, want, seeds):
    """The first seed whose case satisfies ``want(case, vote_ref(case))`` -- a CPU search with the restatement, as the issue asks for the count boundaries."""
    for seed in seeds:
        c = make(seed)
        if want(c, vote_ref(c)):
            return c
    raise AssertionError("no seed in the searched range builds the case")


def exact_zero_depth_case():
    """Small integers, so every product and sum is exact under any rounding: H = identity, the map pose is a translation by (0, 0, 8), the third row of K is
    (0, 0, 1) -- the keypoint at z = -8 projects to a depth of exactly 0 and is NOT in front (z > 0, :1042); pass B's object has a model-mask keypoint there too."""
    rng = np.random.default_rng(404)
    c = empty_case("depth exactly 0", 1, 2, 0, rng)
    T = np.eye(4)
    T[2, 3] = 8.0
    K = np.array([[0.5, 0, 0], [0, 0.5, 0], [0, 0, 1.0]])
    pts = np.array([[1, 2, -8], [2, -1, -4], [-3, 1, 0], [1, 1, 8], [4, -2, 24], [-2, -2, 8], [0, 3, -6]], np.float32)
    pc = pts.astype(np.float64) + [0, 0, 8]
    c["accepted"][0], c["T_pnp"][0], c["blk"][A_IN] = 1, T.reshape(-1), 1.0
    c["blk"][A_T:A_T + 12] = T[:3].reshape(-1)
    c["blk"][A_K:A_K + 9] = K.reshape(-1)
    c["K_a_double"][0] = K
    sl = np.array([0, 3, 7, 12, 20, 33, 40])
    c["mask"][0, sl] = 1
    c["kps_a"][0, sl] = pts
    with np.errstate(divide="ignore", invalid="ignore"):
        c["uv"][0, sl] = (0.5 * pc[:, :2] / pc[:, 2:3]).astype(np.float32)
    c["uv"][0, 0] = 0.0
    for s in range(2):                                          # s = 0: the depth-0 keypoint is in the model mask (prior off); s = 1: it is not (prior stays)
        c["blk"][B_IN + s] = 1.0
        c["blk"][B_T + 12 * s:B_T + 12 * s + 12] = T[:3].reshape(-1)
        c["blk"][B_K + 9 * s:B_K + 9 * s + 9] = K.reshape(-1)
        c["kps_b"][s] = np.stack([rng.integers(-5, 6, NUM_KP), rng.integers(-5, 6, NUM_KP), rng.integers(-6, 20, NUM_KP)], 1).astype(np.float32)
        c["kps_b"][s, 5] = [3, -2, -8]
        c["kmask_b"][s, 2:30] = 1
        c["kmask_b"][s, 5] = 1 - s
    c["edge_depth"] = True
    return c


def build_cases():
    """Every case of tests/test_slam_vote_ref.py and tests/test_gpu_slam_vote.py, by name.  "oracle": False marks the cases the oracle cannot run (non-finite
    covariances: the reference asserts)."""
    cases = []
    # ---- random tracking states
    seed = 1000
    for n_a in (1, 2, 5, 8, 15, 16):
        for n_b in (1, 3, 16):
            for has_cov in (0, 1):
                seed += 1
                cases.append(tracking_case(f"random n_a={n_a} n_b={n_b} cov={has_cov}", seed, n_a, n_b, has_cov, scattered=bool(seed % 4)))
    # ---- validity combinations
    base = tracking_case("validity: rejected / unmapped / both / empty mask", 2001, 6, 3, 1, reject=(1, 3), unmapped=(2, 3), b_unmapped=(1,))
    base["mask"][4] = 0                                          # accepted, in the map, no keypoint: proposes, is not scored
    cases += [base, scramble_invalid(base, "validity: the same with other decoys")]
    none = tracking_case("no hypothesis at all", 2002, 4, 3, 1, reject=(0, 2), unmapped=(1, 3))
    cases += [none, scramble_invalid(none, "no hypothesis at all: other decoys")]
    # ---- count boundaries, searched on the CPU with the restatement
    few = lambda n, cov: (lambda s: tracking_case(f"best count exactly {n}", s, 1, 2, cov, n_kp=[n + 2], outlier_rate=0.3, noise=0.02))   # noqa: E731
    three = _search(few(3, 1), lambda c, r: r["trace"]["counts"][0] == 3, range(3000, 3200))
    four = _search(few(4, 0), lambda c, r: r["trace"]["counts"][0] == 4, range(3200, 3400))
    cases += [three, four]
    for base_, n, tag in ((three, 1, "min_inliers=1 takes a count of 3"), (four, 5, "min_inliers=5 refuses a count of 4"), (four, 1, "min_inliers=1, count 4")):
        c = _copy(base_, tag)
        c["min_inliers"] = n
        cases.append(c)
    # ---- ties
    tie = tracking_case("tie of two: the lower index wins", 4001, 4, 2, 1)
    copy_crop(tie, 1, 3)
    tie["T_pnp"][3, 3] += 1e-9                                   # another pose, the same evidence (asserted by the coverage check: equal counts)
    cases.append(tie)
    tie3 = tracking_case("tie of three", 4002, 5, 2, 0)
    copy_crop(tie3, 1, 3)
    copy_crop(tie3, 1, 4)
    cases.append(tie3)
    later = tracking_case("a later hypothesis with strictly more wins", 4003, 3, 2, 1, pnp_trans=0.0, pnp_rot=0.0)
    later["T_pnp"][0, 3] += 2.0                                  # the first hypothesis is off by 2 mm: fewer inliers than the later, exact ones
    cases.append(later)
    # ---- depth in the vote
    behind = tracking_case("vote: hypotheses that put crops behind the camera", 5001, 4, 2, 1)
    behind["T_pnp"][1] = (np.diag([1.0, -1.0, -1.0, 1.0]) @ behind["T_pnp"][1].reshape(4, 4)).reshape(-1)        # looks the other way
    P2 = behind["T_pnp"][2].reshape(4, 4).copy()
    P2[2, 3] -= P2[2, 3] - 5.0                                   # its own object straddles z = 0 under this hypothesis
    behind["T_pnp"][2] = P2.reshape(-1)
    cases.append(behind)
    skew = tracking_case("vote: third row of K not (0, 0, 1)", 5002, 2, 2, 1, n_kp=[NUM_KP, 30])
    Ps = skew["T_pnp"][0].reshape(4, 4).copy()
    Ps[2, 3] = 5.0                                               # crop 0 straddles z = 0 under its own hypothesis ...
    skew["T_pnp"][0] = Ps.reshape(-1)
    Ks = np.array([[0.01, 0.0, 0.0], [0.0, 0.01, 0.0], [0.75, -0.5, 1.0]])      # ... and the sign of its third homogeneous coordinate is not its z's
    skew["blk"][A_K:A_K + 9] = Ks.reshape(-1)
    skew["K_a_double"][0] = Ks
    m0 = skew["mask"][0] != 0
    q0 = (skew["kps_a"][0][m0].astype(np.float64) @ Ps[:3, :3].T + Ps[:3, 3]) @ Ks.T
    skew["uv"][0][m0] = (q0[:, :2] / q0[:, 2:3]).astype(np.float32)           # the detection agrees with that hypothesis wherever it projects
    cases.append(skew)
    cases.append(exact_zero_depth_case())
    # ---- depth in the priors
    pri = tracking_case("priors: depth <= 0 in and out of the model mask, unmapped, empty model mask", 6001, 3, 6, 1, b_unmapped=(2,))
    cam = vote_ref(pri)["out"][:12]
    assert vote_ref(pri)["trace"]["best"] >= 0
    for s, in_mask in ((0, True), (1, False)):
        lane = 7
        pri["kps_b"][s, lane] = point_behind(pri, s, cam)
        pri["kmask_b"][s, lane] = 1 if in_mask else 0
    pri["kmask_b"][3] = 0                                        # all-false model mask
    pri["blk"][B_K + 9 * 4 + 6:B_K + 9 * 4 + 9] = [0.004, 0.0, 1.0]          # s = 4: a keypoint with p.z > 0 whose third homogeneous coordinate is < 0
    T4 = np.eye(4)
    T4[:3] = np.asarray(cam).reshape(3, 4)
    To4 = np.eye(4)
    To4[:3] = pri["blk"][B_T + 48:B_T + 60].reshape(3, 4)
    pri["kps_b"][4, 11] = (np.linalg.inv(T4 @ To4) @ np.array([-900.0, 0.0, 1.5, 1.0]))[:3].astype(np.float32)
    pri["kmask_b"][4, 11] = 1
    cases.append(pri)
    # ---- covariances
    cv = tracking_case("covariances under the clamp, one or both; unequal off-diagonals", 7001, 4, 2, 1)
    cv["cov"][0, :, 0] = 3e-5
    cv["cov"][1, :, 3] = 1e-6
    cv["cov"][2, :, 0] = 2e-5
    cv["cov"][2, :, 3] = 8e-5
    cv["cov"][3, :, 1] *= 1.5
    cv["cov"][3, :, 2] *= 0.25
    cases.append(cv)
    cases.append(tracking_case("tiny_cov state", 7002, 5, 2, 1, tiny_cov=True))
    corr = tracking_case("strongly correlated covariances", 7003, 4, 2, 1)
    corr["cov"][:, :, 1] = corr["cov"][:, :, 2] = (0.9 * np.sqrt(corr["cov"][:, :, 0] * corr["cov"][:, :, 3])).astype(np.float32)
    cases.append(corr)
    # ---- the NaN flag (non-finite VALUES only)
    for tag, entries in (("whole covariance", (0, 1, 2, 3)), ("diagonal entry", (0,)), ("off-diagonal entry", (2,))):
        c = tracking_case(f"NaN {tag} on a valid keypoint of a scored crop", 8001, 3, 2, 1)
        lane = int(np.flatnonzero(c["mask"][1])[2])
        c["cov"][1, lane, list(entries)] = np.nan
        c["oracle"] = False
        cases.append(c)
    c = tracking_case("NaN on a masked-out keypoint", 8001, 3, 2, 1)
    c["cov"][1][c["mask"][1] == 0] = np.nan
    cases.append(c)
    c = tracking_case("NaN on an unscored crop", 8001, 3, 2, 1, reject=(1,))
    c["cov"][1] = np.nan
    cases.append(c)
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return cases
