"""The frame chain's own two kernels, fg_prep_kernel and fg_build_kernel (csrc/frame_geom.hip), at the edges of the rules they restate: the designed cases of
tests/frame_geom_cases.py, the staged pose graph read back through suo_debug_frame_geom_staged and held against the mp restatement tests/frame_geom_ref.py
(lib/object_slam.py:34-36, :825-828, :1118-1165) -- bit for bit where the arithmetic is exact (compaction, widening, slots, counts, the graph's header),
within bounds derived from the arithmetic where it rounds:

    ys          |err| <= 3 * 2^-53 * (|u k0| + |v k1| + |k2|)          two products, one sum, one offset; holds with or without contraction
    ixx, iyy    relative error <= 4 * 2^-53                            products of two float32 are exact in fp64: det rounds once, one division follows
    ixy         |err| <= 4 * 2^-53 * (|b| + |c|) / (2 |det|)           two divisions, one sum, an exact halving

Worst observed ratios to these bounds on the MI355X (every case of this file): ys 0.464, ixx / iyy 0.431, ixy 0.426.

Then the acceptance rule one ulp either side of equality, the limits of the one-wave LM form (656 edges; 9 objects = the first 4-lane frame; an empty frame inside
a launch) against oracle.geometry.optimize on the staged graph, independence from the stale slots of a reused context, the device-resident sampler key, and the
singular-covariance rule of include/suo_hip.h (suo_frame_geom_launch)."""
import mpmath as mp
import numpy as np
import pytest
import torch

from oracle import geometry as G
from suo_slam_amd.frame_geom import FrameGeometry, kbbox_terms
from tests import frame_geom_cases as Cs
from tests import frame_geom_ref as R

pytestmark = pytest.mark.gpu

CHI2_THR = 5.991
OUT_KEYS = ("T_pnp", "T_opt", "pnp_status", "pnp_best_inliers", "pnp_iterations", "n_kp", "accepted", "inlier", "mask", "uv", "cov", "lm_stats", "pair_start",
            "pair_end", "obj_fixed", "header")
SLOT_KEYS = ("xs", "ys", "edge_uv", "edge_k", "edge_info")
WORST = {"ys": 0.0, "ixx/iyy": 0.0, "ixy": 0.0}


def _launch(fg, frames, seed, use_cov=True, do_lm=True, min_depth=None, seed_dev=None):
    first, cat = Cs.concat(frames)
    dev = [torch.from_numpy(np.ascontiguousarray(cat[k])).cuda() for k in ("uv", "cov", "mask", "kps")]
    kinv, camk = kbbox_terms(cat["K_bbox"])
    md = cat["min_depth"] if min_depth is None else np.asarray(min_depth, np.float64)
    fg.launch(first, *dev, kinv, camk, md, seed=seed, use_cov=use_cov, do_lm=do_lm, seed_dev=seed_dev)
    r = fg.fetch()
    r.update(fg.staged())
    r.update(first=first, cat=cat, kinv=kinv, camk=camk, min_depth=md)
    return r


def _bits_equal(a, b, keys=OUT_KEYS + SLOT_KEYS + ("chi2",)):
    """Every fetched / staged array equal bit for bit over the VALID slots: the first n_kp of a crop (chi2: of an accepted crop)."""
    assert np.array_equal(a["n_kp"], b["n_kp"]) and np.array_equal(a["accepted"], b["accepted"])
    for key in keys:
        x, y = a[key], b[key]
        if key in SLOT_KEYS or key == "chi2":
            for l in range(len(a["n_kp"])):
                n = int(a["n_kp"][l]) if key != "chi2" or a["accepted"][l] else 0
                assert x[l, :n].tobytes() == y[l, :n].tobytes(), (key, l)
        else:
            assert x.tobytes() == y.tobytes(), key


def _check_staging(r, use_cov=True, lm=True):
    """The launch's staged graph and decisions against the mp restatement."""
    cat, first = r["cat"], r["first"]
    ref = R.stage(cat["uv"], cat["cov"], cat["mask"], cat["kps"], r["kinv"], r["camk"], use_cov)
    L = len(cat["mask"])
    assert np.array_equal(r["n_kp"], ref["n"]) and np.array_equal(r["mask"], ref["valid"])
    assert np.array_equal(r["uv"], cat["uv"]) and r["cov"].tobytes() == cat["cov"].tobytes()
    acc = R.accept(ref["n"], r["pnp_status"], r["T_pnp"], r["min_depth"])
    assert np.array_equal(r["accepted"], acc)
    assert np.array_equal(r["pnp_status"][ref["n"] < 4], np.ones(int((ref["n"] < 4).sum()), np.int32))
    ps, pe, fx, hdr = R.graph(first, ref["n"], acc)
    assert np.array_equal(r["pair_start"], ps) and np.array_equal(r["pair_end"], pe) and np.array_equal(r["obj_fixed"], fx)
    assert np.array_equal(r["header"], hdr)
    with mp.workdps(R.DPS):
        for l in range(L):
            n = int(ref["n"][l])
            for key in ("xs", "edge_uv", "edge_k"):                                  # exact: widening and copies
                assert r[key][l, :n].tobytes() == ref[key][l, :n].tobytes(), (key, l)
            for j in range(n):
                for t in range(2):
                    err = abs(mp.mpf(float(r["ys"][l, j, t])) - ref["ys"][l][j][t])
                    WORST["ys"] = max(WORST["ys"], float(err / ref["ys_bound"][l][j][t]))
                    assert err <= ref["ys_bound"][l][j][t], ("ys", l, j, t)
                got, want = r["edge_info"][l, j], ref["info"][l][j]
                if not use_cov:
                    assert got.tobytes() == np.array([1.0, 0.0, 1.0]).tobytes()
                    continue
                for t in (0, 2):
                    rel = abs(mp.mpf(float(got[t])) - want[t]) / abs(want[t])
                    WORST["ixx/iyy"] = max(WORST["ixx/iyy"], float(rel / (4 * R.U)))
                    assert rel <= 4 * R.U, ("info", l, j, t)
                err, bound = abs(mp.mpf(float(got[1])) - want[1]), ref["ixy_bound"][l][j]
                if bound > 0:
                    WORST["ixy"] = max(WORST["ixy"], float(err / bound))
                assert err <= bound, ("ixy", l, j)
    if lm:
        _check_slots_are_in_mask_order(r, ref)
    # inlier flags beyond a crop's edges, and every flag of a crop without edges, are reset to 1 by each launch
    for l in range(L):
        assert r["inlier"][l, (int(ref["n"][l]) if acc[l] else 0):].all()
    print("worst ratio to the derived bounds so far:", {k: round(v, 3) for k, v in WORST.items()})
    return ref


def _check_slots_are_in_mask_order(r, ref):
    """chi2 / inlier slot j of an accepted crop belong to its j-th valid keypoint: chi2 recomputed in fp64 from the refined pose, the staged measurement and the
    mp information.  Tolerance: some fifty fp64 roundings on quantities of at most a few tens (K_bbox entries times a ratio <= 1) leave the residual e with an
    absolute error delta < 1e-12, hence |d chi2| <= |I|_1 (2 |e|_1 delta + delta^2) -- orders below what the neighbouring keypoint's residual would give."""
    delta = 1e-12
    for l in np.nonzero(r["accepted"])[0]:
        n = int(ref["n"][l])
        T = r["T_opt"][l]
        pc = ref["xs"][l, :n] @ T[:, :3].T + T[:, 3]
        k = ref["edge_k"][l, :n]
        e = ref["edge_uv"][l, :n] - np.stack([k[:, 0] * pc[:, 0] / pc[:, 2] + k[:, 2], k[:, 1] * pc[:, 1] / pc[:, 2] + k[:, 3]], 1)
        I = np.array([[float(x) for x in ref["info"][l][j]] for j in range(n)])
        chi2 = e[:, 0] * (I[:, 0] * e[:, 0] + I[:, 1] * e[:, 1]) + e[:, 1] * (I[:, 1] * e[:, 0] + I[:, 2] * e[:, 1])
        tol = (np.abs(I[:, 0]) + 2 * np.abs(I[:, 1]) + np.abs(I[:, 2])) * (2 * np.abs(e).sum(1) * delta + delta * delta) + 1e-13 * np.abs(chi2)
        assert (np.abs(r["chi2"][l, :n] - chi2) <= tol).all(), (l, np.abs(r["chi2"][l, :n] - chi2) / tol)
        away = np.abs(chi2 - CHI2_THR) > 1e-5 * CHI2_THR
        assert np.array_equal(r["inlier"][l, :n][away], (chi2 <= CHI2_THR)[away])


# ---- staging --------------------------------------------------------------------------------------------------------------------------------------------------
def test_mask_cases_are_compacted_in_mask_order():
    import ctypes as C
    from suo_slam_amd import _lib
    f = Cs.mask_frame()
    fg = FrameGeometry(16, 1)
    r = _launch(fg, [f], seed=3)
    _check_staging(r)
    assert tuple(r["n_kp"]) == Cs.MASK_COUNTS
    row = Cs.MASK_ROWS.index("bytes 2 / 255")
    assert r["mask"][row].all() and r["n_kp"][row] == 41
    res = _lib.FrameGeomResult()                                           # the bytes themselves: 1 for a counted keypoint whatever the input byte was
    _lib.check(_lib.lib().suo_frame_geom_fetch(fg._h, C.byref(res)), "suo_frame_geom_fetch")
    raw = np.ctypeslib.as_array(C.cast(res.mask, C.POINTER(C.c_uint8)), shape=(len(Cs.MASK_ROWS), 41))
    assert np.array_equal(raw, (f["mask"] != 0).astype(np.uint8)) and (raw[row] == 1).all()
    for row, n in zip(range(len(Cs.MASK_ROWS)), Cs.MASK_COUNTS):
        if n < 4:
            assert r["pnp_status"][row] == 1 and not r["accepted"][row]
    for row in (Cs.MASK_ROWS.index("count 4"), Cs.MASK_ROWS.index("count 5")):      # exact measurements (mask_frame): PnP has its inliers
        assert r["pnp_status"][row] == 0 and r["accepted"][row]


@pytest.mark.parametrize("name", ["1", "8", "9", "16", "16 x 41", "[0, 3, 3, 8]"])
def test_staged_graph_of_every_frame_shape(name):
    frames = Cs.shape_frames()[name]
    r = _launch(FrameGeometry(16, 3), frames, seed=5)
    _check_staging(r)
    assert len(r["header"]) == len(frames) and r["header"][:, 1].tolist() == [len(f["mask"]) for f in frames]


@pytest.mark.parametrize("use_cov", [True, False])
def test_designed_covariances_against_the_mp_inverse(use_cov):
    f, where = Cs.cov_frame()
    r = _launch(FrameGeometry(16, 1), [f], seed=5, use_cov=use_cov)
    ref = _check_staging(r, use_cov=use_cov)
    for name, (crop, slot) in where.items():
        assert r["mask"][crop, slot]
    if use_cov:                                                           # the designed matrices did reach the staged graph
        crop, slot = where["scaled 1e-12"]
        assert r["edge_info"][crop, ref["idx"][crop].index(slot), 0] > 1e15


# ---- acceptance -----------------------------------------------------------------------------------------------------------------------------------------------
def test_acceptance_at_equality_and_one_ulp_either_side():
    """min_depth = T_pnp[2,3] exactly: rejected (the rule is >); the next double below: accepted; the next above: rejected.  Crop 1 keeps 3 keypoints (status 1,
    rejected whatever min_depth), crop 2 keeps 4 with exact measurements (accepted)."""
    f = Cs.frame(39, 9)
    for crop, cnt in ((1, 3), (2, 4)):
        keep = np.nonzero(f["mask"][crop])[0][:cnt]
        f["mask"][crop] = 0
        f["mask"][crop, keep] = 1
    Cs.exact_uv(f, 2)
    fg = FrameGeometry(16, 1)
    r0 = _launch(fg, [f], seed=9, min_depth=np.zeros(9))
    z = r0["T_pnp"][:, 2, 3].copy()
    solved = r0["pnp_status"] == 0
    assert r0["pnp_status"][1] == 1 and r0["n_kp"][1] == 3 and r0["n_kp"][2] == 4 and solved[2] and solved.sum() == 8 and (z[solved] > 0).all()
    assert np.array_equal(r0["accepted"], solved)
    for md, expect in ((z, False), (np.nextafter(z, -np.inf), True), (np.nextafter(z, np.inf), False)):
        r = _launch(fg, [f], seed=9, min_depth=md)
        _check_staging(r)
        for key in ("T_pnp", "pnp_status", "pnp_best_inliers", "pnp_iterations", "n_kp"):
            assert r[key].tobytes() == r0[key].tobytes(), key
        assert np.array_equal(r["accepted"], solved & expect)
        for l in np.nonzero(~r["accepted"])[0]:
            assert r["T_opt"][l].tobytes() == r["T_pnp"][l, :3].tobytes() and r["pair_end"][l] == r["pair_start"][l] and r["inlier"][l].all() and r["obj_fixed"][l]
        assert r["header"][0, 2] == (r["n_kp"][solved].sum() if expect else 0)
        if not expect:
            assert (r["lm_stats"] == 0).all()
    # and the 3-keypoint crop against a min_depth nothing could fail
    r = _launch(fg, [f], seed=9, min_depth=np.full(9, -1e300))
    assert not r["accepted"][1] and r["pnp_status"][1] == 1 and r["accepted"][2] and np.array_equal(r["T_pnp"][1], np.eye(4))


# ---- limits of the LM form ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,seed", Cs.LM_LIMIT_SEEDS)
def test_lm_limit_frames_meet_the_oracle_on_the_staged_graph(name, seed):
    """16 crops x 41 keypoints = 656 edges (LF2_MAX_EDGES, 62 976 bytes of LDS, level bits up to 10 at four lanes per object) and 9 objects (the first frame of
    the 4-lane body): oracle.geometry.optimize on the graph the chain staged.  Flags within 1e-5 thr of the gate are skipped, at most 1 % of the frame."""
    f = Cs.shape_frames()[name][0]
    r = _launch(FrameGeometry(16, 1), [f], seed=seed)
    _check_staging(r)
    objs = np.nonzero(r["accepted"])[0]
    n = r["n_kp"]
    if name == "16 x 41":
        assert r["accepted"].all() and r["header"][0].tolist() == [1, 16, 656, 16] and (n == 41).all()
    else:
        assert len(f["mask"]) == 9 and len(objs) >= 8
    e_obj = np.concatenate([np.full(int(n[l]), i, np.int32) for i, l in enumerate(objs)])
    cat = lambda key: np.concatenate([r[key][l, :n[l]] for l in objs])
    o = G.optimize(np.eye(4)[None, :3], np.array([1], np.uint8), r["T_pnp"][objs][:, :3], np.zeros(len(objs), np.uint8), np.zeros(len(e_obj), np.int32), e_obj,
                   cat("edge_k"), cat("xs"), cat("edge_uv"), cat("edge_info"), np.ones(len(e_obj), np.uint8))
    np.testing.assert_allclose(r["T_opt"][objs], o[1], rtol=0, atol=1e-6 * np.abs(o[1]).max())
    near = np.abs(o[3] - CHI2_THR) <= 1e-5 * CHI2_THR
    print(f"{name}: {int(near.sum())} of {len(e_obj)} flags within 1e-5 of the chi2 gate skipped")
    assert near.sum() <= 0.01 * len(e_obj)
    assert np.array_equal(cat("inlier")[~near], o[2].astype(bool)[~near])
    assert r["lm_stats"][0, 0] == o[4][0] and r["lm_stats"][0, 1] > 0 and abs(int(r["lm_stats"][0, 3]) - int(o[4][3])) <= int(near.sum())


def test_empty_frame_inside_a_launch():
    frames = Cs.shape_frames()["[0, 3, 3, 8]"]
    r = _launch(FrameGeometry(16, 3), frames, seed=5)
    _check_staging(r)
    assert r["lm_stats"].shape == (3, 4) and (r["lm_stats"][1] == 0).all() and r["header"][1].tolist() == [1, 0, 0, 0]
    assert (r["lm_stats"][[0, 2], 1] > 0).all()
    one, seed, g0 = FrameGeometry(16, 1), 5, 0
    for i in (0, 2):
        r1 = _launch(one, [frames[i]], seed=seed)
        L = len(frames[i]["mask"])
        for key in OUT_KEYS + SLOT_KEYS + ("chi2",):
            if key in ("lm_stats", "header"):
                assert r[key][i].tobytes() == r1[key][0].tobytes(), key
            elif key in SLOT_KEYS or key == "chi2":
                for l in range(L):
                    m = int(r1["n_kp"][l]) if key != "chi2" or r1["accepted"][l] else 0
                    assert r[key][g0 + l, :m].tobytes() == r1[key][l, :m].tobytes(), (key, l)
            else:
                assert r[key][g0:g0 + L].tobytes() == r1[key].tobytes(), key
        seed += int(np.count_nonzero(r1["n_kp"] >= 4))
        g0 += L


# ---- stale slots ----------------------------------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_what_an_earlier_launch_left_in_the_slots():
    dense, sparse = Cs.shape_frames()["16 x 41"][0], Cs.frame(61, 16, drop=0.5)
    used = FrameGeometry(16, 1)
    d = _launch(used, [dense], seed=2)
    a = _launch(used, [sparse], seed=4)
    b = _launch(FrameGeometry(16, 1), [sparse], seed=4)
    assert (a["n_kp"] < 41).all() and a["accepted"].sum() >= 8
    _bits_equal(a, b)
    # the premise: behind the valid slots the reused context does hold the dense frame's values, the fresh one zeros
    l = int(np.argmin(a["n_kp"]))
    n = int(a["n_kp"][l])
    assert a["xs"][l, n:].tobytes() == d["xs"][l, n:].tobytes() and not b["xs"][l, n:].any() and a["xs"][l, n:].any()


# ---- the device-resident sampler key ----------------------------------------------------------------------------------------------------------------------------
def test_seed_dev_adds_to_the_seed_and_advances_by_the_solvable_crops():
    """Crop 0 of frame 0 keeps 2 keypoints (not solvable), crop 1 is solvable but too close (rejected): the key advances by the crops with >= 4 keypoints,
    accepted or not, summed over the launch's frames."""
    frames = [Cs.frame(71, 4), Cs.frame(72, 0), Cs.frame(73, 5)]
    frames[0]["mask"][0, np.nonzero(frames[0]["mask"][0])[0][2:]] = 0
    frames[0]["min_depth"][1] = 1e9
    s, k = 1234, 77
    fg = FrameGeometry(16, 3)
    key = torch.tensor([k], dtype=torch.int64, device="cuda")
    a = _launch(fg, frames, seed=s, seed_dev=key)
    after = int(key.cpu().item())
    b = _launch(fg, frames, seed=s + k)
    _bits_equal(a, b)
    solvable = int(np.count_nonzero(a["n_kp"] >= 4))
    assert a["n_kp"][0] == 2 and a["pnp_status"][1] == 0 and not a["accepted"][1] and solvable == 8 and a["accepted"].sum() < solvable
    assert after == k + solvable
    c = _launch(fg, frames, seed=s)                                        # (the key did matter)
    assert c["T_pnp"].tobytes() != a["T_pnp"].tobytes()


# ---- singular covariances -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Cs.degenerate_covs()))
def test_a_keypoint_without_an_invertible_covariance_is_masked_out(name):
    f, g, crop, slot = Cs.singular_frames()[name]
    fg = FrameGeometry(16, 1)
    a = _launch(fg, [f], seed=5)
    b = _launch(fg, [g], seed=5)
    assert not a["mask"][crop, slot] and a["n_kp"][crop] == f["mask"][crop].sum() - 1
    _bits_equal(a, b, keys=tuple(k for k in OUT_KEYS + SLOT_KEYS + ("chi2",) if k != "cov"))
    assert a["accepted"].sum() >= 8 and a["accepted"][crop] and (a["lm_stats"][0, :3] > 0).all()
    assert np.isfinite(a["T_pnp"]).all() and np.isfinite(a["T_opt"]).all()
    for l in np.nonzero(a["accepted"])[0]:
        n = int(a["n_kp"][l])
        assert np.isfinite(a["chi2"][l, :n]).all() and np.isfinite(a["edge_info"][l, :n]).all() and np.isfinite(a["ys"][l, :n]).all()
    _check_staging(a)
    # without the network covariance the matrix is not looked at: the keypoint stays
    c = _launch(fg, [f], seed=5, use_cov=False)
    assert c["mask"][crop, slot] and c["n_kp"][crop] == f["mask"][crop].sum() and np.isfinite(c["T_opt"]).all()
    _check_staging(c, use_cov=False)


def test_a_singular_covariance_takes_a_crop_from_four_keypoints_to_three():
    f, g, crop, slot = Cs.four_to_three_frame()
    fg = FrameGeometry(16, 1)
    a = _launch(fg, [f], seed=5)
    b = _launch(fg, [g], seed=5)
    assert b["n_kp"][crop] == 4 and b["pnp_status"][crop] == 0 and b["accepted"][crop]
    assert a["n_kp"][crop] == 3 and a["pnp_status"][crop] == 1 and not a["accepted"][crop] and not a["mask"][crop, slot]
    assert a["T_opt"][crop].tobytes() == np.eye(4)[:3].tobytes() and a["pair_end"][crop] == a["pair_start"][crop]
    assert np.isfinite(a["T_opt"]).all() and a["accepted"].sum() == b["accepted"].sum() - 1
    _check_staging(a)
    # the crops in front of it keep their sampler keys, hence their PnP bits
    assert a["T_pnp"][:crop].tobytes() == b["T_pnp"][:crop].tobytes()
