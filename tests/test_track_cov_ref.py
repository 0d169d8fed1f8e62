"""The numpy restatement of the tracking covariances (tests/track_cov_ref.py) is tied to the estimator the project runs, not only to itself: a Monte-Carlo run of
the oracle LM in curr_only form against maps drawn from Sigma_OO must have the covariance the restatement states (CPU only)."""
import functools

import numpy as np

from oracle import geometry as G
from tests import pose_cov_cases as PC
from tests import pose_cov_ref as R
from tests import track_cov_cases as TC
from tests import track_cov_ref as TR


@functools.lru_cache(maxsize=None)
def _cpu_monte_carlo():
    """the 4096 repetitions through oracle.geometry.optimize, started from the true camera; computed once"""
    g = TC.mc_setup()["g"]
    obj_T, d_obj, uv = TC.mc_draws()
    hat = np.zeros((TC.MC_N, 3, 4))
    for n in range(TC.MC_N):
        a = dict(g, obj_T=obj_T[n], edge_uv=uv[n])
        hat[n] = G.optimize(*PC.args(a), **TC.OPT_KW)[0][0]
    return TC.mc_gates(TC.mc_errors(hat), d_obj)


def test_monte_carlo_covariance_of_the_tracked_camera_is_the_consider_covariance():
    """Observed with default_rng(4): whitened eigenvalues under P_c 0.943 .. 1.044, inside the unwidened sampling band [0.925, 1.078]; under Hcc^-1 the smallest
    is 5.8."""
    m = _cpu_monte_carlo()
    print("whitened by P_c:", m["eig_consider"], "band", TC.MC_BAND, "gate", TC.MC_GATE)
    print("whitened by Hcc^-1:", m["eig_fixed_map"])
    assert TC.MC_GATE[0] <= m["eig_consider"].min() and m["eig_consider"].max() <= TC.MC_GATE[1]
    assert m["eig_fixed_map"].min() >= 2.0


def test_monte_carlo_cross_moment_has_the_reported_sign():
    m = _cpu_monte_carlo()
    print("cross: relative Frobenius error", m["cross_err"], "with the sign flipped", m["cross_err_flipped"])
    assert m["cross_err"] < 0.5
    assert m["cross_err_flipped"] > 1.5


def test_fixed_map_below_full_graph_marginal_below_consider_covariance():
    s = TC.mc_setup()
    full = R.covariances(s["full"])["cam_cov"][4]
    lo, hi = s["ref"]["fixed_map_cov"][0], s["ref"]["cam_cov"][0]
    scale = np.linalg.eigvalsh(hi).max()
    d1, d2 = np.linalg.eigvalsh(full - lo).min(), np.linalg.eigvalsh(hi - full).min()
    print("min eig(full - fixed_map) / lambda_max", d1 / scale, " min eig(consider - full) / lambda_max", d2 / scale)
    assert d1 >= -1e-9 * scale
    assert d2 >= -1e-9 * scale


def test_restatement_reads_the_upper_triangle_and_leaves_out_objects_marked_nan():
    g, Sigma, ref = TC.case(2)
    low = Sigma.copy()
    low[np.tril_indices(len(low), -1)] = 1e30
    again = TR.tracking(g, low)
    for k in ("cam_cov", "fixed_map_cov", "cross", "rel"):
        assert np.array_equal(again[k], ref[k], equal_nan=True), k
    zero = TR.tracking(g, np.zeros_like(Sigma))
    assert np.abs(zero["cam_cov"][:2] - zero["fixed_map_cov"][:2]).max() <= 1e-12 * np.abs(zero["fixed_map_cov"][0]).max()      # (inv is symmetric to rounding only)
    assert not np.nan_to_num(zero["cross"]).any()
    # object 1 marked NaN = the same graph without object 1's edges
    marked = Sigma.copy()
    marked[6:, 6:] = np.nan
    without = dict(g, edge_inlier=np.where(g["edge_obj"] == 1, 0, g["edge_inlier"]).astype(np.uint8))
    a, b = TR.tracking(g, marked), TR.tracking(without, Sigma)
    assert list(a["status"]) == [ref["status"][0], 1]
    assert np.isnan(a["cross"][0, 1]).all() and np.isnan(a["rel"][0, 1]).all()
    zeroed = TR.tracking(without, np.where(np.isnan(marked), 0.0, marked))
    assert np.abs(a["cam_cov"][0] - zeroed["cam_cov"][0]).max() <= 1e-12 * np.abs(zeroed["cam_cov"][0]).max()
    assert np.array_equal(a["fixed_map_cov"], b["fixed_map_cov"], equal_nan=True)


def test_cases_cover_what_the_kernel_can_get_wrong():
    for n_obj in TC.SIZES:
        g, Sigma, ref = TC.case(n_obj)
        assert list(g["cam_fixed"]) == [0, 1, 0] and list(ref["status"]) == [1, 0]
        assert np.isnan(ref["cam_cov"][2]).all() and not ref["cam_cov"][1].any() and np.isfinite(ref["cam_cov"][0]).all()
        e0 = g["edge_obj"][g["edge_cam"] == 0]
        assert (g["edge_inlier"][g["edge_cam"] == 0] == 0).any()
        if n_obj >= 2:
            assert n_obj - 1 not in e0 and np.abs(ref["cross"][0, n_obj - 1]).max() > 0           # unseen, yet correlated through the map
        if n_obj > 2:
            assert (np.diff(e0) < 0).any()                                                       # not sorted by object
        assert np.abs(ref["rel"][1] - ref["rel"][1].transpose(0, 2, 1)).max() == 0


def test_extrapolated_jacobians_are_those_of_the_pose_covariance_reference():
    """the restatement's Jacobians against pose_cov_ref.edge_jacobians (one step of 1e-6: 2e-10 of rounding relative to the largest entry, asked for at 1e-8)"""
    g, _, _ = TC.case(16)
    for e in range(0, len(g["edge_cam"]), 7):
        for a, b in zip(TR.edge_jacobians(g, e), R.edge_jacobians(g, e)):
            assert np.abs(a - b).max() <= 1e-8 * np.abs(b).max(), e
