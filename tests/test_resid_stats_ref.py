"""Pins tests/resid_stats_ref.py, the reference the GPU tests of suo_residual_statistics compare with (no GPU needed): its per-edge leverages and residual
covariances against the full stacked hat matrix -- a second, independent derivation --, sum lev = n, the NaN rules on the designed graphs, and the condition on the
inputs that keeps the no-redundancy rule away from rounding."""
import numpy as np
import pytest

from tests import resid_stats_cases as RK


@pytest.mark.parametrize("name", RK.NAMES)
def test_leverages_and_residual_covariances_are_the_blocks_of_the_stacked_hat_matrix(name):
    g, ref, st = RK.case(name)
    A, W = st["A"], st["W"]
    m2, n = A.shape
    assert n == st["summary"][1] and m2 == 2 * st["summary"][0]
    k = np.flatnonzero(st["counted"])
    if m2 == 0:
        return
    Sigma = np.linalg.inv(A.T @ W @ A)
    hat = A @ Sigma @ A.T @ W
    Qvv = np.linalg.inv(W) - A @ Sigma @ A.T
    scale = np.abs(np.linalg.inv(W)).max()
    for row, e in enumerate(k):
        b = slice(2 * row, 2 * row + 2)
        i = g["edge_info"][e]
        Om = np.array([[i[0], i[1]], [i[1], i[2]]])
        P = np.array([[st["edge_pcov"][e, 0], st["edge_pcov"][e, 1]], [st["edge_pcov"][e, 1], st["edge_pcov"][e, 2]]])
        assert abs(np.trace(hat[b, b]) - st["edge_lev"][e]) <= 1e-7, (name, e)
        assert np.abs(Qvv[b, b] - (np.linalg.inv(Om) - P)).max() <= 1e-7 * scale, (name, e)
        assert -1e-7 <= st["edge_lev"][e] <= 2 + 1e-7, (name, e, "0 <= lev <= 2 on a counted edge")
    # sum lev = n = tr(Sigma H), on every case
    assert abs(st["summary"][3] - n) <= 1e-6 * max(n, 1), (name, st["summary"][3], n)
    assert st["summary"][4] == m2 - n


@pytest.mark.parametrize("name", RK.NAMES)
def test_no_input_sits_where_rounding_could_flip_the_no_redundancy_rule(name):
    g, ref, st = RK.case(name)
    assert ref["cond"] <= 1e9, (name, ref["cond"])
    n_cut = RK.far_from_the_threshold(name, g, st)
    assert st["status"][3] == n_cut == (3 if name == "three_edges" else 0)


def test_the_designed_graphs_show_what_they_were_designed_for():
    g, _, st = RK.case("three_edges")
    cut = RK.designed("three_edges", g)
    assert cut.sum() == 3 and np.isnan(st["edge_t"][cut]).all() and np.isfinite(st["edge_lev"][cut]).all() and np.allclose(st["edge_lev"][cut], 2.0, atol=1e-6)
    assert np.isfinite(st["edge_t"][~cut]).all() and list(st["status"]) == [0, 0, 0, 3]
    g, _, st = RK.case("flagged_3x2")
    out = g["edge_inlier"] == 0
    assert out.sum() >= 5 and np.isfinite(st["edge_t"]).all() and (st["edge_t"][out] < st["edge_chi2"][out]).all(), "outside the estimate: Omega^-1 + P"
    assert (st["edge_t"][~out] > st["edge_chi2"][~out]).all(), "inside the estimate: Omega^-1 - P"
    for name, o, status in (("object_out_frame", 2, [0, 1]), ("object_out_3x2", 1, [0, 1]), ("object_out_3x17m", 16, [0, 1])):
        g, _, st = RK.case(name)
        hit = g["edge_obj"] == o
        assert list(st["status"]) == status + [int(hit.sum()), 0] and np.isnan(st["edge_t"][hit]).all() and np.isnan(st["edge_pcov"][hit]).all()
        assert np.isfinite(st["edge_chi2"]).all() and np.isfinite(st["edge_t"][~hit]).all() and np.isfinite(st["summary"]).all()
    g, _, st = RK.case("fixed_pair_3x2")
    both = (g["edge_cam"] == 0) & (g["edge_obj"] == 1)
    assert both.sum() >= 4 and not st["edge_pcov"][both].any() and np.allclose(st["edge_t"][both], st["edge_chi2"][both], rtol=1e-12)
    assert not st["counted"][both].any()
    g, _, st = RK.case("no_edges")
    assert np.array_equal(st["summary"][:5], np.zeros(5)) and np.isnan(st["summary"][5]) and list(st["status"]) == [0, 2, 0, 0]
    g, _, st = RK.case("1x1_4edges")
    assert st["summary"][4] == 2
