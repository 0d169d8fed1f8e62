"""The pair reference (tests/pose_cov_pairs_ref.py) against what it must reproduce, on the CPU: its finite-difference Jacobians equal the adjoint formulas the
header states, and both kinds of relative covariance do not depend on which camera is fixed -- while a marginal block does, so the invariance test can fail."""
import numpy as np

from tests import pose_cov_cases as K
from tests import pose_cov_pair_cases as PK
from tests import pose_cov_pairs_ref as PR
from tests import pose_cov_ref as R


def test_log_inverts_exp():
    rng = np.random.default_rng(0)
    for scale in (1e-6, 1e-2, 1.0):
        u = rng.normal(size=6) * scale
        assert np.abs(PR.log_se3(R.exp_se3(u)) - u).max() <= 1e-12 * max(scale, 1e-3)


def test_finite_difference_jacobians_equal_the_adjoint_formulas():
    g, _ = K.case("3x2")
    C = len(g["cam_T"])
    for c in range(C):
        Tc = R.to4(g["cam_T"][c])
        for o in range(len(g["obj_T"])):
            To = R.to4(g["obj_T"][o])
            J = PR.relative_jacobian(Tc, To, True, False)
            assert np.abs(J - np.hstack([np.eye(6), PR.adjoint(Tc)])).max() <= 1e-9
            J = PR.relative_jacobian(To, Tc, False, True)                      # the same pair named object first
            assert np.abs(J - np.hstack([PR.adjoint(Tc), np.eye(6)])).max() <= 1e-9
    Ta, Tb = R.to4(g["obj_T"][0]), R.to4(g["obj_T"][1])
    B = PR.adjoint(np.linalg.inv(Tb))
    assert np.abs(PR.relative_jacobian(Ta, Tb, False, False) - np.hstack([B, -B])).max() <= 1e-9
    # a camera away from the identity (3x2's are within 0.25 rad and 15 cm of it)
    J = PR.relative_jacobian(PK.MOVED, Ta, True, False)
    assert np.abs(J - np.hstack([np.eye(6), PR.adjoint(PK.MOVED)])).max() <= 1e-9


def test_relative_covariances_do_not_depend_on_the_gauge_and_a_marginal_does():
    g0, ref0 = K.case("3x2")
    g1 = {k: v.copy() for k, v in g0.items()}
    g1["cam_fixed"] = np.array([0, 1, 0], np.uint8)
    ref1 = R.covariances(g1)
    pairs = PK.pairs_of(g0, [(0, 1), (1, 0)])
    _, rel0, n0 = PR.relative(g0, ref0, pairs)
    _, rel1, n1 = PR.relative(g1, ref1, pairs)
    assert n0 == 0 and n1 == 0
    tol = R.bound(ref0) + R.bound(ref1)
    diff = np.abs(rel0 - rel1).reshape(len(pairs), -1).max(1)
    n_co = len(g0["cam_T"]) * len(g0["obj_T"])
    print(f"gauge difference: camera-object {diff[:n_co].max():.3e}  object-object {diff[n_co:].max():.3e}  sum of the bounds {tol:.3e}")
    assert diff.max() <= tol, (diff, tol)
    marginal = float(np.abs(ref0["obj_cov"][0] - ref1["obj_cov"][0]).max())
    assert marginal > 1e3 * tol, (marginal, tol)


def test_a_fixed_vertex_contributes_zeros_and_a_missing_one_nans():
    g, pairs, ref, (cross, rel, n_nan) = PK.case("moved_cam_only")
    assert n_nan == 0
    for q, (a, b) in enumerate(pairs):
        assert not cross[q].any()
        if a == 0:
            assert np.abs(rel[q] - ref["cam_cov"][0]).max() <= 1e-9 * np.abs(ref["cam_cov"][0]).max()     # a free camera and a fixed object: Sigma_cc
        else:
            assert not rel[q].any()                                                                         # two fixed objects
    g, pairs, _, _ = PK.case("3x2")
    g["edge_inlier"][g["edge_obj"] == 1] = 0
    ref = R.covariances(g)
    cross, rel, n_nan = PR.relative(g, ref, pairs)
    hit = np.array([3 + 1 in (a, b) for a, b in pairs])
    assert n_nan == hit.sum() and np.isnan(cross[hit]).all() and np.isnan(rel[hit]).all() and np.isfinite(rel[~hit]).all()
