"""The references of the suo_pose_covariances_graph tests on the CPU: every large graph stays inside what the constant of pose_cov_ref.bound assumes, the
finite-difference Jacobian of a (camera, camera) pair equals the formula the header states, and the covariance of the motion between two cameras does not depend
on which camera is fixed."""
import numpy as np
import pytest

from tests import pose_cov_cases as K
from tests import pose_cov_graph_cases as GK
from tests import pose_cov_graph_ref as GR
from tests import pose_cov_ref as R


@pytest.mark.parametrize("name", GK.NAMES)
def test_large_graphs_stay_inside_the_bounds_constant(name):
    g, ref = GK.case(name)
    n = ref["H"].shape[0]
    print(f"{name}: n {n}  cond(H) {ref['cond']:.2e}  bound {R.bound(ref):.2e}  status {ref['status']}")
    assert n <= 200 and ref["cond"] <= 1e9
    assert list(ref["status"]) == [0, 0]
    assert len(g["obj_T"]) > 16 and not g["obj_fixed"].any() and (~g["cam_fixed"].astype(bool)).any(), "more free objects than the LDS form holds, next to a free camera"


def test_camera_pair_jacobian_equals_the_adjoint_formula():
    for name in ("3x2", "5x16"):
        g, _ = K.case(name)
        C = len(g["cam_T"])
        for a in range(C):
            for b in range(C):
                Ta, Tb = R.to4(g["cam_T"][a]), R.to4(g["cam_T"][b])
                A = GR.adjoint(Tb @ np.linalg.inv(Ta))
                J = GR.camera_pair_jacobian(Ta, Tb)
                assert np.abs(J - np.hstack([-A, np.eye(6)])).max() <= 1e-9, (name, a, b)


def test_the_motion_between_two_cameras_does_not_depend_on_the_gauge():
    g0, ref0 = K.case("3x2")
    g1 = {k: v.copy() for k, v in g0.items()}
    g1["cam_fixed"] = np.array([0, 1, 0], np.uint8)
    ref1 = R.covariances(g1)
    assert max(ref0["cond"], ref1["cond"]) <= 1e9
    pairs = np.array([(a, b) for a in range(3) for b in range(3) if a != b], np.int32)
    _, rel0, n0 = GR.relative(g0, ref0, pairs)
    _, rel1, n1 = GR.relative(g1, ref1, pairs)
    assert n0 == 0 and n1 == 0
    worst = 0.0
    for q, (a, b) in enumerate(pairs):
        amax = np.abs(GR.adjoint(R.to4(g0["cam_T"][b]) @ np.linalg.inv(R.to4(g0["cam_T"][a])))).max()
        tol = (R.bound(ref0) + R.bound(ref1)) * (1 + 6 * amax) ** 2
        err = float(np.abs(rel0[q] - rel1[q]).max())
        worst = max(worst, err / tol)
        assert err <= tol, (a, b, err, tol)
    print(f"camera pairs of 3x2, camera 0 fixed against camera 1 fixed: difference / summed tolerance {worst:.4f}")
    marginal = float(np.abs(ref0["cam_cov"][2] - ref1["cam_cov"][2]).max())
    assert marginal > 1e3 * (R.bound(ref0) + R.bound(ref1)), "the marginal block of camera 2 does depend on the gauge"


def test_fixed_cameras_contribute_zeros_and_a_camera_with_itself_cannot_move():
    g, ref = K.case("3x2")
    pairs = np.array([(0, 1), (1, 0), (0, 0), (2, 2)], np.int32)
    cross, rel, n_nan = GR.relative(g, ref, pairs)
    assert n_nan == 0 and not cross[0].any() and not cross[1].any() and not rel[2].any() and not cross[2].any()
    scale = np.abs(ref["cam_cov"][1]).max()
    assert np.abs(rel[0] - ref["cam_cov"][1]).max() <= 1e-8 * scale, "(gauge, c): Sigma_cc"
    A = GR.adjoint(np.linalg.inv(R.to4(g["cam_T"][1])))            # T_0 = I
    assert np.abs(rel[1] - A @ ref["cam_cov"][1] @ A.T).max() <= 1e-8 * scale * np.abs(A).max() ** 2, "(c, gauge): A Sigma_cc A^T"
    assert np.abs(cross[3] - ref["cam_cov"][2]).max() == 0 and np.abs(rel[3]).max() <= 1e-8 * scale, "(c, c)"
