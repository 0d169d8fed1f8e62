"""Pins tests/pose_cov_ref.py, the reference the GPU tests of the pose covariances compare with: its finite-difference Jacobians against the analytic algebra
of tests/ba_numpy_phases.py, its Hessian blocks against that module's normal equations, and its conventions for fixed and unreachable vertices."""
import numpy as np

from suo_slam_amd import ba
from tests import ba_numpy_phases as NP
from tests import pose_cov_cases as K
from tests import pose_cov_ref as R


def _analytic(g, e):
    """EdgeSE3ProjectFromObject's Jacobians as tests/ba_numpy_phases.py: _linearize writes them"""
    Tc, To = R.to4(g["cam_T"][g["edge_cam"][e]]), R.to4(g["obj_T"][g["edge_obj"][e]])
    pw = To[:3, :3] @ g["edge_p"][e] + To[:3, 3]
    pc = Tc[:3, :3] @ pw + Tc[:3, 3]
    k = g["edge_camk"][e]
    PJ = -np.array([[k[0] / pc[2], 0, -k[0] * pc[0] / pc[2] ** 2], [0, k[1] / pc[2], -k[1] * pc[1] / pc[2] ** 2]])
    return PJ @ np.hstack([-NP._skew(pc), np.eye(3)]), PJ @ Tc[:3, :3] @ np.hstack([-NP._skew(pw), np.eye(3)])


def test_jacobians_agree_with_the_numpy_phases_algebra():
    g, _ = K.case("3x2")
    for e in range(len(g["edge_cam"])):
        Jc, Jo = R.edge_jacobians(g, e)
        Ac, Ao = _analytic(g, e)
        assert np.abs(Jc - Ac).max() <= 1e-8 and np.abs(Jo - Ao).max() <= 1e-8, e


def test_hessian_blocks_agree_with_the_numpy_phases_normal_equations():
    g, ref = K.case("3x2")
    ph = NP.NumpyPhases(ba.Problem(*K.args(g)))
    lin = ph._linearize(False)
    H = ref["H"]                       # free cameras 1, 2 then objects 0, 1
    scale = np.abs(H).max()
    for i, c in enumerate((1, 2)):
        assert np.abs(H[6 * i:6 * i + 6, 6 * i:6 * i + 6] - ph.Hcc[c]).max() <= 1e-8 * scale
        for o in (0, 1):
            assert np.abs(H[6 * i:6 * i + 6, 12 + 6 * o:18 + 6 * o] - ph.Hco[(c, o)]).max() <= 1e-8 * scale
    iu = np.triu_indices(6)
    for o in (0, 1):
        assert np.abs(H[12 + 6 * o:18 + 6 * o, 12 + 6 * o:18 + 6 * o][iu] - lin[1 + 27 * o:1 + 27 * o + 21]).max() <= 1e-8 * scale


def test_fixed_vertices_are_zero_and_unreachable_ones_nan():
    g, _ = K.case("3x2")
    g["edge_inlier"][g["edge_obj"] == 1] = 0
    g["obj_fixed"][:] = 0
    r = R.covariances(g)
    assert np.all(r["cam_cov"][0] == 0) and np.isnan(r["obj_cov"][1]).all() and list(r["status"]) == [0, 1]
    assert np.isfinite(r["obj_cov"][0]).all() and np.isfinite(r["cam_cov"][1:]).all()
    assert r["H"].shape == (18, 18) and np.allclose(r["Sigma"] @ r["H"], np.eye(18), atol=1e-6)


def test_every_case_is_well_conditioned():
    for name in K.CASES:
        _, ref = K.case(name)
        if ref is not None:
            assert ref["cond"] <= 1e9, (name, ref["cond"])
