"""The numpy reference of the consistency figures (tests/nees_ref.py) checked on its own, and the Monte-Carlo inputs of tests/test_gpu_nees.py proven inside
their gates WITHOUT the library: the same generator and seed through a numpy Gauss-Newton (no GPU needed)."""
import numpy as np
import pytest

from tests import nees_ref as R


@pytest.mark.parametrize("theta", [0.0, 1e-9, 1e-4, 0.3, 3.0])
def test_log_inverts_exp(theta):
    rng = np.random.default_rng(3)
    for _ in range(8):
        axis = rng.normal(size=3)
        xi = np.r_[theta * axis / np.linalg.norm(axis), rng.normal(0, 0.05, 3)]
        got = R.log_se3(R.exp_se3(xi))
        assert np.abs(got - xi).max() <= 1e3 * R.EPS * (1 + np.abs(xi).max())


def test_exp_is_the_matrix_exponential():
    xi = np.array([0.3, -0.2, 0.5, 0.01, 0.02, -0.03])
    M = np.zeros((4, 4))
    M[:3, :3], M[:3, 3] = R.skew(xi[:3]), xi[3:]
    E, term = np.eye(4), np.eye(4)
    for k in range(1, 30):
        term = term @ M / k
        E = E + term
    assert np.abs(R.exp_se3(xi) - E).max() < 1e-14


def test_brute_force_pick_returns_the_planted_symmetry():
    rng = np.random.default_rng(4)
    pts = rng.uniform(-0.05, 0.05, (200, 3))
    syms = []
    for k in range(4):
        a = 0.5 * np.pi * k
        S = np.eye(4)
        S[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
        S[:3, 3] = -S[:3, :3] @ [0.01, 0.02, 0] + [0.01, 0.02, 0]
        syms.append(S[:3])
    T_gt = np.eye(4)
    T_gt[:3, :3], T_gt[:3, 3] = R._rot(rng), [0.1, -0.05, 0.8]
    for j in range(4):
        T_est = R.exp_se3(np.r_[rng.normal(0, 0.01, 3), rng.normal(0, 0.002, 3)]) @ T_gt @ R.to4(syms[j])
        assert R.symmetry_pick(pts, syms, T_est, T_gt)[0] == j
        ref = R.pose_nees(pts, syms, T_est, T_gt, np.eye(6))
        assert ref["sym_index"] == j and np.abs(ref["xi"]).max() < 0.05
    # a symmetry listed twice: the first wins
    assert R.symmetry_pick(pts, [syms[0], syms[2], syms[2]], T_gt @ R.to4(syms[2]), T_gt)[0] == 1


def test_keypoint_chi2_of_an_exact_projection_is_zero():
    mc = R.monte_carlo(4, seed=5)
    chi2, err = R.keypoint_chi2(mc["p"][0], mc["uv"][0], mc["cov"][0], R.keypoint_K(mc["k"][0]), mc["T_gt"][0])
    assert chi2.shape == (R.N_KP,) and np.abs(err).max() < 10 * R.SIGMA


def test_monte_carlo_inputs_are_inside_the_gates_on_the_reference_alone():
    """seed 0, 4096 frames, 16 keypoints, sigma 0.001 through the numpy Gauss-Newton: mean NEES 6.0356, share <= 16.8119 0.9873, mean keypoint chi2 1.9972,
    share <= 9.210 0.9900 when this was written; the gates are six standard errors of the exact distributions."""
    mc = R.monte_carlo()
    T, Sigma = R.monte_carlo_chain()
    mean, frac = R.check_pose_gates(R.mc_pose_nees(mc, T, Sigma))
    kmean, kfrac = R.check_keypoint_gates(R.mc_keypoint_chi2(mc))
    print(f"numpy chain: mean NEES {mean:.4f}, share {frac:.4f}; keypoints mean chi2 {kmean:.4f}, share {kfrac:.4f}")


def test_the_gate_tells_a_swapped_convention():
    mc = R.monte_carlo()
    T, Sigma = R.monte_carlo_chain()
    perm = [3, 4, 5, 0, 1, 2]
    with pytest.raises(AssertionError):
        R.check_pose_gates(R.mc_pose_nees({k: v[:512] for k, v in mc.items()}, T[:512], Sigma[:512][:, perm][:, :, perm]))
