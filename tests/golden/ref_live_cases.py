"""Seeded inputs of the two tests that run the REFERENCE's compiled code live when oracle/_ref is built (tests/test_oracle_geometry.py:
test_p4p_live_reference_library, tests/test_ref_sampler.py: test_restatement_equals_the_compiled_reference_header), shared with
tests/golden/make_ref_live_golden.py, which records what that code returns for them (ref_live_golden.npz) so that the tests hold without it."""
import numpy as np


def p4p_cases():
    """300 (x [6,3], y [6,2], idx of 4) problems: random rigid motions of random points, projected with 1e-3 noise."""
    from suo_slam_amd import synthetic as S
    rng = np.random.default_rng(5)
    for _ in range(300):
        x = rng.uniform(-100, 100, (6, 3))
        Q = S.random_rotation(rng)
        X = x @ Q.T + np.array([rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(400, 1200)])
        y = X[:, :2] / X[:, 2:3] + rng.normal(0, 1e-3, (6, 2))
        idx = sorted(rng.choice(6, 4, replace=False).tolist())
        yield x, y, idx


def sampler_ops():
    """40 operations on ONE continuing stream from a fresh seed: ("randui", n, k) = k raw draws in [0, n), ("get4", n, k) = k 4-point samples of n."""
    rng = np.random.default_rng(0)
    for _ in range(40):
        n = int(rng.integers(4, 64))
        k = int(rng.integers(1, 200))
        yield ("randui" if rng.random() < 0.5 else "get4"), n, k
