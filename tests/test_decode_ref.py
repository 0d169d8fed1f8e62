"""CPU: pins tests/decode_ref.py (the fp64 yardstick of tests/test_gpu_decode_edges.py) to what the reference program recorded and to
oracle.cnn_oracle, checks that the seeded case families of tests/decode_cases.py are what they claim to be, and measures the float32 budget
the GPU tolerances are derived from."""
import numpy as np
import pytest
import torch

from tests import decode_cases as DC
from tests import decode_ref as DR


@pytest.fixture(scope="module")
def ref64():
    """decode64 of every family, computed once."""
    return {name: DR.decode64(DC.family(name)) for name in DC.FAMILIES}


@pytest.fixture(scope="module")
def oracle32(state_dict):
    """The reference's own float32 arithmetic (torch CPU) on every family."""
    from oracle import cnn_oracle as O
    P = O.to_torch(state_dict)
    out = {}
    for name in DC.FAMILIES:
        raw = torch.from_numpy(DC.family(name))
        d = O.decode(raw, P)
        out[name] = {"uv": d["uv"].numpy(), "cov": d["cov"].numpy(), "prob": d["prob"].numpy(), "mean_logit": raw.mean(3).mean(2).numpy()}
    return out


@pytest.mark.parametrize("key", ["decode", "backbone"])
def test_restatement_reproduces_the_recorded_reference_outputs(cnn_golden, state_dict, key):
    """Same arrays, same tolerances as tests/test_gpu_cnn.py::test_decode_golden_and_masks / test_decode_hard_argmax_..."""
    logits = cnn_golden["decode_in"] if key == "decode" else cnn_golden["backbone_logits"]
    d = DR.decode64(logits)
    kl, kp = DR.classifier64(d["mean_logit"], state_dict["classifier.2.weight"], state_dict["classifier.2.bias"])
    np.testing.assert_allclose(d["uv"], cnn_golden[key + "_uv"], atol=1e-5, rtol=0)
    np.testing.assert_allclose(d["cov"], cnn_golden[key + "_cov"], atol=1e-5, rtol=0)
    np.testing.assert_allclose(kl, cnn_golden[key + "_kp_mask_logits"], atol=2e-5, rtol=0)
    np.testing.assert_allclose(kp, cnn_golden[key + "_kp_mask"], atol=1e-5, rtol=0)
    np.testing.assert_array_equal(d["argmax"], cnn_golden[key + "_argmax"])
    np.testing.assert_allclose(d["prob"][:, ::5, ::4, ::4], cnn_golden[key + "_prob_sample"], rtol=2e-6, atol=1e-12)
    assert np.array_equal(DR.XX.reshape(64, 64).astype(np.float32), cnn_golden["mesh_xx"])          # u from the row,
    assert np.array_equal(DR.YY.reshape(64, 64).astype(np.float32), cnn_golden["mesh_yy"])          # v from the negated column


def test_argmax_convention_is_torchs():
    rng = np.random.default_rng(0)
    x = np.floor(rng.uniform(0, 4, (50, 4096))).astype(np.float32)          # full of ties
    x[10:20, 77], x[15:25, 3000], x[30, :], x[31, 4095] = np.nan, np.nan, np.nan, np.inf
    x[32, :] = -np.inf
    got = DR.argmax_torch(x)
    np.testing.assert_array_equal(got, torch.argmax(torch.from_numpy(x), -1).numpy())
    assert got[12] == 77 and got[22] == 3000 and got[30] == 0 and got[31] == 4095 and got[32] == 0


def test_non_finite_maps_follow_the_reference(state_dict):
    """What the reference's float32 program makes of poisoned maps is what decode64 / classifier64 make of them (NaN pattern, arg-max)."""
    from oracle import cnn_oracle as O
    P = O.to_torch(state_dict)
    x = DC.family("gauss")[:1].copy()
    x[0, 3], x[0, 7, 5, 9], x[0, 11, 63, 0], x[0, 13], x[0, 17, 8:20, 30:50] = np.nan, np.nan, np.inf, -np.inf, -np.inf
    d, o = DR.decode64(x), O.decode(torch.from_numpy(x), P)
    for k in ("uv", "cov", "prob"):
        assert np.array_equal(np.isnan(d[k]), np.isnan(o[k].numpy())), k
    bad = np.zeros(41, bool)
    bad[[3, 7, 11, 13]] = True
    assert np.array_equal(np.isnan(d["uv"]).all(-1)[0], bad) and np.isfinite(d["cov"][0, 17]).all() and d["mean_logit"][0, 17] == -np.inf
    np.testing.assert_array_equal(d["argmax"], torch.argmax(torch.from_numpy(x).reshape(1, 41, -1), -1).numpy())
    kl, kp = DR.classifier64(d["mean_logit"], state_dict["classifier.2.weight"], state_dict["classifier.2.bias"])
    assert np.isnan(kl).all() and np.isnan(kp).all() and np.isnan(o["kp_mask_logits"].numpy()).all()      # relu keeps the NaN: all 41 logits


def test_multi_peak_expectations_have_the_closed_form():
    """Two equal peaks: uv = the midpoint, cxx = (du/2)^2, cyy = (dv/2)^2, cxy = (du/2)(dv/2) with the sign of the diagonal."""
    for cells in DC.MULTI_PEAKS:
        uv, cov = DC.moments_of_cells(cells)
        assert cov[0, 1] == cov[1, 0]
        for a in (uv, cov):
            assert np.array_equal(a.astype(np.float32).astype(np.float64), a)        # representable: the kernel can be asked for equality
        if len(cells) == 2:
            (r0, c0), (r1, c1) = divmod(cells[0], 64), divmod(cells[1], 64)
            du, dv = (r1 - r0) / 32, -(c1 - c0) / 32
            assert np.array_equal(uv, [(DR.R[r0] + DR.R[r1]) / 2, -(DR.R[c0] + DR.R[c1]) / 2])
            assert np.array_equal(cov, [[du * du / 4, du * dv / 4], [du * dv / 4, dv * dv / 4]])
    assert DC.moments_of_cells(DC.MULTI_PEAKS[0])[1][0, 1] < 0 < DC.moments_of_cells(DC.MULTI_PEAKS[1])[1][0, 1]
    d = DR.decode64(DC.peak_maps(DC.MULTI_PEAKS).reshape(1, -1, 64, 64))              # (fp64: exp(-200) = 1e-87 does not reach the last bit)
    for i, cells in enumerate(DC.MULTI_PEAKS):
        uv, cov = DC.moments_of_cells(cells)
        np.testing.assert_allclose(d["uv"][0, i], uv, rtol=0, atol=1e-15)
        np.testing.assert_allclose(d["cov"][0, i], cov, rtol=0, atol=1e-15)


def test_families_meet_the_issues_conditions(ref64):
    for name in DC.FAMILIES:
        x, d = DC.family(name), ref64[name]
        n = x.shape[0] * x.shape[1]
        assert n >= 100 and x.dtype == np.float32
        assert np.isfinite(d["uv"]).all() and np.isfinite(d["cov"]).all() and np.isfinite(d["prob"]).all(), name
        if name != "uniform":
            ties = DR.top2_gap(x.reshape(n, -1)) == 0
            assert ties.sum() < 0.01 * n, (name, int(ties.sum()))
    assert (ref64["neginf"]["mean_logit"] == -np.inf).all()
    g = ref64["gauss"]
    assert np.abs(g["uv"]).max() > 0.95                                   # truncated blobs reach the border
    assert g["cov"][..., 0, 0].min() < (0.5 / 32) ** 2 and g["cov"][..., 0, 0].max() > 0.03         # sharp peaks and broad ones
    rho = g["cov"][..., 0, 1] / np.sqrt(g["cov"][..., 0, 0] * g["cov"][..., 1, 1])
    assert rho.min() < -0.5 and rho.max() > 0.5                           # both orientations of a slanted blob
    analytic = (1 - 1 / 4096) / 3
    u = ref64["uniform"]
    np.testing.assert_allclose(u["cov"], np.broadcast_to(np.diag([analytic, analytic]), u["cov"].shape), rtol=0, atol=1e-14)
    assert np.abs(u["uv"]).max() < 1e-14 and np.array_equal(u["mean_logit"], DC.UNIFORM_LEVELS.reshape(3, 41).astype(np.float64))


def _within(measured, recorded):
    return recorded / 3 <= measured <= recorded * 3


def test_float32_budget(ref64, oracle32, state_dict):
    """Measures the error of the reference's float32 arithmetic against fp64 and holds DC.BUDGET to it (within [1/3, 3] x: torch's CPU sums
    depend on the vector width of the machine).  Prints the table for the docstring of tests/test_gpu_decode_edges.py."""
    from oracle import cnn_oracle as O
    measured = {name: DC.decode_errors(oracle32[name], ref64[name]) for name in DC.FAMILIES}
    m32 = DC.classifier_inputs()
    for name in DC.CLASSIFIER_FAMILIES:
        W, b = DC.classifier_weights(name, state_dict)
        a64, p64 = DR.classifier64(m32, W, b)
        a32 = torch.nn.functional.linear(torch.relu(torch.from_numpy(m32)), torch.from_numpy(W), torch.from_numpy(b))
        measured[name] = DC.classifier_errors(a32.numpy(), torch.sigmoid(a32).numpy(), m32, W, b, a64, p64)
        assert (np.abs(a64) > 100).sum() >= 20 and (np.abs(a64) < 1).sum() >= 5
        sat = np.abs(a64) > 100
        assert np.abs(p64[sat] - (a64[sat] > 0)).max() < 4e-44               # saturated: 0 or 1 to below float32's smallest normal number
    bad = []
    for name, row in DC.BUDGET.items():
        for q, recorded in row.items():
            print(f"BUDGET {name:22s} {q:10s} measured {measured[name][q]:.3e} recorded {recorded:.1e} tolerance {DC.tol(name, q):.1e}")
            if not _within(measured[name][q], recorded):
                bad.append((name, q, measured[name][q], recorded))
    assert not bad, bad


@pytest.mark.parametrize("bt,vt", DC.THRESHOLDS)
def test_masks_ref_is_the_oracles_rule_at_the_thresholds(bt, vt):
    from oracle import cnn_oracle as O
    uv, cov, kp, mm = DC.mask_cases(bt, vt)
    assert uv.shape[0] <= 7
    for model_mask in (None, mm):
        want = O.keypoint_masks(uv, cov, kp, np.ones(kp.shape, bool) if model_mask is None else model_mask, bt, vt)
        got = DR.masks_ref(uv, cov, kp, model_mask, bt, vt)
        assert got.dtype == bool and np.array_equal(got, want)
    m = DR.masks_ref(uv, cov, kp, None, bt, vt).reshape(-1)
    # the cases really straddle each gate: strict comparisons, float32 thresholds
    assert list(m[:4]) == [True, False, False, True]                     # base; kp = pred(0.3f), 0.3f, succ(0.3f)
    assert list(m[4:10]) == [True, False, False, False, False, True]     # u at bt (pred, =, succ), then at -bt
    assert list(m[16:22]) == [True, True, False, True, True, False]      # cxx, cyy: c - 1 ulp, c, c + 1 ulp
    c = DC.largest_variance_below(vt)
    assert np.sqrt(c) < np.float32(2 * vt) and not np.sqrt(np.nextafter(c, np.float32(np.inf))) < np.float32(2 * vt)
    assert 0 < m.sum() < m.size


def test_masks_ref_is_the_oracles_rule_on_decoded_maps(oracle32, state_dict):
    """The chain test's inputs come off the device; here the same rule on the float32 reference's decode of the same maps."""
    from oracle import cnn_oracle as O
    rng = np.random.default_rng(5)
    for name in DC.FAMILIES:
        o = oracle32[name]
        kp = rng.uniform(0, 1, o["uv"].shape[:2]).astype(np.float32)
        mm = (rng.random(kp.shape) > 0.2).astype(np.uint8) * 255
        for bt, vt in DC.THRESHOLDS:
            assert np.array_equal(DR.masks_ref(o["uv"], o["cov"], kp, mm, bt, vt), O.keypoint_masks(o["uv"], o["cov"], kp, mm, bt, vt))
