"""The tail of the network at its edges: decode_kernel, classifier_kernel and kp_masks_kernel (csrc/misc.hip) through suo_decode_heatmaps,
suo_classifier and suo_keypoint_masks, against the fp64 restatement of tests/decode_ref.py (pinned to the reference's recorded outputs by
tests/test_decode_ref.py) on the seeded cases of tests/decode_cases.py.

  a. exact by construction (no tolerance): one peak per map visiting every cell = every (j, lane, t) register position; two and four equal
     peaks (midpoint, (d/2)^2 variances, the SIGN of cxy under the negated column axis); uniform maps.
  b. against fp64: rotated anisotropic blobs inside, on and beyond the border, the same shifted by +-1000, maps with a block of -inf; the
     validity head with checkpoint and O(1) random weights from |a| ~ 0 to |a| > 100, with and without the logit output.
  c. launch tails (L = 1, 2, 3, 7: 1, 2, 3, 3 live waves in the last decode workgroup), guard regions behind every output, poisoned maps.
  d. masks bit-exact against the reference's numpy rule AT the thresholds, on non-finite fields, and on what the device itself decoded.

Tolerances: none comes from the kernel.  "float32 reference" = the error of the reference's own float32 arithmetic (oracle.cnn_oracle on torch
CPU) against fp64 on the same inputs, measured by tests/test_decode_ref.py::test_float32_budget and recorded in tests/decode_cases.py
(BUDGET, with the definition of each error measure); tolerance = 4 x that (another summation order, another expf), capped at 1e-5
(SURVEY.md 7.2).  No family reaches the cap.  Last column: the kernels' maximum on an MI355X.

  family                 quantity    float32 reference  tolerance  observed
  gauss                  uv          1.4e-6             5.6e-6     4.6e-7
  gauss                  cov         5.4e-8             2.2e-7     6.3e-8
  gauss                  cov_rel     2.1e-6             8.4e-6     2.0e-6
  gauss                  mean_logit  8.7e-8             3.5e-7     1.2e-7
  gauss                  prob        1.8e-6             7.2e-6     4.3e-7
  gauss_p1000 / _m1000   uv          1.4e-6             5.6e-6     5.4e-7
  gauss_p1000 / _m1000   cov         1.4e-7             5.6e-7     6.0e-8
  gauss_p1000 / _m1000   cov_rel     2.2e-6             8.8e-6     1.9e-6
  gauss_p1000 / _m1000   mean_logit  1.1e-7             4.4e-7     8.6e-8
  gauss_p1000 / _m1000   prob        1.8e-6             7.2e-6     4.2e-7
  neginf                 uv          1.1e-6             4.4e-6     4.1e-7
  neginf                 cov         1.7e-7             6.8e-7     6.6e-8
  neginf                 cov_rel     2.2e-6             8.8e-6     1.1e-6
  neginf                 prob        2.3e-6             9.2e-6     6.0e-7
  neginf                 mean_logit  -inf, exactly      equality   -inf
  uniform                all         0 (exact sums)     equality   0
  classifier_checkpoint  kp_logit    2.2e-7             8.8e-7     2.2e-7
  classifier_checkpoint  kp_prob     4.8e-8             1.9e-7     4.8e-8
  classifier_random      kp_logit    1.1e-7             4.4e-7     1.1e-7
  classifier_random      kp_prob     5.3e-8             2.1e-7     5.3e-8
"""
import numpy as np
import pytest
import torch

from tests import decode_cases as DC
from tests import decode_ref as DR

pytestmark = pytest.mark.gpu

GUARD = 256                      # elements behind every output
K, CELLS = DR.NUM_KP, DR.HEAT * DR.HEAT
_SENTINEL = {torch.float32: -7.25, torch.int32: -7, torch.uint8: 0xA5}


@pytest.fixture(scope="module")
def ops():
    from suo_slam_amd import _lib
    _lib.require_gpu()
    from tests import hipops
    return hipops


@pytest.fixture(scope="module")
def ref64():
    return {name: DR.decode64(DC.family(name)) for name in DC.FAMILIES}


class _Out:
    """An output of n elements with a sentinel-filled guard region behind it."""

    def __init__(self, n, dtype=torch.float32):
        self.n, self.buf = n, torch.full((n + GUARD,), _SENTINEL[dtype], dtype=dtype, device="cuda")

    def body(self, *shape):
        return self.buf[:self.n].view(*shape)

    def check(self, what):
        assert bool((self.buf[self.n:] == _SENTINEL[self.buf.dtype]).all()), f"{what}: wrote behind its output"


def _decode(ops, logits, extras=True):
    """logits: numpy or cuda tensor [L,41,64,64] -> dict of cuda tensors (argmax / prob only with extras); checks the guards."""
    from suo_slam_amd import _lib
    ld = logits if torch.is_tensor(logits) else ops.dev(logits)
    L = ld.shape[0]
    n = L * K
    o = {"uv": _Out(n * 2), "cov": _Out(n * 4), "mean_logit": _Out(n)}
    if extras:
        o["argmax"], o["prob"] = _Out(n, torch.int32), _Out(n * CELLS)
    _lib.check(_lib.lib().suo_decode_heatmaps(ops.P(ld), L, ops.P(o["uv"].buf), ops.P(o["cov"].buf), ops.P(o["mean_logit"].buf),
                                              ops.P(o["argmax"].buf) if extras else None, ops.P(o["prob"].buf) if extras else None, ops.S()))
    torch.cuda.synchronize()
    for k, v in o.items():
        v.check("decode " + k)
    shapes = {"uv": (L, K, 2), "cov": (L, K, 2, 2), "mean_logit": (L, K), "argmax": (L, K), "prob": (L, K, DR.HEAT, DR.HEAT)}
    return {k: v.body(*shapes[k]) for k, v in o.items()}


def _classifier(ops, mean_logit, W, b, want_logit=True):
    from suo_slam_amd import _lib
    ml = mean_logit if torch.is_tensor(mean_logit) else ops.dev(mean_logit)
    L = ml.shape[0]
    wd, bd = ops.dev(W), ops.dev(b)
    kl, kp = _Out(L * K), _Out(L * K)
    _lib.check(_lib.lib().suo_classifier(ops.P(ml), ops.P(wd), ops.P(bd), L, ops.P(kl.buf) if want_logit else None, ops.P(kp.buf), ops.S()))
    torch.cuda.synchronize()
    kl.check("classifier logits")
    kp.check("classifier probabilities")
    if not want_logit:
        assert bool((kl.buf == _SENTINEL[torch.float32]).all())
    return (kl.body(L, K) if want_logit else None), kp.body(L, K)


def _masks(ops, uv, cov, kp, model_mask, bt, vt):
    from suo_slam_amd import _lib
    uv, cov, kp = (t if torch.is_tensor(t) else ops.dev(t) for t in (uv, cov, kp))
    L = kp.shape[0]
    mm = None if model_mask is None else torch.as_tensor(np.ascontiguousarray(model_mask, np.uint8)).cuda()
    out = _Out(L * K, torch.uint8)
    _lib.check(_lib.lib().suo_keypoint_masks(ops.P(uv), ops.P(cov), ops.P(kp), ops.P(mm), L, float(bt), float(vt), ops.P(out.buf), ops.S()))
    torch.cuda.synchronize()
    out.check("masks")
    got = out.body(L, K).cpu().numpy()
    assert set(np.unique(got)) <= {0, 1}
    return got.astype(bool)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


# ---- a. exact cases -------------------------------------------------------------------------------------------------------------------------
def test_one_peak_visits_every_cell(ops):
    """100 crops x 41 maps; map m has its single peak (200 above a flat 0) at flat cell m % 4096: every (j, lane, t) register position of the
    kernel's row / column mapping at least once.  expf(-200) = 0 exactly, so everything is exact."""
    L = 100
    n = L * K
    cell = torch.arange(n, device="cuda") % CELLS
    logits = torch.zeros((n, CELLS), device="cuda")
    logits[torch.arange(n, device="cuda"), cell] = 200.0
    d = _decode(ops, logits.view(L, K, DR.HEAT, DR.HEAT))
    r = torch.from_numpy(DR.R.astype(np.float32)).cuda()                  # multiples of 1/64: exact
    want_uv = torch.stack([r[cell // DR.HEAT], -r[cell % DR.HEAT]], -1).view(L, K, 2)
    assert torch.equal(d["uv"], want_uv)
    assert bool((d["cov"] == 0).all())
    assert torch.equal(d["argmax"].view(-1), cell.to(torch.int32))
    assert torch.equal(d["prob"].view(n, CELLS), (logits == 200.0).to(torch.float32))
    assert bool((d["mean_logit"] == 200.0 / CELLS).all())


def test_two_and_four_equal_peaks(ops):
    """Midpoint, (d/2)^2 variances and cxy = (du/2)(dv/2) with its sign (diagonal < 0 < anti-diagonal), on floors 0 and +-1000."""
    cases = [(cells, floor) for floor in (0.0, 1000.0, -1000.0) for cells in DC.MULTI_PEAKS]
    cases += cases[:2 * K - len(cases)]
    x = np.concatenate([DC.peak_maps([cells], floor) for cells, floor in cases]).reshape(2, K, DR.HEAT, DR.HEAT)
    d = _np(_decode(ops, x))
    for i, (cells, floor) in enumerate(cases):
        uv, cov = DC.moments_of_cells(cells)
        l, k = divmod(i, K)
        assert np.array_equal(d["uv"][l, k], uv.astype(np.float32)), (cells, floor)
        assert np.array_equal(d["cov"][l, k], cov.astype(np.float32)), (cells, floor, d["cov"][l, k], cov)
        assert d["cov"][l, k, 0, 1] == d["cov"][l, k, 1, 0]
        assert d["argmax"][l, k] == min(cells)
        want_p = np.zeros(CELLS, np.float32)
        want_p[cells] = 1.0 / len(cells)
        assert np.array_equal(d["prob"][l, k].reshape(-1), want_p)
        assert d["mean_logit"][l, k] == np.float32(floor + 200.0 * len(cells) / CELLS)     # integer partial sums below 2^24: exact
    assert d["cov"][0, 0, 0, 1] < 0 < d["cov"][0, 1, 0, 1]


# ---- b. against fp64 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DC.FAMILIES)
def test_family_against_fp64(ops, ref64, name):
    x, ref = DC.family(name), ref64[name]
    d = _np(_decode(ops, x))
    err = DC.decode_errors(d, ref)
    for q in DC.BUDGET[name]:
        print(f"OBSERVED {name} {q} {err[q]:.3e} tolerance {DC.tol(name, q):.1e}")
    for q in DC.BUDGET[name]:
        assert err[q] <= DC.tol(name, q), (name, q, err[q], DC.tol(name, q))
    assert np.array_equal(d["cov"][..., 0, 1], d["cov"][..., 1, 0])
    if name == "neginf":
        assert (d["mean_logit"] == -np.inf).all()
    if name == "uniform":                                                 # (tolerance 0 above: uv = 0 and cov = the analytic value, exactly)
        analytic = np.float32((1 - 1 / 4096) / 3)
        assert np.array_equal(d["mean_logit"], DC.UNIFORM_LEVELS.reshape(3, K))
        assert (d["uv"] == 0).all() and (d["cov"][..., 0, 0] == analytic).all() and (d["cov"][..., 1, 1] == analytic).all()
        assert (d["cov"][..., 0, 1] == 0).all() and (d["argmax"] == 0).all()
    else:
        sure = DR.top2_gap(x.reshape(3, K, -1)) != 0
        assert sure.mean() > 0.99
        assert np.array_equal(d["argmax"][sure], ref["argmax"][sure])
    d2 = _np(_decode(ops, x, extras=False))                               # the extras do not perturb the decode
    for q in ("uv", "cov", "mean_logit"):
        assert np.array_equal(d[q], d2[q], equal_nan=True)


@pytest.mark.parametrize("want_logit", [True, False])
@pytest.mark.parametrize("name", DC.CLASSIFIER_FAMILIES)
def test_classifier_against_fp64(ops, state_dict, name, want_logit):
    m32 = DC.classifier_inputs()
    W, b = DC.classifier_weights(name, state_dict)
    a64, p64 = DR.classifier64(m32, W, b)
    kl, kp = _classifier(ops, m32, W, b, want_logit)
    kl, kp = (None if kl is None else kl.cpu().numpy()), kp.cpu().numpy()
    err = DC.classifier_errors(kl, kp, m32, W, b, a64, p64)
    for q, e in err.items():
        print(f"OBSERVED {name} {q} {e:.3e} tolerance {DC.tol(name, q):.1e}")
    for q, e in err.items():
        assert e <= DC.tol(name, q), (name, q, e, DC.tol(name, q))
    sat = np.abs(a64) > 100
    assert sat.sum() >= 20
    assert np.array_equal(kp[sat], (a64[sat] > 0).astype(np.float32))     # saturated: exactly 0 or 1, never NaN
    assert np.isfinite(kp).all() and (kp >= 0).all() and (kp <= 1).all()
    neg = (m32 <= 0).all(-1)                                              # an all-negative row (zeros of either sign included): the bias alone
    assert neg.any()
    if want_logit:
        assert np.array_equal(kl[neg], np.broadcast_to(b, kl[neg].shape))


# ---- c. launch tails and isolation ----------------------------------------------------------------------------------------------------------
def _tail_maps(L):
    pool = np.concatenate([DC.family("gauss"), DC.family("neginf"), DC.family("gauss_p1000")]).reshape(-1, DR.HEAT, DR.HEAT)
    return pool[:L * K].reshape(L, K, DR.HEAT, DR.HEAT).copy()


def _poison(x):
    """-> (poisoned copy, flat indices of the poisoned maps).  Crop 0 always; the last two maps (the last, partial workgroup) when L > 1."""
    L = x.shape[0]
    p = x.copy().reshape(L * K, DR.HEAT, DR.HEAT)
    p[5], p[9, 17, 33], p[20, 63, 62], p[33] = np.nan, np.nan, np.inf, -np.inf
    idx = [5, 9, 20, 33]
    if L > 1:
        p[L * K - 1], p[L * K - 2, 0, 1] = np.nan, np.nan
        idx += [L * K - 1, L * K - 2]
    return p.reshape(x.shape), np.array(idx)


@pytest.mark.parametrize("L", [1, 2, 3, 7])
def test_launch_tails_guards_and_poisoned_maps(ops, state_dict, L):
    x = _tail_maps(L)
    xp, bad = _poison(x)
    clean, dirty = _np(_decode(ops, x)), _np(_decode(ops, xp))
    ref_clean, ref = DR.decode64(x), DR.decode64(xp)
    good = np.ones(L * K, bool)
    good[bad] = False
    flat = lambda a: a.reshape((L * K,) + a.shape[2:])
    for q in ("uv", "cov", "mean_logit", "argmax", "prob"):               # every other map: bit-identical to the launch without the poison
        assert np.array_equal(flat(dirty[q])[good], flat(clean[q])[good]), q
    assert np.abs(clean["uv"] - ref_clean["uv"]).max() < 1e-5 and np.abs(clean["cov"] - ref_clean["cov"]).max() < 1e-5     # (and right)
    for q in ("uv", "cov", "prob", "mean_logit"):                         # NaN exactly where the reference's are
        assert np.array_equal(np.isnan(dirty[q]), np.isnan(ref[q])), q
    assert np.isnan(flat(dirty["uv"])[bad]).all() and np.isnan(flat(dirty["cov"])[bad]).all()
    assert np.isposinf(flat(dirty["mean_logit"])[20]) and np.isneginf(flat(dirty["mean_logit"])[33])
    assert (dirty["argmax"] >= 0).all() and (dirty["argmax"] < CELLS).all()
    sure = flat(DR.top2_gap(xp.reshape(L, K, -1)) != 0)
    sure[bad] = True                                                      # torch.argmax's convention: first NaN, else first maximum
    assert np.array_equal(flat(dirty["argmax"])[sure], flat(ref["argmax"])[sure])
    assert list(flat(dirty["argmax"])[bad[:4]]) == [0, 17 * 64 + 33, 63 * 64 + 62, 0]
    # the validity head: one NaN heat-map makes all 41 logits of its crop NaN (relu keeps NaN), and every keypoint of the crop is dropped
    W, b = DC.classifier_weights("classifier_checkpoint", state_dict)
    kl_c, kp_c = (t.cpu().numpy() for t in _classifier(ops, clean["mean_logit"], W, b))
    kl_d, kp_d = (t.cpu().numpy() for t in _classifier(ops, dirty["mean_logit"], W, b))
    nan_crop = np.isnan(dirty["mean_logit"]).any(-1)
    assert nan_crop[0] and nan_crop.sum() == (1 if L == 1 else 2)
    assert np.isnan(kl_d[nan_crop]).all() and np.isnan(kp_d[nan_crop]).all()
    assert np.array_equal(kl_d[~nan_crop], kl_c[~nan_crop]) and np.array_equal(kp_d[~nan_crop], kp_c[~nan_crop])
    assert np.isfinite(kl_c).all()
    a64, _ = DR.classifier64(dirty["mean_logit"], W, b)
    assert np.array_equal(np.isnan(a64), np.isnan(kl_d))
    mm = (np.random.default_rng(L).random((L, K)) > 0.2).astype(np.uint8)
    for bt, vt in DC.THRESHOLDS:
        for model_mask in (None, mm):
            for d, kp in ((clean, kp_c), (dirty, kp_d)):
                got = _masks(ops, d["uv"], d["cov"], kp, model_mask, bt, vt)
                assert np.array_equal(got, DR.masks_ref(d["uv"], d["cov"], kp, model_mask, bt, vt))
            assert not got[nan_crop].any()


# ---- d. masks at the thresholds -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bt,vt", DC.THRESHOLDS)
def test_masks_at_the_thresholds_and_on_non_finite_fields(ops, bt, vt):
    """Every element, no 'near' exclusion: strict comparisons, the float32 conversion of 0.3, +-bt and 2*vt, the rounding of sqrtf, NaN / inf /
    negative and zero variances, model_mask NULL and with the bytes 0, 1, 2, 255."""
    uv, cov, kp, mm = DC.mask_cases(bt, vt)
    for model_mask in (None, mm):
        got = _masks(ops, uv, cov, kp, model_mask, bt, vt)
        want = DR.masks_ref(uv, cov, kp, model_mask, bt, vt)
        assert np.array_equal(got, want), np.argwhere(got != want)


def test_chain_masks_equal_the_rule_on_what_the_device_decoded(ops, state_dict):
    """decode -> classifier -> masks on the device over the maps of a. and b.; the mask equals the reference's rule applied to the very
    uv / cov / kp read back: no tolerance, no exclusion."""
    W, b = DC.classifier_weights("classifier_checkpoint", state_dict)
    one_hot = DC.peak_maps([[c] for c in np.random.default_rng(7).integers(0, CELLS, K - len(DC.MULTI_PEAKS))])
    exact = np.concatenate([DC.peak_maps(DC.MULTI_PEAKS), one_hot]).reshape(1, K, DR.HEAT, DR.HEAT)
    x = np.concatenate([exact] + [DC.family(name) for name in DC.FAMILIES])
    L = x.shape[0]
    assert L == 16
    d = _decode(ops, x, extras=False)
    _, kp = _classifier(ops, d["mean_logit"], W, b, want_logit=False)
    mm = (np.random.default_rng(8).random((L, K)) > 0.2).astype(np.uint8)
    uv, cov, kpn = d["uv"].cpu().numpy(), d["cov"].cpu().numpy(), kp.cpu().numpy()
    seen = set()
    for bt, vt in DC.THRESHOLDS:
        for model_mask in (None, mm):
            got = _masks(ops, d["uv"], d["cov"], kp, model_mask, bt, vt)
            assert np.array_equal(got, DR.masks_ref(uv, cov, kpn, model_mask, bt, vt))
            seen |= set(np.unique(got))
    assert seen == {False, True}
