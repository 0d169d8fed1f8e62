"""Seeded inputs of tests/test_gpu_decode_edges.py, shared with tests/test_decode_ref.py (which checks on the CPU that the families are large
enough, nearly free of arg-max ties, and measures the float32 budget).  numpy only; nothing here looks at a kernel's output.

BUDGET is the error of the reference's own float32 arithmetic (oracle.cnn_oracle.decode / classifier on torch CPU) against the fp64
restatement of tests/decode_ref.py, per family and quantity, as measured by tests/test_decode_ref.py::test_float32_budget (which fails when a
re-measurement leaves [1/3, 3] x the recorded figure).  tol() is what the GPU test asserts: 4 x that figure -- the kernel adds 4096 terms in
another order (64 per lane, then a 6-step tree) and has another expf -- capped at the project's 1e-5.

Error measures (each a maximum over the family):
  uv          |d uv|
  cov         |d cov|, all four entries
  cov_rel     |d cov| / max(cxx, cyy) of the same map (fp64 values)
  mean_logit  |d mean| / max(1, |mean|): a float32 near 1000 has an ulp of 6.1e-5, so no float32 result can meet 1e-5 absolutely there
  prob        |d prob| / max(prob) of the same map
  kp_logit    |d a| / S with S = max(1, sum_j |W_kj| relu(m_j) + |b_k|), the scale the rounding errors of the dot product carry
  kp_prob     |d sigmoid(a)| / S: the sigmoid passes on up to a quarter of the logit's error, which grows with S (a logit near 0 formed from
              terms of size 1e4 cannot be held to 1e-5 absolutely by any float32 program; the reference's own error there is 2.3e-5)"""
import numpy as np

from tests.decode_ref import HEAT, NUM_KP

CAP = 1e-5

BUDGET = {
    "gauss":       {"uv": 1.4e-6, "cov": 5.4e-8, "cov_rel": 2.1e-6, "mean_logit": 8.7e-8, "prob": 1.8e-6},
    "gauss_p1000": {"uv": 1.4e-6, "cov": 1.4e-7, "cov_rel": 2.2e-6, "mean_logit": 1.1e-7, "prob": 1.8e-6},
    "gauss_m1000": {"uv": 1.4e-6, "cov": 1.4e-7, "cov_rel": 2.2e-6, "mean_logit": 1.1e-7, "prob": 1.8e-6},
    "neginf":      {"uv": 1.1e-6, "cov": 1.7e-7, "cov_rel": 2.2e-6, "prob": 2.3e-6},                      # (mean_logit is -inf: equality)
    "uniform":     {"uv": 0.0, "cov": 0.0, "cov_rel": 0.0, "prob": 0.0},     # every sum is exact in float32: equality (mean_logit too)
    "classifier_checkpoint": {"kp_logit": 2.2e-7, "kp_prob": 4.8e-8},
    "classifier_random":     {"kp_logit": 1.1e-7, "kp_prob": 5.3e-8},
}


def tol(family, quantity):
    return min(4.0 * BUDGET[family][quantity], CAP)


# ---- heat-map families ----------------------------------------------------------------------------------------------------------------------
def _gauss(rng, L, block=False):
    """L*41 rotated anisotropic Gaussian blobs (amplitude 5..60, sigma 0.3..8 cells along each principal axis, any angle) over N(0, 0.5) noise.
    Positions in cell units: cell i is centred at i, the map spans [-0.5, 63.5].  The first 8 centres lie within one cell of a border (4) or
    of a corner (4), the next 32 up to 4 cells OUTSIDE the map (truncated blobs; sigma >= 1.5 so the tail reaches in), the rest inside."""
    n = L * NUM_KP
    lo, hi = -0.5, HEAT - 0.5
    rows, cols = np.meshgrid(np.arange(HEAT, dtype=np.float64), np.arange(HEAT, dtype=np.float64), indexing="ij")
    out = np.empty((n, HEAT, HEAT), np.float32)
    for i in range(n):
        cy, cx = rng.uniform(2, HEAT - 3, 2)
        smin = 0.3
        if i < 4:                                                        # within a cell of the top / bottom / left / right border
            near = lo + rng.uniform(0, 1) if i % 2 == 0 else hi - rng.uniform(0, 1)
            cy, cx = (near, cx) if i < 2 else (cy, near)
        elif i < 8:                                                      # ... of each corner
            cy = lo + rng.uniform(0, 1) if i & 1 else hi - rng.uniform(0, 1)
            cx = lo + rng.uniform(0, 1) if i & 2 else hi - rng.uniform(0, 1)
        elif i < 40:                                                     # outside: beyond one border, or beyond two (past a corner)
            smin = 1.5
            k = i - 8
            out_y = lo - rng.uniform(0, 4) if k & 1 else hi + rng.uniform(0, 4)
            out_x = lo - rng.uniform(0, 4) if k & 2 else hi + rng.uniform(0, 4)
            which = (k >> 2) % 3
            cy, cx = (out_y, cx) if which == 0 else (cy, out_x) if which == 1 else (out_y, out_x)
        s1, s2 = np.exp(rng.uniform(np.log(smin), np.log(8.0), 2))
        th = rng.uniform(0, np.pi)
        amp = rng.uniform(5, 60)
        a = np.cos(th) * (rows - cy) + np.sin(th) * (cols - cx)
        b = -np.sin(th) * (rows - cy) + np.cos(th) * (cols - cx)
        m = amp * np.exp(-0.5 * ((a / s1) ** 2 + (b / s2) ** 2)) + 0.5 * rng.standard_normal((HEAT, HEAT))
        if block:                                                        # a rectangle of -inf cells, anywhere (it may cover the peak)
            h, w = rng.integers(1, 33, 2)
            r0, c0 = rng.integers(0, HEAT - h + 1), rng.integers(0, HEAT - w + 1)
            m[r0:r0 + h, c0:c0 + w] = -np.inf
        out[i] = m.astype(np.float32)
    return out.reshape(L, NUM_KP, HEAT, HEAT)


UNIFORM_LEVELS = np.concatenate([[0.0, 1000.0, -1000.0], np.linspace(-990, 990, 3 * NUM_KP - 3).round()]).astype(np.float32)


def family(name):
    """float32 logits [3,41,64,64] of a family compared with fp64 (123 maps each)."""
    if name == "gauss":
        return _gauss(np.random.default_rng(101), 3)
    if name in ("gauss_p1000", "gauss_m1000"):                           # rounded to float32 after the shift: kernel and reference read these values
        return (family("gauss") + np.float32(1000.0 if name == "gauss_p1000" else -1000.0)).astype(np.float32)
    if name == "neginf":
        return _gauss(np.random.default_rng(102), 3, block=True)
    if name == "uniform":                                                # integer levels: sums of 4096 of them are exact in float32
        return np.broadcast_to(UNIFORM_LEVELS.reshape(3, NUM_KP, 1, 1), (3, NUM_KP, HEAT, HEAT)).copy()
    raise KeyError(name)


FAMILIES = ("gauss", "gauss_p1000", "gauss_m1000", "neginf", "uniform")


def peak_maps(cells_per_map, floor=0.0, height=200.0):
    """One map per entry of cells_per_map (a list of lists of flat cells): `height` above a flat `floor` at those cells.  expf(-200) is
    exactly 0 in float32, so the soft-max is exactly 1/len(cells) there and 0 elsewhere."""
    out = np.full((len(cells_per_map), HEAT * HEAT), floor, np.float32)
    for i, cells in enumerate(cells_per_map):
        out[i, list(cells)] = floor + height
    return out


def _c(r, c):
    return r * HEAT + c


# two / four equal peaks: (cells, note).  Every moment of these point sets is a dyadic rational with few bits: exact in float32 in any order.
MULTI_PEAKS = [
    [_c(10, 20), _c(14, 26)],                   # diagonal pair: row and column grow together -> cxy < 0 (v = -r[col])
    [_c(10, 26), _c(14, 20)],                   # anti-diagonal pair -> cxy > 0
    [_c(0, 0), _c(63, 63)],                     # corner to corner
    [_c(0, 63), _c(63, 0)],
    [_c(31, 31), _c(31, 32)],                   # adjacent cells, same row / same column / diagonal
    [_c(31, 31), _c(32, 31)],
    [_c(31, 31), _c(32, 32)],
    [_c(0, 0), _c(0, 1)],
    [_c(63, 62), _c(63, 63)],
    [_c(5, 40), _c(50, 40)],                    # same column: cyy = cxy = 0
    [_c(7, 3), _c(7, 60)],                      # same row
    [_c(10, 20), _c(10, 26), _c(14, 20), _c(14, 26)],      # rectangle: cxy = 0
    [_c(0, 0), _c(0, 63), _c(63, 0), _c(63, 63)],          # the four corners
    [_c(8, 8), _c(12, 16), _c(16, 24), _c(20, 32)],        # four on a diagonal line
    [_c(8, 32), _c(12, 24), _c(16, 16), _c(20, 8)],        # ... on an anti-diagonal line
    [_c(31, 31), _c(31, 32), _c(32, 31), _c(32, 32)],      # 2x2 block of adjacent cells
]


def moments_of_cells(cells):
    """Exact uv / cov (fp64; dyadic rationals) of equal weights on the given flat cells."""
    from tests.decode_ref import XX, YY
    u, v = XX[list(cells)], YY[list(cells)]
    mu, mv = u.mean(), v.mean()
    du, dv = u - mu, v - mv
    return np.array([mu, mv]), np.array([[(du * du).mean(), (du * dv).mean()], [(du * dv).mean(), (dv * dv).mean()]])


# ---- validity head --------------------------------------------------------------------------------------------------------------------------
def classifier_inputs():
    """float32 mean logits [7,41]: every scale the head can see.  Negative entries (the relu clamps them), exact 0.0 and -0.0, and rows large
    enough that the outputs pass |a| = 100 (the sigmoid must saturate to exactly 0 or 1)."""
    rng = np.random.default_rng(103)
    m = rng.standard_normal((7, NUM_KP))
    m[0] *= 0.1
    m[1] *= 3.0
    m[2] = np.abs(m[2]) * 5.0                      # all positive
    m[3] = -np.abs(m[3]) * 5.0                     # all negative: the output is the bias
    m[4] *= 300.0                                  # |a| > 100
    m[5] *= 3000.0
    m[6] *= 10.0
    m[0, ::5], m[1, ::7], m[6, 1::4] = 0.0, -0.0, 0.0
    m[6, 2::4] = -0.0
    return m.astype(np.float32)


def classifier_weights(name, state_dict):
    if name == "classifier_checkpoint":
        return np.asarray(state_dict["classifier.2.weight"], np.float32), np.asarray(state_dict["classifier.2.bias"], np.float32)
    rng = np.random.default_rng(104)
    return rng.standard_normal((NUM_KP, NUM_KP)).astype(np.float32), rng.standard_normal(NUM_KP).astype(np.float32)


CLASSIFIER_FAMILIES = ("classifier_checkpoint", "classifier_random")


# ---- masks at the thresholds ----------------------------------------------------------------------------------------------------------------
THRESHOLDS = ((0.9, 0.2), (1.0, 0.5), (0.85, 0.13))       # evaluate.py's two sets, and an awkward pair


def _near(x):
    x = np.float32(x)
    return [np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))]


def largest_variance_below(vt):
    """The largest float32 c with np.sqrt(c) < float32(2*vt), by search: pins the rounding of sqrtf and the conversion of the threshold."""
    t = np.float32(2 * vt)
    c = np.float32(t * t)
    while not np.sqrt(c) < t:
        c = np.nextafter(c, np.float32(0))
    while np.sqrt(np.nextafter(c, np.float32(np.inf))) < t:
        c = np.nextafter(c, np.float32(np.inf))
    return c


def mask_cases(bt, vt):
    """-> uv [L,41,2], cov [L,41,2,2], kp [L,41] float32 and model_mask [L,41] uint8: every gate at its threshold with the other three held
    comfortably true (u = v = 0.1, variances 1e-4, kp 0.9, mask byte 1), then the non-finite fields.  Padded with comfortable entries to a
    whole number of crops."""
    base = dict(u=0.1, v=0.1, cxx=1e-4, cxy=0.0, cyy=1e-4, kp=0.9, mm=1)
    cases = [dict(base)]
    add = lambda **kw: cases.append({**base, **kw})
    for x in _near(0.3):
        add(kp=x)
    for comp in ("u", "v"):
        for edge in (bt, -bt):
            for x in _near(edge):
                add(**{comp: x})
    c = largest_variance_below(vt)
    for comp in ("cxx", "cyy"):
        for x in (np.nextafter(c, np.float32(0)), c, np.nextafter(c, np.float32(np.inf))):
            add(**{comp: x})
    for byte in (0, 1, 2, 255):
        add(mm=byte)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    for field in ("u", "v", "kp", "cxx", "cyy", "cxy"):
        for x in (nan, inf, -inf):
            add(**{field: x})
    add(u=nan, v=nan)
    add(u=nan, v=2.0)                      # the other component outside the box
    add(u=-2.0, v=nan)
    for comp in ("cxx", "cyy"):
        for x in (-1e-4, -1e-30, -0.0, 0.0, 1e-45):      # negative variance: sqrt = NaN masks it; both zeros and a denormal pass
            add(**{comp: x})
    add(cxx=-0.0, cyy=-0.0)
    L = -(-len(cases) // NUM_KP)
    cases += [dict(base)] * (L * NUM_KP - len(cases))
    f = lambda k: np.array([q[k] for q in cases], np.float32).reshape(L, NUM_KP)
    uv = np.stack([f("u"), f("v")], -1)
    cov = np.stack([np.stack([f("cxx"), f("cxy")], -1), np.stack([f("cxy"), f("cyy")], -1)], -2)
    mm = np.array([q["mm"] for q in cases], np.uint8).reshape(L, NUM_KP)
    return uv, cov, f("kp"), mm


# ---- error measures (see the module docstring) ----------------------------------------------------------------------------------------------
def decode_errors(got, ref):
    """got: uv / cov / mean_logit / prob arrays (any float type) of one family; ref: decode64 of the same logits -> {quantity: max error}."""
    with np.errstate(invalid="ignore"):
        dcov = np.abs(np.asarray(got["cov"], np.float64) - ref["cov"])
        scale = np.maximum(ref["cov"][..., 0, 0], ref["cov"][..., 1, 1])[..., None, None]
        dmean = np.abs(np.asarray(got["mean_logit"], np.float64) - ref["mean_logit"]) / np.maximum(1.0, np.abs(ref["mean_logit"]))
        dprob = np.abs(np.asarray(got["prob"], np.float64) - ref["prob"]) / ref["prob"].max((-1, -2), keepdims=True)
        return {"uv": float(np.abs(np.asarray(got["uv"], np.float64) - ref["uv"]).max()), "cov": float(dcov.max()),
                "cov_rel": float((dcov / scale).max()), "mean_logit": float(np.nan_to_num(dmean, nan=0.0).max()), "prob": float(dprob.max())}


def classifier_errors(got_logit, got_prob, m32, W, b, ref_logit, ref_prob):
    from tests.decode_ref import relu_keeps_nan
    scale = np.maximum(1.0, (np.abs(np.asarray(W, np.float64)) * relu_keeps_nan(m32)[..., None, :]).sum(-1) + np.abs(np.asarray(b, np.float64)))
    out = {"kp_prob": float((np.abs(np.asarray(got_prob, np.float64) - ref_prob) / scale).max())}
    if got_logit is not None:
        out["kp_logit"] = float((np.abs(np.asarray(got_logit, np.float64) - ref_logit) / scale).max())
    return out
