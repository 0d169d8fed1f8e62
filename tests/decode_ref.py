"""Plain fp64 restatement (numpy only) of the tail of the network: spatial soft-max, post_process_kp with its two-pass covariance and the
validity head in eval mode (lib/models/pkpnet.py:13-63, 74-78, 116-118), and the keypoint masks of lib/object_slam.py:1100-1115.

decode64 / classifier64 are the high-precision yardstick of tests/test_gpu_decode_edges.py; masks_ref is the reference's numpy rule on float32
arrays.  tests/test_decode_ref.py pins all three to what the reference program recorded (tests/golden/cnn_golden.npz) and to
oracle.cnn_oracle, so the GPU tests do not rest on an unpinned restatement.

Non-finite values follow the reference's libraries: np.max / torch.max propagate NaN into the soft-max (one NaN, one +inf or an all -inf map
make the whole map NaN; a block of -inf cells among finite ones does not), relu keeps NaN, argmax counts NaN as the maximum."""
import numpy as np

HEAT = 64
NUM_KP = 41
R = (np.arange(HEAT, dtype=np.float64) + 0.5) / (HEAT / 2) - 1          # mesh_grid: r[i] = (i + 0.5) / 32 - 1
XX = np.repeat(R[:, None], HEAT, 1).reshape(-1)                         # u from the row ...
YY = np.repeat(-R[None, :], HEAT, 0).reshape(-1)                        # ... v from the negated column


def argmax_torch(x):
    """torch.argmax over the last axis: the first maximum, and NaN counts as the maximum (the first NaN wins)."""
    x = np.asarray(x)
    nan = np.isnan(x)
    with np.errstate(invalid="ignore"):
        first_max = np.argmax(np.where(nan, -np.inf, x), -1)
    return np.where(nan.any(-1), np.argmax(nan, -1), first_max).astype(np.int32)


def top2_gap(x):
    """Largest minus second largest value over the last axis (0 = the argmax is a tie)."""
    s = np.sort(np.asarray(x, np.float64), -1)
    with np.errstate(invalid="ignore"):
        return s[..., -1] - s[..., -2]


def decode64(logits_f32):
    """float32 logits [L,K,64,64], widened to fp64 as given -> dict of uv [L,K,2], cov [L,K,2,2], prob [L,K,64,64], mean_logit [L,K] (fp64)
    and argmax [L,K] (int32, flat h*64+w)."""
    x = np.asarray(logits_f32)
    assert x.dtype == np.float32 and x.shape[-2:] == (HEAT, HEAT)
    lead = x.shape[:-2]
    x = x.astype(np.float64).reshape(lead + (HEAT * HEAT,))
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(x - x.max(-1, keepdims=True))                         # np.max propagates NaN, as torch's soft-max does
        p = e / e.sum(-1, keepdims=True)
        u, v = (p * XX).sum(-1), (p * YY).sum(-1)
        dx, dy = XX - u[..., None], YY - v[..., None]                    # two-pass covariance about the mean (pkpnet.py:53-57)
        cxx, cxy, cyy = (p * dx * dx).sum(-1), (p * dx * dy).sum(-1), (p * dy * dy).sum(-1)
        mean = x.mean(-1)
    cov = np.stack([np.stack([cxx, cxy], -1), np.stack([cxy, cyy], -1)], -2)
    return {"uv": np.stack([u, v], -1), "cov": cov, "prob": p.reshape(lead + (HEAT, HEAT)), "mean_logit": mean, "argmax": argmax_torch(x)}


def relu_keeps_nan(m):
    m = np.asarray(m, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(m < 0, 0.0, m)


def classifier64(mean_logit, W, b):
    """sigmoid(W relu(mean_logit) + b) in fp64 -> (logits, probabilities), [L,K] each."""
    m = relu_keeps_nan(mean_logit)
    with np.errstate(invalid="ignore", over="ignore"):
        a = (m[..., None, :] * np.asarray(W, np.float64)).sum(-1) + np.asarray(b, np.float64)
        return a, 1.0 / (1.0 + np.exp(-a))


def masks_ref(uv32, cov32, kp32, model_mask, bt, vt):
    """object_slam.py:1100-1115 verbatim on float32 arrays; bt / vt are Python floats as the reference's attributes are.  model_mask: None
    (= all true) or anything whose non-zero entries are true (the reference's is a bool array)."""
    exp_uv, cov_uv, kp = np.asarray(uv32), np.asarray(cov32), np.asarray(kp32)
    assert exp_uv.dtype == cov_uv.dtype == kp.dtype == np.float32
    bt, vt = float(bt), float(vt)
    mm = np.ones(kp.shape, bool) if model_mask is None else np.asarray(model_mask) != 0
    with np.errstate(invalid="ignore"):
        kp_masks = (kp > 0.3) & mm
        kp_masks = kp_masks & (np.min(exp_uv, -1) > -bt) & (np.max(exp_uv, -1) < bt)
        std = np.sqrt(cov_uv[..., [0, 1], [0, 1]])
        kp_masks = kp_masks & np.all(std < 2 * vt, axis=-1)
    return kp_masks
