"""Per-site activation exponents of the two-term fp16 form (include/suo_hip.h: suo_net_calibrate; csrc/f16x2.h).

Wide-range weights: make_random_state_dict(0, 8.0) with every convolution redrawn N(0, 1) g / sqrt(fan_in) (tools/measure_activation_range.py's recipe).
Measured with the CPU oracle on this file's frame and its first two boxes: g = 1.1 -- the largest input of a 3x3 convolution is
backbone.Residual.3.conv2's, max |x| = 4813 (4.7x past the default 3x3 limit of 1023), of a 1x1 convolution backbone.tmpOut.1's, 6619 (limit 4094);
g = sqrt(2) (He) -- 7.2e9 at backbone.Residual.3.conv2, 1.4e10 at backbone.tmpOut.1.  Uncalibrated, either network leaves the fp16 range at s = 4 (the precondition each test asserts); calibrated, it stays on the fp16
form and its logits agree with a network built on the bf16x3 form (SUO_F16X2=0) at the gate of tests/test_gpu_f16x2.py, 1e-5 of their largest magnitude.
(Its uv / cov gate of 1e-5 holds for the seeded weights; logits of thousands make the soft-argmax follow their last bits on ANY form, so there the fp16
form is held to what separates the fp32 matrix pipe from bf16x3.)"""
import numpy as np
import pytest
import torch

from suo_slam_amd import _lib

pytestmark = pytest.mark.gpu

BOXES4 = np.array([[100, 80, 300, 290], [350.5, 100.25, 600, 400], [10, 200, 130, 330], [200, 150, 420, 330]], np.float32)
BOUND = 65504.0 / 16


def _frame(seed=4):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0, 1, (480, 640, 3)) * 255).astype(np.uint8)


def _wide_sd(gain):
    from suo_slam_amd import weights
    sd = dict(weights.make_random_state_dict(seed=0, logit_gain=8.0))
    rng = np.random.default_rng(1000)
    for k, v in sd.items():
        if k.endswith(".weight") and v.ndim == 4:
            sd[k] = (rng.standard_normal(v.shape) * gain / np.sqrt(int(np.prod(v.shape[1:])))).astype(np.float32)
    return sd


def _seeded_sd():
    from suo_slam_amd import weights
    return weights.make_random_state_dict(seed=0, logit_gain=8.0)


def _net(sd, max_crops, monkeypatch, pipe=2):
    from suo_slam_amd.pkpnet import PkpNet
    for k in ("SUO_F16X2", "SUO_WINO_BF16X3"):
        monkeypatch.delenv(k, raising=False)
    if pipe == 1:
        monkeypatch.setenv("SUO_F16X2", "0")
    if pipe == 0:
        monkeypatch.setenv("SUO_WINO_BF16X3", "0")
    net = PkpNet(state_dict=sd, max_crops=max_crops)
    for k in ("SUO_F16X2", "SUO_WINO_BF16X3"):
        monkeypatch.delenv(k, raising=False)
    assert net.pipe() == pipe
    return net


def _run(net, img, boxes):
    """One blocking call (the C entry checks its own call and re-issues an invalid one on bf16x3 by itself): (outputs as numpy, whether it was re-issued)."""
    before = net.last_call()
    out = net(img, [torch.from_numpy(boxes)], None)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, net.last_call() - before > 1


def _agree(o, ref, uv_cov=True):
    scale = np.abs(ref["prob_logits"]).max()
    assert np.isfinite(o["prob_logits"]).all()
    err = np.abs(o["prob_logits"] - ref["prob_logits"]).max()
    assert err <= 1e-5 * scale, (err, scale)
    if uv_cov:
        assert np.abs(o["uv"] - ref["uv"]).max() <= 1e-5 and np.abs(o["cov"] - ref["cov"]).max() <= 1e-5


def _rule(amax, ksize):
    import ctypes as C
    out = C.c_int()
    _lib.check(_lib.lib().suo_f16x2_shift_for(float(amax), ksize, C.byref(out)), "suo_f16x2_shift_for")
    return out.value


def _oracle_conv_inputs(sd, img, boxes):
    """The CPU oracle's max |input| per convolution (tools/measure_activation_range.py's _conv spy) and its logits, prior-less crops."""
    from oracle import cnn_oracle as O
    P = O.to_torch(sd)
    crops = torch.from_numpy(O.roi_align(O.image_to_chw(img), boxes))
    x = torch.cat([crops, torch.zeros(crops.shape[0], 41, 256, 256)], 1)
    rec = {}
    orig = O._conv

    def spy(x_, P_, p, stride=1, padding=0):
        rec[p] = (int(P_[p + ".weight"].shape[-1]), float(x_.abs().max()))
        return orig(x_, P_, p, stride, padding)

    O._conv = spy
    try:
        with torch.no_grad():
            logits = O.hourglass_net(x, P).numpy()
    finally:
        O._conv = orig
    return rec, logits


@pytest.mark.parametrize("gain", [1.1, float(np.sqrt(2.0))])
def test_wide_range_weights_stay_on_the_fp16_form_after_calibration(monkeypatch, gain):
    sd = _wide_sd(gain)
    img = _frame()
    boxes = np.tile(BOXES4, (10, 1))                                        # 40 crops: the large-launch kernels
    net = _net(sd, 40, monkeypatch)
    _, reissued = _run(net, img, boxes)
    assert reissued and net.pipe() == 1                                     # precondition: s = 4 cannot hold these activations
    shifts = net.calibrate(img, [boxes[:8]])
    assert net.pipe() == 2 and len(shifts) == len(net.f16x2_sites()) and min(shifts.values()) < 4
    o16, reissued = _run(net, img, boxes)
    assert not reissued and net.pipe() == 2 and not net.range_exceeded()
    o3, _ = _run(_net(sd, 40, monkeypatch, pipe=1), img, boxes)
    _agree(o16, o3, uv_cov=False)
    if gain < 1.2:
        # uv / cov: logits of thousands make the soft-argmax sensitive to their last bits whatever the form -- the fp16 form is held to what separates the
        # fp32 matrix pipe from bf16x3 on the same weights
        o0, _ = _run(_net(sd, 40, monkeypatch, pipe=0), img, boxes)
        for k in ("uv", "cov"):
            assert np.abs(o16[k] - o3[k]).max() <= max(1e-5, 4 * np.abs(o0[k] - o3[k]).max()), k
        _, lo = _oracle_conv_inputs(sd, img, boxes[:2])                    # and the CPU oracle's logits, two crops
        assert np.abs(o16["prob_logits"][:2] - lo).max() <= 1e-5 * np.abs(lo).max()


def test_every_site_measured_and_the_rule_matches_the_oracle(monkeypatch):
    """One site per convolution with fp16 planes -- every conv of the network except the image stem, the 64-wide r4.conv1 (fp32-pipe GEMM only), conv4 (the
    second K segment of its block's conv3 site) and tmpOut_.0 (folded with ll_.0 into the re-injection GEMM, site ll_.0) -- and s = the rule applied to the CPU
    oracle's max |input| of that convolution."""
    sd = _wide_sd(1.1)
    img = _frame()
    boxes = BOXES4[:2].copy()
    net = _net(sd, 8, monkeypatch)
    shifts = net.calibrate(img, [boxes])
    names = net.f16x2_sites()
    assert len(set(names)) == len(names) == len(shifts)
    rec, _ = _oracle_conv_inputs(sd, img, boxes)
    expect = {p for p in rec if p not in ("backbone.conv1_", "backbone.r4.conv1", "backbone.tmpOut_.0") and not p.endswith(".conv4")}
    assert set(names) == expect, set(names) ^ expect
    for name in names:
        ks, m = rec[name]
        conv4 = name[:-len("conv3")] + "conv4"
        if name.endswith(".conv3") and conv4 in rec:
            m = max(m, rec[conv4][1])
        want = _rule(m, ks)
        if shifts[name] != want:
            k = 4.0 if ks == 3 else 1.0
            edge = BOUND / k / 2.0 ** want                                  # the max at which the rule steps from want to want - 1
            near = min(abs(m - edge), abs(m - edge / 2)) <= 1e-4 * m
            assert near and abs(shifts[name] - want) == 1, (name, m, shifts[name], want)


def test_captured_graphs_read_the_calibrated_factors(monkeypatch):
    sd = _wide_sd(1.1)
    img = _frame()
    boxes = np.tile(BOXES4, (2, 1))
    net = _net(sd, 8, monkeypatch)
    net.prepare(crop_counts=[8], with_priors=(False,))                     # graphs captured BEFORE calibration: they bake the factor pointers
    net.calibrate(img, [boxes])
    og, reissued = _run(net, img, boxes)
    assert not reissued and net.pipe() == 2
    net.set_graph(False)
    oe, reissued = _run(net, img, boxes)
    assert not reissued
    for k in og:
        assert np.array_equal(og[k], oe[k]), k


def test_shifts_round_trip_and_the_default_is_bit_identical(monkeypatch):
    sd = _seeded_sd()
    img = _frame()
    boxes = np.tile(BOXES4, (10, 1))
    a = _net(sd, 40, monkeypatch)
    assert set(a.f16x2_shifts().values()) == {4}
    shifts = a.calibrate(img, [boxes[:4]])
    assert min(shifts.values()) > 4                                          # (the seeded weights leave >= 195x of headroom at s = 4)
    oa, reissued = _run(a, img, boxes)
    assert not reissued
    b = _net(sd, 40, monkeypatch)
    b.set_f16x2_shifts(shifts)
    assert b.f16x2_shifts() == shifts
    ob, reissued = _run(b, img, boxes)
    assert not reissued
    for k in oa:
        assert np.array_equal(oa[k], ob[k]), k
    b.set_f16x2_shifts({n: 4 for n in shifts})
    c = _net(sd, 40, monkeypatch)                                            # never calibrated
    oc, _ = _run(c, img, boxes)
    ob4, _ = _run(b, img, boxes)
    for k in oc:
        assert np.array_equal(ob4[k], oc[k]), k
    with pytest.raises(ValueError):
        b.set_f16x2_shifts({n: 4 for n in list(shifts)[1:]})
    with pytest.raises(_lib.SuoError):
        b.set_f16x2_shifts({n: 27 for n in shifts})
    assert b.f16x2_shifts() == {n: 4 for n in shifts}                        # (a refused set changes nothing)


@pytest.mark.parametrize("L", [40, 16])
def test_calibrated_seeded_network_meets_the_reference_goldens(cnn_golden, state_dict, monkeypatch, L):
    """tests/test_gpu_cnn.py::test_full_network_golden_on_the_winograd_path's gates, fp16 form, after calibration."""
    from suo_slam_amd.pkpnet import decode_extras
    from tests.gpu_backbone import run_backbone_from_staged
    net = _net(state_dict, L, monkeypatch)
    shifts = net.calibrate(_frame(), [BOXES4])
    assert min(shifts.values()) > 4
    rng = np.random.Generator(np.random.PCG64(int(cnn_golden["backbone_in_seed"])))
    x = rng.uniform(0, 1, (1, 44, 256, 256)).astype(np.float32)
    xin = np.zeros((L, 256, 256, 48), np.float32)
    xin[..., :44] = x.transpose(0, 2, 3, 1)
    ref = cnn_golden["backbone_logits"]
    logits = run_backbone_from_staged(net, xin)
    assert not net.range_exceeded() and net.pipe() == 2
    assert np.abs(logits - ref).max() / np.abs(ref).max() < 1e-5
    dec = decode_extras(torch.from_numpy(logits[:2]).cuda())
    assert np.abs(dec["uv"].cpu().numpy() - cnn_golden["backbone_uv"]).max() < 1e-5
    assert np.abs(dec["cov"].cpu().numpy() - cnn_golden["backbone_cov"]).max() < 1e-5


def test_range_guard_still_fires_past_the_calibrated_range(monkeypatch):
    """Calibrated on the uint8 frame; the same frame as SUO_IMG_F32_CHW holding raw 0-255 values (255x what the network was calibrated on; the stem's own
    operand 255 x 16 stays below 4094) drives the calibrated sites far past their range: the call is flagged, the network falls back, the re-issued call
    equals the bf16x3 network's."""
    sd = _seeded_sd()
    img = _frame()
    boxes = np.tile(BOXES4, (10, 1))
    net = _net(sd, 40, monkeypatch)
    net.calibrate(img, [boxes[:4]])
    raw = torch.from_numpy(img.transpose(2, 0, 1)[None].astype(np.float32))
    o16, reissued = _run(net, raw, boxes)
    assert reissued and net.pipe() == 1
    o3, _ = _run(_net(sd, 40, monkeypatch, pipe=1), raw, boxes)
    for k in o3:
        assert np.isfinite(o3[k]).all() and np.array_equal(o16[k], o3[k]), k


def test_bench_shape_after_calibration_on_one_frame(monkeypatch):
    """Calibrated on one frame of 8 crops, then 32 frames x 8 crops in one forward_frames call (the headline's shape): flag down, bf16x3's results."""
    sd = _wide_sd(1.1)
    frames = np.stack([_frame(100 + i) for i in range(32)])
    boxes8 = np.concatenate([BOXES4, BOXES4 + np.float32(20)])
    net = _net(sd, 256, monkeypatch)
    net.calibrate(frames[:1], [boxes8])
    assert net.pipe() == 2

    def run(n):
        before = n.last_call()
        out = n.forward_frames(frames, [boxes8] * 32)
        torch.cuda.synchronize()
        return {k: out[k].cpu().numpy() for k in ("prob_logits", "uv", "cov")}, n.last_call() - before > 1

    o16, reissued = run(net)
    assert not reissued and net.pipe() == 2 and not net.range_exceeded()
    o3, _ = run(_net(sd, 256, monkeypatch, pipe=1))
    _agree(o16, o3, uv_cov=False)                                            # (uv / cov of these weights: see the 40-crop test)
