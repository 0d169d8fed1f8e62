"""The four-wave fp16 Winograd kernels stage their halo by LDS-DMA (csrc/conv_wino_x3.hip: DMA; SUO_WINO_HALO_DMA=0 keeps the register-staged path).  The two
paths form the same sums of the same products in the same order -- the exact factor 2^s moves from the staged elements to the transform's first differences,
which commutes with the rounding -- so every output and the range flag must agree BIT FOR BIT, on maps whose tiles leave the map, whose halo is entirely
outside it, which are smaller than a tile, and between crops (a halo row of one crop is never its neighbour's first row)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 16),        # one tile, every halo pixel outside the map
          (3, 20, 24),       # tiles leave the map on both axes; three crops, the outer two filled with 1e4-sized values
          (2, 16, 32),       # interior tiles
          (1, 4, 8)]         # a map smaller than a tile


@pytest.fixture(scope="module")
def ops():
    from suo_slam_amd import _lib
    _lib.require_gpu()
    from tests import hipops
    return hipops


def _weights(seed, C=128):
    rng = np.random.default_rng(seed)
    w = dict(w2=(rng.standard_normal((C, C, 3, 3)) / np.sqrt(9 * C)).astype(np.float32), b2=(rng.standard_normal(C) * 0.3).astype(np.float32),
             w3=(rng.standard_normal((256, 128)) / np.sqrt(128)).astype(np.float32), b3=rng.standard_normal(256).astype(np.float32),
             ns=rng.uniform(0.5, 1.5, 256).astype(np.float32), nt=(rng.standard_normal(256) * 0.3).astype(np.float32),
             w1=(rng.standard_normal((128, 256)) / 16).astype(np.float32), b1=(rng.standard_normal(128) * 0.2).astype(np.float32))
    return w


def _inputs(L, H, W, C=128):
    rng = np.random.default_rng(1000 * L + 10 * H + W)
    x = rng.standard_normal((L, H, W, C)).astype(np.float32)
    if L == 3:                                                             # the middle crop O(1), its neighbours huge: a halo that crossed a crop end would show
        x[0] *= np.float32(1e4)
        x[2] *= np.float32(1e4)
    skip = rng.standard_normal((L, H, W, 256)).astype(np.float32)
    up = rng.standard_normal((L, H // 2, W // 2, 256)).astype(np.float32)
    return torch.from_numpy(x).cuda(), torch.from_numpy(skip).cuda(), torch.from_numpy(up).cuda()


def _run(ops, form, x, skip, up, w):
    """-> ([outputs], flag) of one form of the kernel"""
    if form == "plain":
        o, f = ops.conv3x3_wino_f16x2(x, w["w2"], w["b2"], relu=True)
        return [o], f
    if form == "tail":
        o, f = ops.conv3x3_wino_f16x2_conv1x1_skip_up(x, w["w2"], w["b2"], w["w3"], w["b3"], skip)
        return [o], f
    if form == "tail_up":
        o, f = ops.conv3x3_wino_f16x2_conv1x1_skip_up(x, w["w2"], w["b2"], w["w3"], w["b3"], skip, up)
        return [o], f
    assert form == "tail_next"
    o, n, f = ops.conv3x3_wino_f16x2_tail_next(x, w["w2"], w["b2"], w["w3"], w["b3"], skip, None, (w["ns"], w["nt"]), w["w1"], w["b1"])
    return [o, n], f


def _both(ops, monkeypatch, form, x, skip, up, w):
    monkeypatch.setenv("SUO_WINO_W8", "0")                                  # the four-wave form at every launch size
    monkeypatch.setenv("SUO_WINO_HALO_DMA", "0")
    reg = _run(ops, form, x, skip, up, w)
    monkeypatch.setenv("SUO_WINO_HALO_DMA", "1")
    dma = _run(ops, form, x, skip, up, w)
    return reg, dma


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))           # (bit patterns: the huge crops of the three-crop case may hold inf / NaN, equal in both paths)


@pytest.mark.parametrize("form", ["plain", "tail", "tail_up", "tail_next"])
@pytest.mark.parametrize("L,H,W", SHAPES)
def test_dma_form_equals_register_form_bit_for_bit(ops, monkeypatch, form, L, H, W):
    x, skip, up = _inputs(L, H, W)
    w = _weights(7)
    (reg, freg), (dma, fdma) = _both(ops, monkeypatch, form, x, skip, up, w)
    assert fdma == freg == (1 if L == 3 else 0)                             # (1e4 x 2^4 is beyond fp16: the huge crops raise the flag in both paths)
    for r, d in zip(reg, dma):
        if L != 3:
            assert torch.isfinite(d).all() and torch.equal(r, d)
        assert _same_bits(r, d)
    if L == 3:
        # the middle crop has not seen its neighbours: launched alone it gives the same bits, flag down
        monkeypatch.setenv("SUO_WINO_HALO_DMA", "1")
        alone, falone = _run(ops, form, x[1:2].contiguous(), skip[1:2].contiguous(), up[1:2].contiguous(), w)
        assert falone == 0
        for a, d in zip(alone, dma):
            assert torch.isfinite(d[1]).all() and torch.equal(a[0], d[1])


def test_dma_form_of_the_64_channel_kernel(ops, monkeypatch):
    x, _, _ = _inputs(1, 32, 32, C=64)
    w = _weights(9, C=64)
    (reg, freg), (dma, fdma) = _both(ops, monkeypatch, "plain", x, None, None, w)
    assert freg == 0 and fdma == 0
    assert torch.isfinite(dma[0]).all() and torch.equal(reg[0], dma[0])
    # and it is the convolution (fp64, the split forms' tolerance of tests/test_gpu_f16x2.py)
    import torch.nn.functional as F
    ref = F.relu(F.conv2d(x.cpu().permute(0, 3, 1, 2).double(), torch.from_numpy(w["w2"]).double(), torch.from_numpy(w["b2"]).double(), padding=1)).permute(0, 2, 3, 1)
    assert float((dma[0].cpu().double() - ref).abs().max()) < 5e-6 * float(ref.abs().max())


@pytest.mark.parametrize("where", ["map corner", "last channel chunk"])
@pytest.mark.parametrize("form", ["plain", "tail"])
def test_range_guard_sees_every_staged_element_in_both_forms(ops, monkeypatch, form, where):
    """One element of 2000 (x 2^4 x 4 is beyond the guard's limit) raises the flag in the launch that staged it, in both paths; without it the flag stays down."""
    L, H, W = 2, 16, 32
    x, skip, up = _inputs(L, H, W)
    w = _weights(7)
    (_, freg), (_, fdma) = _both(ops, monkeypatch, form, x, skip, up, w)
    assert freg == 0 and fdma == 0
    x = x.clone()
    if where == "map corner":
        x[L - 1, H - 1, W - 1, 3] = 2000.0                                  # the last pixel of the last crop: a halo element of one tile only
    else:
        x[0, 7, 16, 127] = -2000.0                                          # the last channel of the last chunk, on a tile boundary
    (_, freg), (_, fdma) = _both(ops, monkeypatch, form, x, skip, up, w)
    assert freg == 1 and fdma == 1
