"""The LDS-DMA Winograd kernels' fused tail with the up-sampled addend fetches its skip rows by LDS-DMA, one epilogue block ahead (csrc/conv_wino_x3_kernel.h:
SKD; SUO_WINO_SKIP_DMA=0 keeps the register loads).  The two paths add the same 16 bytes to the same sums in the same order, so every output and the range flag
must agree BIT FOR BIT: on maps whose tiles leave the map (there a lane's slot holds another block's row and must count as zero), on maps smaller than a
tile, between crops, with inf / NaN in the skip, and when the launch before left huge values behind.  The plain tail and the tail with the next block's conv1
have one path only (the switch must not touch them): they run through the same cases."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 16),        # one tile
          (3, 20, 24),       # tiles leave the map on both axes; three crops, the outer two with 1e4-sized skip and input
          (2, 16, 32),       # interior tiles
          (1, 4, 8),         # a map smaller than a tile
          (2, 32, 48)]       # 24 workgroups
FORMS = ["tail", "tail_up", "tail_next"]


@pytest.fixture(scope="module")
def ops():
    from suo_slam_amd import _lib
    _lib.require_gpu()
    from tests import hipops
    return hipops


def _weights(seed):
    rng = np.random.default_rng(seed)
    return dict(w2=(rng.standard_normal((128, 128, 3, 3)) / np.sqrt(9 * 128)).astype(np.float32), b2=(rng.standard_normal(128) * 0.3).astype(np.float32),
                w3=(rng.standard_normal((256, 128)) / np.sqrt(128)).astype(np.float32), b3=rng.standard_normal(256).astype(np.float32),
                ns=rng.uniform(0.5, 1.5, 256).astype(np.float32), nt=(rng.standard_normal(256) * 0.3).astype(np.float32),
                w1=(rng.standard_normal((128, 256)) / 16).astype(np.float32), b1=(rng.standard_normal(128) * 0.2).astype(np.float32))


def _inputs(L, H, W, huge_outer=True):
    rng = np.random.default_rng(2000 * L + 10 * H + W)
    x = rng.standard_normal((L, H, W, 128)).astype(np.float32)
    skip = rng.standard_normal((L, H, W, 256)).astype(np.float32)
    up = rng.standard_normal((L, H // 2, W // 2, 256)).astype(np.float32)
    if L == 3 and huge_outer:                                              # the middle crop O(1), its neighbours huge: a skip row fetched across a crop end would show
        for t in (x, skip, up):
            t[0] *= np.float32(1e4)
            t[2] *= np.float32(1e4)
    return torch.from_numpy(x).cuda(), torch.from_numpy(skip).cuda(), torch.from_numpy(up).cuda()


def _run(ops, form, x, skip, up, w):
    """-> ([outputs], flag) of one form of the fused tail"""
    if form == "tail":
        o, f = ops.conv3x3_wino_f16x2_conv1x1_skip_up(x, w["w2"], w["b2"], w["w3"], w["b3"], skip)
        return [o], f
    if form == "tail_up":
        o, f = ops.conv3x3_wino_f16x2_conv1x1_skip_up(x, w["w2"], w["b2"], w["w3"], w["b3"], skip, up)
        return [o], f
    assert form == "tail_next"
    o, n, f = ops.conv3x3_wino_f16x2_tail_next(x, w["w2"], w["b2"], w["w3"], w["b3"], skip, None, (w["ns"], w["nt"]), w["w1"], w["b1"])
    return [o, n], f


def _path(monkeypatch, skip_dma):
    monkeypatch.setenv("SUO_WINO_W8", "0")                                  # the four-wave form at every launch size
    monkeypatch.setenv("SUO_WINO_HALO_DMA", "1")
    monkeypatch.setenv("SUO_WINO_SKIP_DMA", "1" if skip_dma else "0")


def _both(ops, monkeypatch, form, x, skip, up, w):
    _path(monkeypatch, False)
    reg = _run(ops, form, x, skip, up, w)
    _path(monkeypatch, True)
    dma = _run(ops, form, x, skip, up, w)
    return reg, dma


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("L,H,W", SHAPES)
def test_skip_dma_equals_register_loads_bit_for_bit(ops, monkeypatch, form, L, H, W):
    x, skip, up = _inputs(L, H, W)
    w = _weights(11)
    (reg, freg), (dma, fdma) = _both(ops, monkeypatch, form, x, skip, up, w)
    assert fdma == freg == (1 if L == 3 else 0)                             # (1e4 x 2^4 is beyond fp16: the huge crops raise the flag in both paths)
    for r, d in zip(reg, dma):
        if L != 3:
            assert torch.isfinite(d).all() and torch.equal(r, d)
        assert _same_bits(r, d)
    if L == 3:
        # the middle crop has not seen its neighbours' rows: launched alone it gives the same bits, flag down
        alone, falone = _run(ops, form, x[1:2].contiguous(), skip[1:2].contiguous(), up[1:2].contiguous(), w)
        assert falone == 0
        for a, d in zip(alone, dma):
            assert torch.isfinite(d[1]).all() and torch.equal(a[0], d[1])


@pytest.mark.parametrize("form", FORMS)
def test_inf_and_nan_of_the_skip_pass_through_and_stay_in_their_crop(ops, monkeypatch, form):
    L, H, W = 2, 16, 32
    x, skip, up = _inputs(L, H, W)
    w = _weights(11)
    _path(monkeypatch, True)
    clean, fclean = _run(ops, form, x, skip, up, w)
    assert fclean == 0
    bad_s, bad_u = skip.clone(), up.clone()
    special = torch.tensor([0x7F800000, -0x00800000, 0x7FC12345, -0x003FFFFF], dtype=torch.int32, device="cuda").view(torch.float32)      # +inf, -inf, two NaN payloads
    sites = [(0, 0, 0), (0, 7, 16), (0, 15, 31), (0, 8, 5)]                 # (crop 0) a tile's first pixel, a tile boundary, the map's last pixel, both passes' rows
    for q, (l, y, xx) in enumerate(sites):
        bad_s[l, y, xx, 37 * q: 37 * q + 4] = special
    if form == "tail_up":
        bad_u[0, 3, 9, 200:204] = special
    (reg, freg), (dma, fdma) = _both(ops, monkeypatch, form, x, bad_s, bad_u, w)
    assert fdma == freg
    for r, d, c in zip(reg, dma, clean):
        assert _same_bits(r, d)
        assert _same_bits(d[1], c[1])                                       # the neighbouring crop: as without them
    out = dma[0]
    for q, (l, y, xx) in enumerate(sites):                                  # a finite sum plus the skip's special value is that value (NaN stays NaN)
        got = out[l, y, xx, 37 * q: 37 * q + 4]
        assert _same_bits(got[:2], special[:2]) and torch.isnan(got[2:]).all()
    if form == "tail_up":
        got = out[0, 6:8, 18:20, 200:204]                                   # the four pixels above the up-sampled source pixel
        assert _same_bits(got[..., :2], special[:2].expand(2, 2, 2)) and torch.isnan(got[..., 2:]).all()
    else:
        untouched = torch.ones_like(out[0], dtype=torch.bool)
        for q, (l, y, xx) in enumerate(sites):
            untouched[y, xx, 37 * q: 37 * q + 4] = False
        assert _same_bits(out[0][untouched], clean[0][0][untouched])        # `out` elsewhere in the crop: as without them


@pytest.mark.parametrize("form", ["tail_next", "tail_up"])
@pytest.mark.parametrize("L,H,W", [(1, 4, 8), (3, 20, 24)])
def test_lanes_outside_the_map_count_as_zero_after_a_huge_launch(ops, monkeypatch, form, L, H, W):
    """A lane whose pixel is outside the map reads a slot that holds some other row, or what the launch before left there: it must add zero, in `out`, in the next
    block's operand and in the range guard's maximum."""
    w = _weights(11)
    x, skip, up = _inputs(L, H, W, huge_outer=False)
    _path(monkeypatch, False)
    reg, freg = _run(ops, form, x, skip, up, w)
    assert freg == 0
    bx, bskip, bup = _inputs(2, 16, 32)
    _path(monkeypatch, True)
    _, fbig = _run(ops, form, bx * 1e4, bskip * 1e4, bup * 1e4, w)
    assert fbig == 1
    dma, fdma = _run(ops, form, x, skip, up, w)
    assert fdma == 0
    for r, d in zip(reg, dma):
        assert torch.isfinite(d).all() and _same_bits(r, d)
