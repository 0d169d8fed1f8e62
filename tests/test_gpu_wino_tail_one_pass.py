"""The LDS-DMA Winograd kernels' tail with the next block's conv1 runs its 1x1 stages in ONE pass over the 128-pixel tile (csrc/conv_wino_x3_kernel.h: ONEP;
SUO_WINO_TAIL_ONE_PASS=0 keeps the two passes of 64 pixels).  Both forms build every output element as the same sum of the same products in ascending k, with
the same scale / bias / skip / next-prologue arithmetic, and the range guard sees the same values: every output and the range flag must agree BIT FOR BIT -- on
one full tile, on a ragged map (partial tiles, rows outside the map in a block's second patch round, a crop boundary), on a map of several tiles, at site
shifts other than 4, and when the flag is raised.  The plain tail has one form only (built in one pass too, it did not gain: profiles/REJECTED.md) -- the switch
must not touch it: it runs through the same cases.  The switch is read when a launch is issued (like SUO_WINO_HALO_DMA, and as tests/test_gpu_wino_skip_dma.py
switches its path), so one process runs both forms."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 16),        # one full tile
          (2, 9, 17),        # ragged: four tiles a crop, three of them partial; two crops
          (1, 16, 32)]       # four full tiles
FORMS = ["tail", "tail_next"]


@pytest.fixture(scope="module")
def ops():
    from suo_slam_amd import _lib
    _lib.require_gpu()
    from tests import hipops
    return hipops


@pytest.fixture(scope="module")
def weights():
    rng = np.random.default_rng(23)
    return dict(w2=(rng.standard_normal((128, 128, 3, 3)) / np.sqrt(9 * 128)).astype(np.float32), b2=(rng.standard_normal(128) * 0.3).astype(np.float32),
                w3=(rng.standard_normal((256, 128)) / np.sqrt(128)).astype(np.float32), b3=rng.standard_normal(256).astype(np.float32),
                ns=rng.uniform(0.5, 1.5, 256).astype(np.float32), nt=(rng.standard_normal(256) * 0.3).astype(np.float32),
                w1=(rng.standard_normal((128, 256)) / 16).astype(np.float32), b1=(rng.standard_normal(128) * 0.2).astype(np.float32))


def _inputs(L, H, W, gain=1.0):
    rng = np.random.default_rng(3000 * L + 10 * H + W)
    x = (rng.standard_normal((L, H, W, 128)) * gain).astype(np.float32)
    skip = (rng.standard_normal((L, H, W, 256)) * gain).astype(np.float32)
    return torch.from_numpy(x).cuda(), torch.from_numpy(skip).cuda()


def _run(ops, form, x, skip, w):
    """-> ([outputs], flag) of one form of the fused tail"""
    if form == "tail":
        o, f = ops.conv3x3_wino_f16x2_conv1x1_skip_up(x, w["w2"], w["b2"], w["w3"], w["b3"], skip)
        return [o], f
    o, n, f = ops.conv3x3_wino_f16x2_tail_next(x, w["w2"], w["b2"], w["w3"], w["b3"], skip, None, (w["ns"], w["nt"]), w["w1"], w["b1"])
    return [o, n], f


def _both(ops, monkeypatch, form, x, skip, w):
    monkeypatch.setenv("SUO_WINO_W8", "0")                                  # the four-wave form at every launch size
    monkeypatch.setenv("SUO_WINO_HALO_DMA", "1")
    monkeypatch.setenv("SUO_WINO_TAIL_ONE_PASS", "0")
    two = _run(ops, form, x, skip, w)
    monkeypatch.setenv("SUO_WINO_TAIL_ONE_PASS", "1")
    one = _run(ops, form, x, skip, w)
    return two, one


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("L,H,W", SHAPES)
def test_one_pass_equals_two_passes_bit_for_bit(ops, monkeypatch, weights, form, L, H, W):
    x, skip = _inputs(L, H, W)
    (two, ftwo), (one, fone) = _both(ops, monkeypatch, form, x, skip, weights)
    assert fone == ftwo == 0
    for t, o in zip(two, one):
        assert torch.isfinite(o).all() and _same_bits(t, o)
    assert float(one[0].abs().max()) > 1.0                                  # (not an empty comparison)
    if form == "tail_next":
        assert float(one[1].max()) > 0.1 and float(one[1].min()) == 0.0     # conv1's ReLU output: every element written (the buffer starts at -7)


@pytest.mark.parametrize("form", FORMS)
def test_one_pass_equals_two_passes_at_other_site_shifts(ops, monkeypatch, weights, form):
    """Sites of conv2's, conv3's and the next conv1's inputs at 2^3, 2^6, 2^2 instead of 2^4 (suo_debug_f16x2_stage_sites), on the ragged map."""
    x, skip = _inputs(2, 9, 17)
    with ops.sites(in_=3, inner=6, next=2):
        (two, ftwo), (one, fone) = _both(ops, monkeypatch, form, x, skip, weights)
    assert fone == ftwo == 0
    for t, o in zip(two, one):
        assert torch.isfinite(o).all() and _same_bits(t, o)
    (_, f4), (ref, _) = _both(ops, monkeypatch, form, x, skip, weights)     # the shifts took effect: at the default sites the same call stores other bits
    assert f4 == 0 and not _same_bits(one[0], ref[0])


@pytest.mark.parametrize("form", FORMS)
def test_range_flag_is_raised_alike(ops, monkeypatch, weights, form):
    """1e4-sized activations times 2^4 leave fp16's range: both forms raise the flag, and what they store is still the same bits."""
    x, skip = _inputs(2, 9, 17, gain=1e4)
    (two, ftwo), (one, fone) = _both(ops, monkeypatch, form, x, skip, weights)
    assert fone == ftwo == 1
    for t, o in zip(two, one):
        assert _same_bits(t, o)
    xs, ss = _inputs(2, 9, 17)                                              # and the flag is the launch's own: the same map in range leaves it down
    (_, f0), (_, f1) = _both(ops, monkeypatch, form, xs, ss, weights)
    assert f0 == f1 == 0
