"""csrc/res_small_x3.hip with mid1, mid2 and the output patch aliased inside the x tile: the fp16 form (NP = 2) now holds two workgroups on a CU,
each a tile of whatever crop the grid put there.  What can go wrong is a missing or misplaced barrier around the aliased regions and two
co-resident workgroups touching each other's tile.  A launch of more than 256 tiles is the first at which a CU holds two workgroups; a lone crop
(<= 32 tiles) never does, so a crop must come out of the big launch with the bits it has alone."""
import numpy as np
import pytest
import torch

from tests.test_gpu_res_block import _block_weights, _fp64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from suo_slam_amd import _lib
    _lib.require_gpu()
    from tests import hipops
    return hipops


def _run(ops, form, x, B, up=None, pool=False):
    """-> (out, range flag); the bf16x3 entry has no flag: 0."""
    args = (x, B["pro"], B["w1"], B["b1"], B["w2"], B["b2"], B["w3"], B["b3"])
    if form == "f16x2":
        return ops.res_block_f16x2(*args, up_nhwc=up, pool_in=pool)
    return ops.res_block_x3(*args, up_nhwc=up, pool_in=pool), 0


def _inputs(L, H, up, pool, seed):
    rng = np.random.default_rng(seed)
    B = _block_weights(rng)
    x = torch.from_numpy(rng.standard_normal((L, 2 * H, 2 * H, 256) if pool else (L, H, H, 256)).astype(np.float32)).cuda()
    low = torch.from_numpy(rng.standard_normal((L, H // 2, H // 2, 256)).astype(np.float32)).cuda() if up else None
    picks = sorted({0, L - 1, *(int(i) for i in rng.choice(np.arange(1, L - 1), 3, replace=False))})      # first, last, three seeded
    return B, x, low, picks


def _check_batch_invariance(ops, form, L, H, up, pool):
    B, x, low, picks = _inputs(L, H, up, pool, seed=L * 100 + H + 2 * up + pool)
    tiles = L * ((H + 3) // 4) * ((H + 7) // 8)
    assert tiles > 256 and len(picks) == 5                       # more tiles than CUs: some CU holds two workgroups of the fp16 form
    got, flag = _run(ops, form, x, B, low, pool)
    assert torch.isfinite(got).all()
    for i in picks:
        one, f1 = _run(ops, form, x[i:i + 1].contiguous(), B, low[i:i + 1].contiguous() if up else None, pool)
        assert torch.equal(got[i:i + 1], one), (i, float((got[i:i + 1] - one).abs().max()))
        assert f1 == flag == 0, (i, f1, flag)


# 8x8 x 144: 288 tiles, two per crop, ring rows partly inside the map; 4x4 x 288: half-empty tile, no ring; 16x16 x 40: 320 tiles, interior tiles
# with a full ring; then the 8x8 case with the 2x2 pool taken while staging, and with the up-sampled addend
@pytest.mark.parametrize("L,H,up,pool", [(144, 8, False, False), (288, 4, False, False), (40, 16, False, False), (144, 8, False, True), (144, 8, True, False)])
def test_f16x2_crop_in_a_two_per_cu_launch_equals_the_crop_alone(ops, L, H, up, pool):
    _check_batch_invariance(ops, "f16x2", L, H, up, pool)


@pytest.mark.parametrize("L,H", [(144, 8), (40, 16)])
def test_bf16x3_crop_in_a_big_launch_equals_the_crop_alone(ops, L, H):
    """Same LDS layout on three planes (101 376 B: one workgroup per CU)."""
    _check_batch_invariance(ops, "bf16x3", L, H, False, False)


def test_f16x2_range_flag_of_a_big_launch_equals_the_crops_alone(ops):
    """The flag with something to say: one input of the LAST crop beyond the fp16 form's range (prologue scale 1, shift 0).  The launch raises it, that
    crop alone raises it, the first crop alone does not -- and the first crop's output has the bits it has alone."""
    rng = np.random.default_rng(31)
    B = dict(_block_weights(rng), pro=(np.ones(256, np.float32), np.zeros(256, np.float32)))
    xg = rng.standard_normal((144, 8, 8, 256)).astype(np.float32)
    xg[143, 7, 7, 255] = 4095.0
    x = torch.from_numpy(xg).cuda()
    got, flag = _run(ops, "f16x2", x, B)
    first, f_first = _run(ops, "f16x2", x[:1].contiguous(), B)
    _, f_last = _run(ops, "f16x2", x[143:].contiguous(), B)
    assert (flag, f_first, f_last) == (1, 0, 1)
    assert torch.equal(got[:1], first)


@pytest.mark.parametrize("form,L,H", [("f16x2", 144, 8), ("bf16x3", 144, 8), ("bf16x3", 40, 16)])
def test_same_launch_five_times_same_bits(ops, form, L, H):
    """A race on the aliased tile shows as a run-to-run difference first.  Five launches, each into its own output buffer (all kept alive)."""
    B, x, _, _ = _inputs(L, H, False, False, seed=77 + H)
    outs = [_run(ops, form, x, B) for _ in range(5)]
    assert len({o.data_ptr() for o, _ in outs}) == 5
    for o, f in outs[1:]:
        assert torch.equal(o, outs[0][0]) and f == outs[0][1]


def test_f16x2_two_per_cu_launch_forward_error_per_element(ops):
    """The 8x8 x 144 launch against fp64 under the per-element gate of tests/test_gpu_res_block.py for the fp16 form: one-signed data (every partial
    result positive, so sum |.||.| IS the result), |err| <= 2 sqrt(K) 2^-24 of it with K = 256 + 1152 + 128 terms per output, never worse than
    1.5x the fp32-pipe kernel + 1.5, signed mean within 1.5 units; and the bound every convolution kernel is held to, 5e-6 of the output range."""
    rng = np.random.default_rng(11)
    B = _block_weights(rng)
    B = dict(B, pro=(np.abs(B["pro"][0]), np.abs(B["pro"][1])), w1=np.abs(B["w1"]), b1=np.abs(B["b1"]), w2=np.abs(B["w2"]), b2=np.abs(B["b2"]),
             w3=np.abs(B["w3"]), b3=np.abs(B["b3"]))
    x = torch.from_numpy(np.abs(rng.standard_normal((144, 8, 8, 256))).astype(np.float32)).cuda()
    got, flag = _run(ops, "f16x2", x, B)
    assert flag == 0
    got = got.cpu().numpy().astype(np.float64)
    f32 = ops.res_block(x, B["pro"], B["w1"], B["b1"], B["w2"], B["b2"], B["w3"], B["b3"]).cpu().numpy().astype(np.float64)
    ref = _fp64(x, B)
    U = 2.0 ** -24
    ex, ef = (got - ref) / (U * ref), (f32 - ref) / (U * ref)
    print("\nres_block f16x2 8x8 x 144 one-signed: max|err| %.3f (fp32 pipe %.3f), mean signed %+.4f, std %.3f   [units of 2^-24 sum|x||w|]"
          % (np.abs(ex).max(), np.abs(ef).max(), ex.mean(), ex.std()))
    assert np.abs(ex).max() <= 2.0 * np.sqrt(256 + 1152 + 128)
    assert np.abs(ex).max() <= 1.5 * np.abs(ef).max() + 1.5
    assert abs(ex.mean()) <= 1.5
    assert np.abs(got - ref).max() / np.abs(ref).max() < 5e-6
