"""The fp16 1x1 GEMMs run their four waves side by side on 128 x 128 tiles (csrc/gemm_bf16x3.hip: W14; SUO_GEMM_WAVES_1X4=0 keeps 2 x 2), and so does the first
stage of the lin -> head chain.  Both layouts give every output element the same sum of the same products in ascending k and track the same activations, so every
stored byte and the range flag must agree BIT FOR BIT, through the C ABI's direct GEMM entries, in one library, by the switch.

Un-pooled launches of at most 1023 tiles of 128 rows take 64-row tiles (csrc/gemm_bf16x3.hip: rows64), which have the 2 x 2 layout only: there the switch must be
inert.  So every un-pooled case runs twice -- at its own M (`tail`), and with its rows behind 1024 full tiles (M = 131072 + tail), the smallest launch that takes
the 128-row kernels: the last tile is then the case's own tile and the first 1024 are plain interior ones.  Pooled launches take 128-row tiles at every size."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FULL = 1024 * 128                                           # rows of 1024 full tiles
SENTINEL = -7.25                                            # what rows past M and columns past N of an output must still hold


@pytest.fixture(scope="module")
def ops():
    from suo_slam_amd import _lib
    _lib.require_gpu()
    from tests import hipops
    return hipops


def _bits(t):
    return t.view(torch.int32)


def _gemm(ops, a1, w, bias, pro=None, a2=None, res=None, relu=False, pool_hw=None, want_full=True, pad_rows=128, ldo_extra=0):
    """One launch of suo_conv1x1_f16x2_ex / _pool.  `res` may be a column slice of a wider tensor (ldr != N); the outputs are allocated with `pad_rows` rows past M
    and `ldo_extra` columns past N, all pre-filled with SENTINEL.  -> (out or None, pooled or None, flag)"""
    from suo_slam_amd import _lib
    P, S = ops.P, ops.S
    lib = _lib.lib()
    M, K1 = a1.shape
    N = w.shape[0]
    K2 = a2.shape[1] if a2 is not None else 0
    w16, _, osc = ops.pack_gemm_f16x2(w)
    osc = ops._osc(osc, "in")
    b = ops.dev(bias)
    ps, pt = (ops.dev(pro[0]), ops.dev(pro[1])) if pro is not None else (None, None)
    ldo = N + ldo_extra
    out = torch.full((M + pad_rows, ldo), SENTINEL, device="cuda") if want_full else None
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    lda2 = a2.stride(0) if a2 is not None else 0
    ldr = res.stride(0) if res is not None else 0
    if pool_hw is None:
        _lib.check(lib.suo_conv1x1_f16x2_ex(P(a1), a1.stride(0), K1, P(ps), P(pt), P(a2), lda2, K2, P(w16), P(osc), P(b), P(res), ldr, P(out), ldo, M, N, int(relu),
                                            P(flag), S()), "suo_conv1x1_f16x2_ex")
        pooled = None
    else:
        pooled = torch.full((M // 4 + pad_rows, ldo), SENTINEL, device="cuda")
        _lib.check(lib.suo_conv1x1_f16x2_pool(P(a1), a1.stride(0), K1, P(ps), P(pt), P(a2), lda2, K2, P(w16), P(osc), P(b), P(res), ldr, P(out), ldo, M, N, int(relu),
                                              pool_hw[0], pool_hw[1], P(pooled), P(flag), S()), "suo_conv1x1_f16x2_pool")
    torch.cuda.synchronize()
    return out, pooled, int(flag.item())


def _layouts(monkeypatch, run):
    """run() under 2 x 2 and under 1 x 4"""
    monkeypatch.setenv("SUO_GEMM_WAVES_1X4", "0")
    two = run()
    monkeypatch.setenv("SUO_GEMM_WAVES_1X4", "1")
    four = run()
    return two, four


def _assert_same(two, four, M, N, pooled_rows=None):
    (o2, p2, f2), (o4, p4, f4) = two, four
    assert f2 == f4
    if o2 is not None:
        assert torch.equal(_bits(o2), _bits(o4))
        assert (o4[M:] == SENTINEL).all() and (o4[:, N:] == SENTINEL).all()      # rows past M, columns past N: nothing stored
        assert (o4[:M, :N] != SENTINEL).all()
    if p2 is not None:
        assert torch.equal(_bits(p2), _bits(p4))
        assert (p4[pooled_rows:] == SENTINEL).all() and (p4[:, N:] == SENTINEL).all()
        assert (p4[:pooled_rows, :N] != SENTINEL).all()
    return f4


def _data(seed, M, K, N, K2=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    a1 = torch.randn((M, K), device="cuda", generator=g)
    a2 = torch.randn((M, K2), device="cuda", generator=g) if K2 else None
    w = (rng.standard_normal((N, K + K2)) / np.sqrt(K + K2)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    return a1, a2, w, bias, rng, g


# (name, tail rows, K1, K2, N, prologue, residual, relu): the smallest shapes at which the layout can go wrong
CASES = [("one_tile_one_ring_round", 128, 64, 0, 128, False, False, False),
         ("two_segments", 128, 128, 128, 128, False, False, False),
         ("prologue", 128, 256, 0, 128, True, False, True),
         ("column_tile_1", 128, 64, 0, 256, False, False, False),
         ("ragged_rows", 200, 64, 0, 128, False, False, True),
         ("residual_ldr", 128, 128, 0, 128, False, True, True)]


@pytest.mark.parametrize("behind", [0, FULL], ids=["own_rows", "behind_1024_tiles"])
@pytest.mark.parametrize("name,tail,K1,K2,N,pro,res,relu", CASES, ids=[c[0] for c in CASES])
def test_layouts_agree_bit_for_bit(ops, monkeypatch, behind, name, tail, K1, K2, N, pro, res, relu):
    M = behind + tail
    a1, a2, w, bias, rng, g = _data(len(name) + M, M, K1, N, K2)
    pr = (rng.uniform(0.5, 1.5, K1).astype(np.float32), (rng.standard_normal(K1) * 0.3).astype(np.float32)) if pro else None
    r = torch.randn((M, N + 64), device="cuda", generator=g)[:, 32:32 + N] if res else None      # ldr = N + 64, starting 32 columns in
    run = lambda: _gemm(ops, a1, w, bias, pro=pr, a2=a2, res=r, relu=relu, ldo_extra=32)      # noqa: E731
    two, four = _layouts(monkeypatch, run)
    assert _assert_same(two, four, M, N) == 0
    assert torch.isfinite(four[0][:M, :N]).all()
    # the last tile holds the case's own rows: against the same rows launched alone (2 x 2, 64-row tiles) -- the same sums, whichever tile and layout
    if behind:
        alone = _gemm(ops, a1[behind:].contiguous(), w, bias, pro=pr, a2=a2[behind:].contiguous() if a2 is not None else None,
                      res=r[behind:] if res else None, relu=relu, ldo_extra=32)
        assert torch.equal(_bits(alone[0][:tail, :N]), _bits(four[0][behind:M, :N]))


@pytest.mark.parametrize("want_full", [True, False], ids=["pooled_and_full", "pooled_only"])
@pytest.mark.parametrize("K1,K2,res", [(256, 0, True), (128, 128, False)], ids=["residual", "two_segments"])
def test_pooled_launch_layouts_agree(ops, monkeypatch, want_full, K1, K2, res):
    """One crop of 2 x 64 pixels = one tile, N = 256 (both column tiles); and three crops of 4 x 128 (twelve row tiles: two per image row pair, two pairs per crop)."""
    for L, H, W in ((1, 2, 64), (3, 4, 128)):
        M, N = L * H * W, 256
        a1, a2, w, bias, rng, g = _data(17 * M + K2, M, K1, N, K2)
        r = torch.randn((M, N + 64), device="cuda", generator=g)[:, 32:32 + N] if res else None
        run = lambda: _gemm(ops, a1, w, bias, a2=a2, res=r, relu=True, pool_hw=(H, W), want_full=want_full, pad_rows=64)      # noqa: E731
        two, four = _layouts(monkeypatch, run)
        assert _assert_same(two, four, M, N, pooled_rows=M // 4) == 0
        if want_full:                                                         # the pooled rows are the 2 x 2 maxima of the full ones
            full = four[0][:M].view(L, H // 2, 2, W // 2, 2, N).amax(dim=(2, 4)).reshape(M // 4, N)
            assert torch.equal(_bits(full), _bits(four[1][:M // 4]))


@pytest.mark.parametrize("behind", [0, FULL], ids=["own_rows", "behind_1024_tiles"])
def test_range_flag_is_the_same_in_both_layouts(ops, monkeypatch, behind):
    """One activation at fp16's limit (65504 / 16 = 4094 at the default shift) raises the flag in both layouts, just below it in neither -- placed in the last k-step
    of the last tile's last row, and in a row of the upper half of an interior tile."""
    M, K, N = behind + 128, 128, 128
    a1, _, w, bias, _, _ = _data(5 + M, M, K, N)
    for row in (M - 1, 37):
        for big, want in ((4093.0, 0), (4094.0, 1)):
            a = a1.clone()
            a[row, K - 3] = big
            two, four = _layouts(monkeypatch, lambda: _gemm(ops, a, w, bias))
            assert _assert_same(two, four, M, N) == want, (row, big)


@pytest.mark.parametrize("behind", [0, FULL], ids=["own_rows", "behind_1024_tiles"])
def test_site_shift_other_than_4(ops, monkeypatch, behind):
    """At shift 1 the activations enter times 2: 4094 is far inside the range, 65504 / 2 = 32752 is the limit."""
    M, K, N = behind + 128, 64, 128
    a1, _, w, bias, _, _ = _data(9 + M, M, K, N)
    with ops.sites(in_=1):
        for big, want in ((4094.0, 0), (32751.0, 0), (32752.0, 1)):
            a = a1.clone()
            a[M - 5, 7] = big
            two, four = _layouts(monkeypatch, lambda: _gemm(ops, a, w, bias))
            assert _assert_same(two, four, M, N) == want, big
    at4 = _gemm(ops, a1, w, bias)
    with ops.sites(in_=1):
        at1 = _gemm(ops, a1, w, bias)
    assert at4[2] == at1[2] == 0 and not torch.equal(_bits(at4[0]), _bits(at1[0]))      # (the shift reached the kernel: other roundings)


@pytest.mark.parametrize("M", [64, 192])
def test_chain_head_layouts_agree(ops, monkeypatch, M):
    """lin -> head in one launch (gemm_chain_head_kernel): one and three 64-row tiles, NCHW store of the first 41 of 64 channels."""
    rng = np.random.default_rng(M)
    hw, n_valid = 64, 41
    a = torch.randn((M, 256), device="cuda", generator=torch.Generator(device="cuda").manual_seed(M))
    w1 = (rng.standard_normal((256, 256)) / 16).astype(np.float32)
    b1 = (rng.standard_normal(256) * 0.3).astype(np.float32)
    w2 = (rng.standard_normal((64, 256)) / 16).astype(np.float32)
    w2[n_valid:] = 0
    b2 = rng.standard_normal(64).astype(np.float32)
    b2[n_valid:] = 0
    two, four = _layouts(monkeypatch, lambda: ops.conv1x1_chain_head_f16x2(a, w1, b1, w2, b2, n_valid, hw))
    assert two[1] == four[1] == 0
    assert torch.isfinite(four[0]).all() and torch.equal(_bits(two[0]), _bits(four[0]))      # (the helper pre-fills with nan: every element was stored)
    big = a.clone()
    big[M - 1, 255] = 4094.0
    two, four = _layouts(monkeypatch, lambda: ops.conv1x1_chain_head_f16x2(big, w1, b1, w2, b2, n_valid, hw))
    assert two[1] == four[1] == 1
