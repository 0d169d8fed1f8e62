"""The fp16 kernels at site shifts other than 4 -- what a calibrated network runs (suo_net_calibrate) -- per kernel and per site.

The kernels read a site's factor 2^s through a pointer (GemmArgs.xscale, GemmChainArgs.xs1 / xs2, ConvArgs.xscale / xscale3 / n_xscale, ResBlockArgs.xs1 / xs2 / xs3,
StemNext.xscale); suo_debug_f16x2_stage_sites lets the per-stage entries hand such pointers over (tests/hipops.py: sites).

The oracle needs NO tolerance.  Multiplying by a power of two is exact, so every kernel is scale-covariant bit for bit: take a call at the default s = 4; move a site
to s = 4 - d, multiply that site's operand by 2^d, pass ldexp(oscale, d) (hipops.sites does, as Net::set_f16x2_shifts), and multiply biases, skip, up-sampled addend and
prologue shift by 2^(exponent of the tensor they are added to).  Every fp16 term, every MFMA input and every accumulator then has the baseline's bits, the output is
ldexp(baseline, d_out) exactly and the flag is the baseline's.  Sites inside one launch get DIFFERENT d by scaling the weights between them by a power of two (the
packers' row shift t_n moves by exactly that exponent: same planes) -- with equal shifts everywhere a swapped pointer could not be seen.  |d| <= 30 and |t_n| < 100
throughout: nothing is clamped, nothing becomes subnormal.  The baseline itself is held to fp64 by tests/test_gpu_f16x2.py; one case per family here is gated per
element against fp64 at the scaled data as well (|out - ref| <= 2 sqrt(K) 2^-24 sum |x||w|, the magnitudes propagated through the layers of a multi-layer launch).

Guards: one element of ldexp(65504, -s) at a 1x1 site (ldexp(65504, -(s + 2)) at a 3x3 site: |B^T d B| <= 4 max |d|) raises the flag, the float below it does not
(csrc/f16x2.h: S2_LIMIT; derived, not measured); the inner-site guards keep the baseline's flag in both directions when only the inner shift moves."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MIXED = (-2, 9, 1)                      # input, inner, third / next site: all different
ENDS = ((-26, 26, -26), (26, -26, 26))  # S2_SHIFT_MIN / S2_SHIFT_MAX
HALO = (("reg", {"SUO_WINO_HALO_DMA": "0", "SUO_WINO_W8": "0"}), ("dma", {"SUO_WINO_HALO_DMA": "1", "SUO_WINO_W8": "0"}), ("w8", {"SUO_WINO_HALO_DMA": "1", "SUO_WINO_W8": "1"}))
WINO_SHAPES = [(1, 8, 16), (2, 20, 24), (1, 4, 8)]      # one tile; ragged on both axes, several tiles and crops; a map smaller than the tile


@pytest.fixture(scope="module")
def ops():
    from suo_slam_amd import _lib
    _lib.require_gpu()
    from tests import hipops
    return hipops


def p2(x, d):
    """x 2^d, exact (numpy array or cuda tensor; None stays None)"""
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        return x * float(2.0 ** d)
    return np.ldexp(np.asarray(x, np.float32), d).astype(np.float32)


def same(a, b):
    """bit for bit (signed zeros and nans included)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def gate(out, ref, S, K, what):
    e = np.abs(out.detach().cpu().numpy().astype(np.float64) - ref) / (U * S)
    print("   %-40s max|err| %.3f of %.1f   [units of 2^-24 sum|x||w|]" % (what, e.max(), 2.0 * np.sqrt(K)))
    assert np.isfinite(e).all() and e.max() <= 2.0 * np.sqrt(K), (what, e.max())


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def halo_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---- suo_conv1x1_f16x2_ex / _pool ------------------------------------------------------------------------------------------------------------------------------------
def _gemm_case(rng, kind):
    """(args of ops.conv1x1_f16x2 as a dict, fp64 reference, sum of magnitudes, K) -- every operand path of the kernel at its smallest shape"""
    n = lambda *s: rng.standard_normal(s).astype(np.float32)
    if kind == "prologue":                                                  # two 128-row tiles plus a ragged 37; BN + ReLU prologue, ReLU
        M, K, N = 293, 128, 128
        c = dict(a1=n(M, K), w1=n(N, K) / 12, bias=n(N), pro=(rng.uniform(0.5, 1.5, K).astype(np.float32), n(K) * 0.3), relu=True)
    elif kind == "residual":                                                # the 64-row tiles, 256 columns, the residual operand
        M, K, N = 192, 256, 256
        c = dict(a1=n(M, K), w1=n(N, K) / 16, bias=n(N), res=n(M, N))
    elif kind == "n64":                                                     # 64 output columns
        M, K, N = 200, 256, 64
        c = dict(a1=n(M, K), w1=n(N, K) / 16, bias=n(N))
    else:                                                                   # second K segment with the fused 2x2 max-pool, (L, H, W) = (1, 4, 64)
        M, K, N = 256, 192, 128
        c = dict(a1=n(M, 128), w1=n(N, 128) / 12, bias=n(N), a2=n(M, 64), w2=n(N, 64) / 8, pool_hw=(4, 64))
    return c, K


def _gemm_run(ops, c, d):
    """the case moved by 2^d: operand(s), bias, residual, prologue shift; the site at 4 - d"""
    kw = dict(relu=c.get("relu", False), pool_hw=c.get("pool_hw"))
    if "pro" in c:
        kw["pro"] = (c["pro"][0], p2(c["pro"][1], d))
    if "a2" in c:
        kw.update(a2=cuda(p2(c["a2"], d)), w2=c["w2"])
    if "res" in c:
        kw["res"] = cuda(p2(c["res"], d))
    if d == 0:
        return ops.conv1x1_f16x2(cuda(c["a1"]), c["w1"], c["bias"], **kw)
    with ops.sites(in_=4 - d):
        return ops.conv1x1_f16x2(cuda(p2(c["a1"], d)), c["w1"], p2(c["bias"], d), **kw)


def _gemm_fp64(c, d):
    f = lambda k: np.ldexp(c[k].astype(np.float64), d)
    x = f("a1")
    if "pro" in c:
        x = np.maximum(x * c["pro"][0].astype(np.float64) + np.ldexp(c["pro"][1].astype(np.float64), d), 0)
    ref, S = x @ c["w1"].astype(np.float64).T + f("bias"), np.abs(x) @ np.abs(c["w1"]).astype(np.float64).T + np.abs(f("bias"))
    if "a2" in c:
        ref, S = ref + f("a2") @ c["w2"].astype(np.float64).T, S + np.abs(f("a2")) @ np.abs(c["w2"]).astype(np.float64).T
    if "res" in c:
        ref, S = ref + f("res"), S + np.abs(f("res"))
    return (np.maximum(ref, 0) if c.get("relu") else ref), S


@pytest.mark.parametrize("kind", ["prologue", "residual", "n64", "dual_pool"])
def test_gemm_at_a_site_shift(ops, kind):
    c, K = _gemm_case(np.random.default_rng(11), kind)
    base, f0 = _gemm_run(ops, c, 0)
    assert f0 == 0
    for s in (-2, 9, -26, 26):
        d = 4 - s
        got, flag = _gemm_run(ops, c, d)
        assert flag == 0, s
        if kind == "dual_pool":
            (full, pooled), (bfull, bpooled) = got, base
            assert same(pooled, p2(bpooled, d)), s
            o = full.reshape(1, 4, 64, 128).permute(0, 3, 1, 2)
            assert torch.equal(pooled.reshape(1, 2, 32, 128), F.max_pool2d(o, 2, 2).permute(0, 2, 3, 1)), s
            got, bfull_ = full, bfull
        else:
            bfull_ = base
        assert same(got, p2(bfull_, d)), (kind, s)
        if s == -2:
            ref, S = _gemm_fp64(c, d)
            gate(got, ref, S, K, "1x1 %s at s = %d" % (kind, s))


# ---- suo_conv1x1_chain_head_f16x2 ------------------------------------------------------------------------------------------------------------------------------------
def _chain_run(ops, c, s1, s2, a_moved=None):
    """lin's input at s1, tmpOut's input at s2: a 2^d1 (a_moved: given as it enters), W1 2^(d2 - d1), b1 2^d2 -> the inner tensor times 2^d2; W2 as it is, b2 2^d2 -> the
    logits times 2^d2"""
    d1, d2 = 4 - s1, 4 - s2
    a, w1, b1, b2 = cuda(p2(c["a"], d1) if a_moved is None else a_moved), p2(c["w1"], d2 - d1), p2(c["b1"], d2), p2(c["b2"], d2)
    with ops.sites(in_=s1, inner=s2):
        got = ops.conv1x1_chain_head_f16x2(a, w1, b1, c["w2"], b2, 41, c["hw"])
    with ops.sites(in_=s1):
        ll, f1 = ops.conv1x1_f16x2(a, w1, b1, relu=True)
    with ops.sites(in_=s2):
        two, f2 = ops.conv1x1_f16x2(ll, c["w2"], b2)
    return got, (ll, two, f1 | f2)


@pytest.mark.parametrize("M,hw", [(64, 64), (128, 64)])
def test_chain_head_at_two_site_shifts(ops, M, hw):
    rng = np.random.default_rng(M)
    w2 = np.zeros((64, 256), np.float32)
    w2[:41] = (rng.standard_normal((41, 256)) / 16).astype(np.float32)
    b2 = np.zeros(64, np.float32)
    b2[:41] = rng.standard_normal(41).astype(np.float32)
    c = dict(a=rng.standard_normal((M, 256)).astype(np.float32), w1=(rng.standard_normal((256, 256)) / 16).astype(np.float32),
             b1=(rng.standard_normal(256) * 0.2).astype(np.float32), w2=w2, b2=b2, hw=hw)
    base, f0 = ops.conv1x1_chain_head_f16x2(cuda(c["a"]), c["w1"], c["b1"], w2, b2, 41, hw)
    assert f0 == 0 and torch.isfinite(base).all()
    for s1, s2 in (MIXED[:2], MIXED[1::-1]) + tuple(e[:2] for e in ENDS):
        (got, flag), (ll, two, f12) = _chain_run(ops, c, s1, s2)
        assert flag == 0 and f12 == 0, (s1, s2)
        assert same(got, p2(base, 4 - s2)), (s1, s2)
        assert same(got, two.reshape(M // hw, hw, 64)[:, :, :41].permute(0, 2, 1).contiguous()), (s1, s2)     # the two launches at the same two shifts
        if (s1, s2) == MIXED[:2]:                                          # fp64: the head on the inner tensor the first launch stored (bit-identical to the one in LDS)
            x, b = ll.double().cpu().numpy(), np.ldexp(b2.astype(np.float64), 4 - s2)
            ref, S = x @ w2.astype(np.float64).T + b, np.abs(x) @ np.abs(w2).astype(np.float64).T + np.abs(b)
            S[:, 41:] = 1.0
            gate(two, ref, S, 256, "chain head at s = (%d, %d)" % (s1, s2))


# ---- suo_conv3x3_wino_f16x2_n ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [128, 64])
@pytest.mark.parametrize("L,H,W", WINO_SHAPES)
def test_winograd_at_a_site_shift(ops, monkeypatch, C, L, H, W):
    rng = np.random.default_rng(C + H)
    x = rng.standard_normal((L, H, W, C)).astype(np.float32)
    w = (rng.standard_normal((C, C, 3, 3)) / np.sqrt(9 * C)).astype(np.float32)
    b = (rng.standard_normal(C) * 0.3).astype(np.float32)
    xt, wt = torch.from_numpy(x).permute(0, 3, 1, 2).double(), torch.from_numpy(w).double()
    res = {}
    for s in (4, -2, 9, -26, 26):
        d = 4 - s
        for name, env in HALO:
            halo_env(monkeypatch, env)
            with ops.sites(in_=s):
                res[name, s] = ops.conv3x3_wino_f16x2(cuda(p2(x, d)), w, p2(b, d), relu=True)
            out, flag = res[name, s]
            assert flag == 0, (name, s)
            assert same(out, p2(res[name, 4][0], d)), (name, s)
        assert same(res["dma", s][0], res["reg", s][0]), s                 # the DMA halo equals the register halo at every shift
        if s == 9 and (L, H, W) == WINO_SHAPES[1]:
            ref = F.relu(F.conv2d(xt, wt, torch.from_numpy(b).double(), padding=1)).permute(0, 2, 3, 1).numpy() * 2.0 ** d
            S = (F.conv2d(xt.abs(), wt.abs(), torch.from_numpy(b).double().abs(), padding=1)).permute(0, 2, 3, 1).numpy() * 2.0 ** d
            for name, _ in HALO:
                gate(res[name, s][0], ref, S, 9 * C, "3x3 C = %d %s at s = %d" % (C, name, s))


# ---- the fused tail (conv2 3x3 -> ReLU -> conv3 1x1 + skip [+ up]) [+ the next block's conv1] -----------------------------------------------------------------------
def _tail_case(rng, L, H, W, up):
    n = lambda *s: rng.standard_normal(s).astype(np.float32)
    return dict(x=n(L, H, W, 128), skip=n(L, H, W, 256), up=n(L, H // 2, W // 2, 256) if up else None, w2=n(128, 128, 3, 3) / np.float32(np.sqrt(9 * 128)), b2=n(128) * 0.3,
                w3=n(256, 128) / np.float32(np.sqrt(128)), b3=n(256), ns=rng.uniform(0.5, 1.5, 256).astype(np.float32), nt=n(256) * 0.3, w1=n(128, 256) / 16, b1=n(128) * 0.2)


def _tail_args(c, s2, s3):
    """conv2's input at s2, conv3's at s3: x 2^d2, W2 2^(d3 - d2), b2 2^d3 -> relu(conv2) times 2^d3; W3 as it is; b3, skip, up 2^d3 -> out times 2^d3"""
    d2, d3 = 4 - s2, 4 - s3
    return (cuda(p2(c["x"], d2)), p2(c["w2"], d3 - d2), p2(c["b2"], d3), c["w3"], p2(c["b3"], d3), cuda(p2(c["skip"], d3)), cuda(p2(c["up"], d3)) if c["up"] is not None else None)


def _next_args(c, s3, sn):
    """the next conv1's input at sn, on an `out` that carries 2^d3: BN scale 2^(dn - d3), BN shift 2^dn -> the operand times 2^dn; W1 as it is, b1 2^dn"""
    d3, dn = 4 - s3, 4 - sn
    return (p2(c["ns"], dn - d3), p2(c["nt"], dn)), c["w1"], p2(c["b1"], dn)


def _tail_fp64(c):
    xm = torch.from_numpy(c["x"]).permute(0, 3, 1, 2).double()
    t = lambda k: torch.from_numpy(c[k]).double()
    m = F.relu(F.conv2d(xm, t("w2"), t("b2"), padding=1))
    ma = F.conv2d(xm.abs(), t("w2").abs(), t("b2").abs(), padding=1)       # magnitudes through the two layers
    ref = F.conv2d(m, t("w3")[:, :, None, None], t("b3")).permute(0, 2, 3, 1).numpy() + c["skip"]
    S = F.conv2d(ma, t("w3").abs()[:, :, None, None], t("b3").abs()).permute(0, 2, 3, 1).numpy() + np.abs(c["skip"])
    if c["up"] is not None:
        u = np.repeat(np.repeat(c["up"].astype(np.float64), 2, axis=1), 2, axis=2)
        ref, S = ref + u, S + np.abs(u)
    return ref, S


@pytest.mark.parametrize("up", [False, True])
@pytest.mark.parametrize("L,H,W", WINO_SHAPES)
def test_fused_tail_at_two_site_shifts(ops, monkeypatch, up, L, H, W):
    c = _tail_case(np.random.default_rng(40 + H + up), L, H, W, up)
    res = {}
    for s2, s3 in ((4, 4), MIXED[:2], MIXED[1::-1]) + tuple(e[:2] for e in ENDS):
        for name, env in HALO:
            halo_env(monkeypatch, env)
            with ops.sites(in_=s2, inner=s3):
                res[name, s2, s3] = ops.conv3x3_wino_f16x2_conv1x1_skip_up(*_tail_args(c, s2, s3))
            out, flag = res[name, s2, s3]
            assert flag == 0, (name, s2, s3)
            assert same(out, p2(res[name, 4, 4][0], 4 - s3)), (name, s2, s3)
        assert same(res["dma", s2, s3][0], res["reg", s2, s3][0]), (s2, s3)
        if (s2, s3) == MIXED[:2] and (L, H, W) == WINO_SHAPES[1]:
            ref, S = _tail_fp64(c)
            for name, _ in HALO:
                gate(res[name, s2, s3][0], ref * 2.0 ** (4 - s3), S * 2.0 ** (4 - s3), 9 * 128 + 128, "tail up = %s %s at s = (%d, %d)" % (up, name, s2, s3))


@pytest.mark.parametrize("dma", ["0", "1"])
def test_fused_tail_with_next_at_three_site_shifts(ops, monkeypatch, dma):
    """`out` = the tail without NEXT at the same shifts, `next` = suo_conv1x1_f16x2_ex on that `out` at the next site's shift, both bit for bit (the four-wave forms)."""
    monkeypatch.setenv("SUO_WINO_W8", "0")
    monkeypatch.setenv("SUO_WINO_HALO_DMA", dma)
    L, H, W = WINO_SHAPES[1]
    c = _tail_case(np.random.default_rng(50), L, H, W, False)
    b_out, b_nxt, f0 = ops.conv3x3_wino_f16x2_tail_next(*_tail_args(c, 4, 4), *_next_args(c, 4, 4))
    assert f0 == 0
    for s2, s3, sn in (MIXED, (MIXED[2], MIXED[0], MIXED[1])) + ENDS:
        with ops.sites(in_=s2, inner=s3, next=sn):
            out, nxt, flag = ops.conv3x3_wino_f16x2_tail_next(*_tail_args(c, s2, s3), *_next_args(c, s3, sn))
        with ops.sites(in_=s2, inner=s3):
            plain, f1 = ops.conv3x3_wino_f16x2_conv1x1_skip_up(*_tail_args(c, s2, s3))
        pro, w1, b1 = _next_args(c, s3, sn)
        with ops.sites(in_=sn):
            sep, f2 = ops.conv1x1_f16x2(plain.reshape(-1, 256), w1, b1, pro=pro, relu=True)
        assert flag == 0 and f1 == 0 and f2 == 0, (s2, s3, sn)
        assert same(out, plain) and same(out, p2(b_out, 4 - s3)), (s2, s3, sn)
        assert same(nxt.reshape(-1, 128), sep) and same(nxt, p2(b_nxt, 4 - sn)), (s2, s3, sn)
        if (s2, s3, sn) == MIXED:                                          # fp64: conv1 on the stored `out` (the tail itself is gated above)
            o = plain.reshape(-1, 256).double().cpu().numpy()
            x = np.maximum(o * pro[0].astype(np.float64) + pro[1].astype(np.float64), 0)
            ref = np.maximum(x @ w1.astype(np.float64).T + b1, 0)
            gate(sep, ref, np.abs(x) @ np.abs(w1).astype(np.float64).T + np.abs(b1), 256, "next conv1 at s = %d" % sn)


# ---- suo_res_block_f16x2 ---------------------------------------------------------------------------------------------------------------------------------------------
def _block_case(rng, L, H, pool, up, one_signed=False):
    f = (lambda a: np.abs(a).astype(np.float32)) if one_signed else (lambda a: a.astype(np.float32))
    n = lambda *s: rng.standard_normal(s)
    return dict(x=f(n(L, 2 * H, 2 * H, 256) if pool else n(L, H, H, 256)), up=f(n(L, H // 2, H // 2, 256)) if up else None, pool=pool,
                ps=rng.uniform(0.5, 1.5, 256).astype(np.float32), pt=f(n(256) * 0.3), w1=f(n(128, 256) / 16), b1=f(n(128) * 0.2), w2=f(n(128, 128, 3, 3) / np.sqrt(9 * 128)),
                b2=f(n(128) * 0.2), w3=f(n(256, 128) / np.sqrt(128)), b3=f(n(256) * 0.2))


def _block_run(ops, c, s1, s2, s3, x_moved=None):
    """conv1 / conv2 / conv3 inputs at s1 / s2 / s3.  out = conv3 + x [+ up] carries 2^d3 (W3 as it is), so x (x_moved: given as it enters) and up 2^d3; the prologue takes
    x 2^d3 to the operand 2^d1 (scale 2^(d1 - d3), shift 2^d1); W1 2^(d2 - d1), b1 2^d2; W2 2^(d3 - d2), b2 2^d3; b3 2^d3"""
    d1, d2, d3 = 4 - s1, 4 - s2, 4 - s3
    with ops.sites(in_=s1, inner=s2, third=s3):
        return ops.res_block_f16x2(cuda(p2(c["x"], d3) if x_moved is None else x_moved), (p2(c["ps"], d1 - d3), p2(c["pt"], d1)), p2(c["w1"], d2 - d1), p2(c["b1"], d2), p2(c["w2"], d3 - d2), p2(c["b2"], d3),
                                   c["w3"], p2(c["b3"], d3), up_nhwc=cuda(p2(c["up"], d3)) if c["up"] is not None else None, pool_in=c["pool"])


def _block_fp64(c):
    t = lambda k: torch.from_numpy(c[k]).double()
    x = t("x").permute(0, 3, 1, 2)
    if c["pool"]:
        x = F.max_pool2d(x, 2, 2)
    v = lambda k: t(k)[None, :, None, None]
    a = F.relu(x * v("ps") + v("pt"))
    m1 = F.relu(F.conv2d(a, t("w1")[:, :, None, None], t("b1")))
    m1a = F.conv2d(a, t("w1").abs()[:, :, None, None], t("b1").abs())
    m2 = F.relu(F.conv2d(m1, t("w2"), t("b2"), padding=1))
    m2a = F.conv2d(m1a, t("w2").abs(), t("b2").abs(), padding=1)
    ref = F.conv2d(m2, t("w3")[:, :, None, None], t("b3")) + x
    S = F.conv2d(m2a, t("w3").abs()[:, :, None, None], t("b3").abs()) + x.abs()
    if c["up"] is not None:
        u = t("up").permute(0, 3, 1, 2).repeat_interleave(2, 2).repeat_interleave(2, 3)
        ref, S = ref + u, S + u.abs()
    return ref.permute(0, 2, 3, 1).numpy(), S.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("pool,up", [(True, False), (False, True), (False, False)])
@pytest.mark.parametrize("L,H", [(2, 8), (3, 4)])
def test_res_block_at_three_site_shifts(ops, L, H, pool, up):
    c = _block_case(np.random.default_rng(60 + H + pool + 2 * up), L, H, pool, up)
    base, f0 = _block_run(ops, c, 4, 4, 4)
    assert f0 == 0 and torch.isfinite(base).all()
    for s in (MIXED, (MIXED[2], MIXED[0], MIXED[1])) + ENDS:
        out, flag = _block_run(ops, c, *s)
        assert flag == 0, s
        assert same(out, p2(base, 4 - s[2])), s
        if s == MIXED:
            ref, S = _block_fp64(c)
            gate(out, ref * 2.0 ** (4 - s[2]), S * 2.0 ** (4 - s[2]), 256 + 9 * 128 + 128, "block pool = %s up = %s at s = %s" % (pool, up, s))


# ---- suo_stem_f16x2_next ---------------------------------------------------------------------------------------------------------------------------------------------
def test_stem_next_at_a_site_shift(ops):
    """Two boxes on one 480 x 640 frame.  The stem's own site stays at 2^4 by design: its output is unchanged bit for bit; only the next site moves."""
    rng = np.random.default_rng(71)
    img = torch.from_numpy(rng.integers(0, 256, (1, 480, 640, 3), dtype=np.uint8)).cuda()
    boxes, idx = np.array([[100.3, 50.7, 300.9, 260.2], [10, 20, 522, 472]], np.float32), np.zeros(2, np.int32)
    w = (rng.standard_normal((64, 44, 7, 7)) / np.sqrt(49 * 3)).astype(np.float32)
    scale, bias = rng.uniform(0.5, 1.5, 64).astype(np.float32), (rng.standard_normal(64) * 0.3).astype(np.float32)
    ps, pt = rng.uniform(0.5, 1.5, 64).astype(np.float32), (rng.standard_normal(64) * 0.2).astype(np.float32)
    w1, b1 = (rng.standard_normal((64, 64)) / 8).astype(np.float32), (rng.standard_normal(64) * 0.2).astype(np.float32)
    plain, _, f0 = ops.stem_f16x2(img, 0, boxes, idx, w, scale, bias)
    b_out, b_mid, f1 = ops.stem_f16x2(img, 0, boxes, idx, w, scale, bias, nxt=(ps, pt, w1, b1))
    assert f0 == 0 and f1 == 0 and same(b_out, plain)
    for s in (-2, 9, -26, 26):
        d = 4 - s
        nxt = (p2(ps, d), p2(pt, d), w1, p2(b1, d))
        with ops.sites(next=s):
            out, mid, flag = ops.stem_f16x2(img, 0, boxes, idx, w, scale, bias, nxt=nxt)
        with ops.sites(in_=s):
            sep, f2 = ops.conv1x1_f16x2(plain.reshape(-1, 64), w1, nxt[3], pro=nxt[:2], relu=True)
        assert flag == 0 and f2 == 0, s
        assert same(out, plain), s
        assert same(mid.reshape(-1, 64), sep) and same(mid, p2(b_mid, d)), s
        if s == -2:
            x = np.maximum(plain.reshape(-1, 64).double().cpu().numpy() * nxt[0].astype(np.float64) + nxt[1].astype(np.float64), 0)
            gate(sep, np.maximum(x @ w1.astype(np.float64).T + nxt[3], 0), np.abs(x) @ np.abs(w1).astype(np.float64).T + np.abs(nxt[3]), 64, "stem's next conv1 at s = %d" % s)
    # the guard on conv1's operand relu(bn(out)), which the caller never sees: a BatchNorm scale of 3e4 takes it far beyond 4094 (out >= 0, scale >= 0.5, |shift| < 2)
    assert 0.5 * 3e4 * plain.max().item() - 2.0 >= 2 * 4094.0
    for gain, want in ((1.0, 0), (3e4, 1)):
        for s in (4, -5, 9):
            d = 4 - s
            with ops.sites(next=s):
                assert ops.stem_f16x2(img, 0, boxes, idx, w, scale, bias, nxt=(p2(ps * np.float32(gain), d), p2(pt, d), w1, p2(b1, d)))[2] == want, (gain, s)


# ---- the guards at a shift ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [-5, 0, 9])
@pytest.mark.parametrize("pro", [False, True])
def test_gemm_guard_at_a_site_shift(ops, s, pro):
    """2^s |x| = 65504 raises the flag, the float below does not (with a prologue: the value after relu(x * 2 + 2^(4 - s)) counts); the last element of the ragged last tile."""
    rng = np.random.default_rng(3)
    M, K, N = 293, 128, 128
    d = 4 - s
    w = (rng.standard_normal((N, K)) / 12).astype(np.float32)
    limit = np.ldexp(np.float32(65504.0), -s)
    below = np.nextafter(limit, np.float32(0))
    assert below < limit and np.ldexp(below, s) < 65504.0
    sc, sh = np.full(K, 2.0, np.float32), np.full(K, np.ldexp(np.float32(1.0), d), np.float32)
    for big, want in ((below, 0), (limit, 1)):
        a = np.ldexp(np.abs(rng.standard_normal((M, K))).astype(np.float32), d)
        a[M - 1, K - 1] = (big - sh[0]) / np.float32(2.0) if pro else big  # (exact: big and the shift are multiples of 2 ulp of big / 2)
        if pro:
            assert np.float32(a[M - 1, K - 1] * np.float32(2.0) + sh[0]) == big
        with ops.sites(in_=s):
            out, flag = ops.conv1x1_f16x2(cuda(a), w, np.zeros(N, np.float32), pro=(sc, sh) if pro else None)
        assert flag == want, (s, big, flag)
        if not want:
            assert torch.isfinite(out).all()


@pytest.mark.parametrize("s", [-5, 0, 9])
@pytest.mark.parametrize("C", [128, 64])
def test_winograd_guard_at_a_site_shift(ops, monkeypatch, C, s):
    """3x3 input: the guard bounds |B^T d B| by 4 max |d|, so the limit is ldexp(65504, -(s + 2)).  The element sits at the last pixel and channel of the last crop, and
    once where every tile but its own sees it only in its halo (the first row and column of the tile at (8, 16)); the register halo, the DMA halo and the eight-wave form."""
    rng = np.random.default_rng(21 + C)
    L, H, W = WINO_SHAPES[1]
    d = 4 - s
    w = (rng.standard_normal((C, C, 3, 3)) / np.sqrt(9 * C)).astype(np.float32)
    b = np.zeros(C, np.float32)
    limit = np.ldexp(np.float32(65504.0), -(s + 2))
    below = np.nextafter(limit, np.float32(0))
    x0 = np.ldexp(rng.standard_normal((L, H, W, C)).astype(np.float32), d)
    for pos in ((L - 1, H - 1, W - 1, C - 1), (0, 8, 16, C - 1)):
        for big, want in ((below, 0), (-limit, 1)):
            x = x0.copy()
            x[pos] = big
            flags = {}
            for name, env in HALO:
                halo_env(monkeypatch, env)
                with ops.sites(in_=s):
                    out, flags[name] = ops.conv3x3_wino_f16x2(cuda(x), w, b)
                assert flags[name] == want, (name, s, pos, big)
                if not want:
                    assert torch.isfinite(out).all()


@pytest.mark.parametrize("s", [-5, 0, 9])
def test_block_and_chain_head_input_guard_at_a_site_shift(ops, s):
    """The other two 1x1 input sites: conv1 of the one-launch block (prologue scale 1, shift 0) and lin of the chain head, the element in the last pixel and channel.
    Only the input carries the large value: the inner operands stay below a quarter of the limit (|w| <= 0.3, so one product of 4094 adds at most ~1000)."""
    rng = np.random.default_rng(33)
    d = 4 - s
    limit = np.ldexp(np.float32(65504.0), -s)
    blk = dict(_block_case(rng, 2, 8, False, False), ps=np.ones(256, np.float32), pt=np.zeros(256, np.float32))
    w2 = np.zeros((64, 256), np.float32)
    w2[:41] = (rng.standard_normal((41, 256)) / 16).astype(np.float32)
    ch = dict(a=rng.standard_normal((128, 256)).astype(np.float32), w1=(rng.standard_normal((256, 256)) / 16).astype(np.float32), b1=np.zeros(256, np.float32), w2=w2,
              b2=np.zeros(64, np.float32), hw=64)
    for big, want in ((np.nextafter(limit, np.float32(0)), 0), (limit, 1)):
        x = p2(blk["x"], d)
        x[1, 7, 7, 255] = big
        out, flag = _block_run(ops, blk, s, 4, s, x_moved=x)
        assert flag == want and (want or torch.isfinite(out).all()), ("block", s, big, flag)
        a = p2(ch["a"], d)
        a[127, 255] = big
        (out, flag), _ = _chain_run(ops, ch, s, 4, a_moved=a)
        assert flag == want and (want or torch.isfinite(out).all()), ("chain head", s, big, flag)


def test_inner_site_guards_keep_the_baselines_flag(ops, monkeypatch):
    """The s = 4 constructions of tests/test_gpu_f16x2.py and tests/test_gpu_res_block.py whose INNER activation (a tensor the caller never sees) does / does not reach the
    limit, moved by the scale identity so that only that inner site's shift differs from 4: the flag is the baseline's, raised and not raised."""
    rng = np.random.default_rng(21)
    # the tail's conv3 input relu(conv2 + b2) (gains as in test_winograd_and_tail_range_guard), under both halo paths and the eight-wave form
    c = _tail_case(rng, 1, 8, 16, False)
    c.update(x=np.abs(c["x"]), b2=np.zeros(128, np.float32), b3=np.zeros(256, np.float32))
    w2 = np.abs(c["w2"])
    for gain, want in ((100.0, 0), (250.0, 1)):
        c["w2"] = w2 * np.float32(gain)
        m = F.relu(F.conv2d(torch.from_numpy(c["x"]).permute(0, 3, 1, 2).double(), torch.from_numpy(c["w2"]).double(), padding=1)).max().item()
        assert (m >= 65504.0 / 16.0) == bool(want), m
        for name, env in HALO:
            halo_env(monkeypatch, env)
            for s3 in (4, -5, 9):
                with ops.sites(inner=s3):
                    assert ops.conv3x3_wino_f16x2_conv1x1_skip_up(*_tail_args(c, 4, s3))[1] == want, (name, gain, s3)
    # the NEXT conv1's input relu(bn_next(out)): a BatchNorm scale of 3000 (test_fused_tail_with_the_next_blocks_conv1_equals_the_separate_launches)
    monkeypatch.setenv("SUO_WINO_W8", "0")
    c = _tail_case(rng, 1, 8, 16, False)
    ns = c["ns"]
    for gain, want in ((1.0, 0), (3000.0, 1)):
        c["ns"] = ns * np.float32(gain)
        for dma in ("0", "1"):
            monkeypatch.setenv("SUO_WINO_HALO_DMA", dma)
            for sn in (4, -5, 9):
                with ops.sites(next=sn):
                    assert ops.conv3x3_wino_f16x2_tail_next(*_tail_args(c, 4, 4), *_next_args(c, 4, sn))[2] == want, (dma, gain, sn)
    # the chain head's tmpOut input relu(lin) (test_chain_head_range_guard: W1 x 400)
    w2h = np.zeros((64, 256), np.float32)
    w2h[:41] = (rng.standard_normal((41, 256)) / 16).astype(np.float32)
    ch = dict(a=np.abs(rng.standard_normal((64, 256))).astype(np.float32), b1=np.zeros(256, np.float32), w2=w2h, b2=np.zeros(64, np.float32), hw=64)
    w1 = np.abs(rng.standard_normal((256, 256)) / 16).astype(np.float32)
    for gain, want in ((1.0, 0), (400.0, 1)):
        ch["w1"] = w1 * np.float32(gain)
        for s2 in (4, -5, 9):
            assert _chain_run(ops, ch, 4, s2)[0][1] == want, (gain, s2)
    # the one-launch block's conv2 and conv3 inputs relu(conv1), relu(conv2) (test_res_block_f16x2_forward_error_per_element_and_range_guard: W1 x 2000, W2 x 3000)
    blk = _block_case(rng, 2, 8, False, False, one_signed=True)
    for key, gain, want in (("w1", 1.0, 0), ("w1", 2000.0, 1), ("w2", 3000.0, 1)):
        bi = dict(blk)
        bi[key] = blk[key] * np.float32(gain)
        for s in ((4, 4, 4), (4, -5, 4), (4, 9, 4), (4, 4, -5), (4, 4, 9)):
            assert _block_run(ops, bi, *s)[1] == want, (key, gain, s)


# ---- a null hook is the behaviour without it -----------------------------------------------------------------------------------------------------------------------
def test_cleared_hook_restores_every_entry_bit_for_bit(ops, monkeypatch):
    """One call per entry before the hook was ever set in this test, the same call after hipops.sites has exited -- once normally, once through an exception."""
    monkeypatch.setenv("SUO_WINO_W8", "0")
    rng = np.random.default_rng(90)
    g, _ = _gemm_case(rng, "prologue")
    gp, _ = _gemm_case(rng, "dual_pool")
    t = _tail_case(rng, 1, 8, 16, True)
    tn = dict(t, up=None)
    blk = _block_case(rng, 2, 8, False, True)
    w2h = np.zeros((64, 256), np.float32)
    w2h[:41] = (rng.standard_normal((41, 256)) / 16).astype(np.float32)
    a = cuda(rng.standard_normal((64, 256)))
    img = torch.from_numpy(rng.integers(0, 256, (1, 480, 640, 3), dtype=np.uint8)).cuda()
    box, idx = np.array([[100.3, 50.7, 300.9, 260.2]], np.float32), np.zeros(1, np.int32)
    ws = (rng.standard_normal((64, 44, 7, 7)) / np.sqrt(49 * 3)).astype(np.float32)
    one64 = np.ones(64, np.float32)
    w64 = (rng.standard_normal((64, 64)) / 8).astype(np.float32)

    def calls():
        r = [_gemm_run(ops, g, 0)[0], *_gemm_run(ops, gp, 0)[0], ops.conv1x1_chain_head_f16x2(a, g["w1"].repeat(2, 0).repeat(2, 1), np.zeros(256, np.float32), w2h, np.zeros(64, np.float32), 41, 64)[0],
             ops.conv3x3_wino_f16x2(cuda(t["x"]), t["w2"], t["b2"])[0], ops.conv3x3_wino_f16x2(cuda(t["x"][..., :64]), t["w2"][:64, :64], t["b2"][:64])[0],
             ops.conv3x3_wino_f16x2_conv1x1_skip_up(*_tail_args(t, 4, 4))[0], *ops.conv3x3_wino_f16x2_tail_next(*_tail_args(tn, 4, 4), *_next_args(tn, 4, 4))[:2],
             ops.res_block_f16x2(cuda(blk["x"]), (blk["ps"], blk["pt"]), blk["w1"], blk["b1"], blk["w2"], blk["b2"], blk["w3"], blk["b3"], up_nhwc=cuda(blk["up"]))[0],
             *ops.stem_f16x2(img, 0, box, idx, ws, one64, one64, nxt=(one64, one64, w64, one64))[:2]]
        return r
    before = calls()
    with ops.sites(in_=2, inner=6, third=3, next=5):
        calls()                                                            # every entry has run with the hook set (that it is live there: the tests above)
    assert all(same(x, y) for x, y in zip(before, calls()))
    with pytest.raises(RuntimeError, match="inside"):
        with ops.sites(in_=2, inner=6, third=3, next=5):
            raise RuntimeError("inside")
    assert all(v is None for v in ops._SITES.values())
    assert all(same(x, y) for x, y in zip(before, calls()))
