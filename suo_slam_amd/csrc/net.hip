// Host-side runtime of the keypoint CNN: workspace, launch schedule, multi-stream hourglass branches, hipGraph capture of the backbone and the fp16 form's
// range guard.  Mirrors PkpNet.forward (lib/models/pkpnet.py:80-119) over the weights csrc/net_weights.hip builds.
#include "net.h"
#include "f16x2.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include "tune.h"

namespace suo {

// ------------------------------------------------------------------------------------------------
Net::Net(int n, const char* const* names, const float* const* data, const int64_t* const* shapes, const int* ndims, int max_crops)
    : max_crops_(max_crops) {
    build_weights(n, names, data, shapes, ndims);
    // the range guard's words: host memory mapped into the device's address space -- the kernels store to the live flag (rarely: only beyond fp16's range), each
    // forward's commit launch moves it into the call's slot, the host reads plain words after whatever synchronisation its results needed anyway
    const size_t guard_bytes = (size_t)(kSlotWord + kCallRing) * sizeof(unsigned);
    if (hipHostMalloc(reinterpret_cast<void**>(&range_flag_), guard_bytes, hipHostMallocMapped) != hipSuccess) throw std::runtime_error("hipHostMalloc(range flag) failed");
    memset(range_flag_, 0, guard_bytes);

    // ---- workspace: every intermediate gets its own slab (288 GB of HBM: no aliasing games).
    // Size it with a dry run of the launch schedule at max_crops.
    dry_run_ = true;
    ws_floats_ = (size_t)-1 / sizeof(float) / 2;
    (void)layout_slabs();
    // (every pipe this network can run on: the forms pick different kernels -- per-layer launches with their intermediate tensors where another form
    //  takes a one-launch block -- and a network that falls back to bf16x3 must find its workspace large enough)
    size_t need = 0;
    for (int p = pipe_built_; p >= (pipe_built_ == 0 ? 0 : 1); --p) {
        pipe_ = p;
        if (backbone(nullptr, IN_C, nullptr, max_crops_, nullptr) != SUO_OK) throw std::runtime_error("dry run failed");
        need = std::max(need, ws_used_);
    }
    pipe_ = pipe_built_;
    ws_floats_ = need;
    dry_run_ = false;
    if (hipMalloc(&ws_, ws_floats_ * sizeof(float)) != hipSuccess) throw std::runtime_error("hipMalloc(workspace) failed");
    if (hipMalloc(&d_mean_logit_, (size_t)max_crops_ * NUM_KP * sizeof(float)) != hipSuccess)
        throw std::runtime_error("hipMalloc failed");
    if (hipStreamCreateWithFlags(&own_stream_, hipStreamNonBlocking) != hipSuccess) throw std::runtime_error("hipStreamCreate failed");
    for (int i = 0; i < kNumSide; ++i) {
        if (hipStreamCreateWithFlags(&side_[i], hipStreamNonBlocking) != hipSuccess) throw std::runtime_error("hipStreamCreate failed");
    }
    for (int i = 0; i < kNumEvents; ++i)
        if (hipEventCreateWithFlags(&ev_[i], hipEventDisableTiming) != hipSuccess) throw std::runtime_error("hipEventCreate failed");
}

Net::~Net() {
    for (auto& kv : graphs_) { for (int i = 0; i < 2; ++i) if (kv.second.exec[i]) (void)hipGraphExecDestroy(kv.second.exec[i]); (void)hipGraphDestroy(kv.second.graph); }
    for (float* p : owned_) (void)hipFree(p);
    if (ws_) (void)hipFree(ws_);
    if (d_mean_logit_) (void)hipFree(d_mean_logit_);
    if (range_flag_) (void)hipHostFree(range_flag_);
    for (int i = 0; i < kNumSide; ++i) if (side_[i]) (void)hipStreamDestroy(side_[i]);
    if (own_stream_) (void)hipStreamDestroy(own_stream_);
    for (int i = 0; i < kNumEvents; ++i) if (ev_[i]) (void)hipEventDestroy(ev_[i]);
}

// The persistent slabs at the bottom of the workspace, the same for every call (captured graphs hold their addresses); the schedule's intermediates follow ws_mark_.
// (calibrate lays out its own: sized by its crop count, without r1's conv1 slab)
std::pair<float*, float*> Net::layout_slabs() {
    ws_used_ = 0;
    float* in0 = alloc((size_t)max_crops_ * CROP * CROP * IN_C);      // the staged input
    float* logits = alloc((size_t)max_crops_ * NUM_KP * HEAT * HEAT);
    stem_slab_ = alloc((size_t)max_crops_ * 128 * 128 * 64);          // the stem's output: persistent, the fused stem writes it OUTSIDE the captured graph
    stem_mid1_slab_ = alloc((size_t)max_crops_ * 128 * 128 * 64);     // ... and r1's conv1 of it, when the stem launch computes that too
    ws_mark_ = ws_used_;
    return {in0, logits};
}

float* Net::alloc(size_t floats) {
    floats = (floats + 63) & ~(size_t)63;
    if (ws_used_ + floats > ws_floats_) throw std::runtime_error("workspace exhausted");
    float* p = ws_ + ws_used_;
    ws_used_ += floats;
    return p;
}

#define SUO_TRY(x) do { int _r = (x); if (_r != SUO_OK) return _r; } while (0)
#define SUO_LAUNCH(x) do { if (acct_on_) ++acct_launches_; if (!dry_run_) { int _r = (x); if (_r != SUO_OK) return _r; } } while (0)
#define SUO_HIP_LIVE(x) do { if (!dry_run_) SUO_HIP_CHECK(x); } while (0)

// ---- algorithmic (compulsory) HBM bytes of a launch: every operand read once, every result written once, the weights once.  Summed per kind over the launch
// schedule by Net::schedule_bytes (a dry run): what bench.py's `roofline_all.whole_call` divides by the step time.  wb = bytes per weight element in the form the
// launch reads (4: fp32 or two fp16 planes; 6: three bf16 planes).
enum { ACCT_STAGE = 0, ACCT_CONV3 = 1, ACCT_GEMM = 2, ACCT_BLOCK = 3, ACCT_ELTWISE = 4, ACCT_DECODE = 5, ACCT_KINDS = 6 };
static double gemm_bytes(const GemmArgs& g, double wb) {
    const double M = g.M, nv = g.nchw_hw > 0 ? g.n_valid : g.N;
    double b = 4.0 * M * (g.K1 + g.K2) + (g.R ? 4.0 * M * g.N : 0.0) + wb * (double)g.N * (g.K1 + g.K2);
    if (g.out) b += 4.0 * M * nv;
    if (g.pool_out) b += 4.0 * (M / 4) * g.N;
    return b;
}
static double conv_bytes(const ConvArgs& c, double wb, int taps, bool fused) {
    const double pin = (double)c.L * c.H * c.W, pout = (double)c.L * c.OH * c.OW;
    double b = 4.0 * pin * c.C + wb * (double)c.N * c.C * taps;
    if (!fused) return b + 4.0 * pout * c.N;
    b += 4.0 * pout * c.N2 * 2 + wb * (double)c.N2 * c.N;                   // skip read, out2 written, conv3's weights
    if (c.up) b += 4.0 * (pout / 4) * c.N2;
    if (c.n_out) b += 4.0 * pout * 128 + wb * 128.0 * 256.0;               // the next block's conv1 written, its weights
    return b;
}
static double block_bytes(const ResBlockArgs& a, double wb) {
    const double px = (double)a.L * a.H * a.W;
    return 4.0 * px * 256 * (a.pool_in ? 4 : 1) + 4.0 * px * 256 + (a.up ? 4.0 * (px / 4) * 256 : 0.0) + wb * (256.0 * 128 + 128.0 * 128 * 9 + 128.0 * 256);
}

static double weight_bytes(int form) { return form == 1 ? 6 : 4; }      // per element: fp32 or two fp16 planes | three bf16 planes

// Launch-size thresholds of the split-operand kernels.  The Winograd kernels and the bf16x3 GEMM were introduced for batched calls and measured against the fp32-pipe
// kernels' smaller tiles: from 256 tiles of 8 x 16 pixels / 32768 rows up.  The fp16 forms changed the balance for calls of FEW crops (SLAM passes run 2-7): a fused fp16
// tail takes ~50 us whatever the crop count below 8 (one workgroup per CU) where direct 3x3 + conv3 take 84-106; measured per network call of L crops (bench.py --only cnn
// --objects L --frames-per-step 1, ms, thresholds 256 / 32768 -> 32 / 4096): L = 1 1.544 -> 1.531, 2 1.631 -> 1.567, 3 1.886 -> 1.678, 4 1.921 -> 1.726, 5 2.155 -> 1.759,
// 6 2.218 -> 1.800, 7 2.435 -> 1.832, 8 and up unchanged.
long Net::wino_min_tiles() const {
    static const long env = (long)SUO_TUNE("SUO_WINO_FUSE_TILES", -1);      // (0: never fuse)
    return env >= 0 ? env : (pipe_ == 2 ? 32 : 256);
}
long Net::x3_min_rows() const {
    static const long env = (long)SUO_TUNE("SUO_GEMM_X3_MIN_ROWS", -1);
    return env >= 0 ? env : (pipe_ == 2 ? 4096 : 32768);
}
// a 1x1 convolution of M rows as a launch of its own: large launches with a bf16x3 form of the weights run on the bf16 pipe (csrc/gemm_bf16x3.hip; 464 vs 595 us at
// 256 crops / 64 x 64; below ~256 tiles the fp32 kernels' smaller tiles win), as two fp16 terms where the network is on that form (csrc/f16x2.h)
int Net::gemm_form(const GemmW& gw, long M) const {
    return !gw.w.w[1] || M < x3_min_rows() ? 0 : (pipe_ == 2 && gw.w.w[2] ? 2 : 1);
}

// conv2 of a block at L x H x W, on the direct kernel's operands: what the kernels' shape predicates look at; residual() adds the tensors
static ConvArgs conv2_args(const ResidualW& r, int L, int H, int W) {
    ConvArgs c2 = {};
    c2.L = L; c2.H = H; c2.W = W; c2.C = r.c2.C; c2.Wp = r.c2.Wp; c2.bias = r.c2.bias; c2.OH = H; c2.OW = W; c2.N = r.c2.N; c2.relu = 1;
    return c2;
}

// Residual.forward (layers/Residual.py): THE place that decides how a block runs -- a pure function of the block, the call shape and the network's state.
Net::BlockPlan Net::plan_block(const ResidualW& r, int L, int H, int W) const {
    // A 256 -> 256 block on a small map in ONE launch (csrc/res_small_x3.hip / csrc/res_small.hip) instead of three: the call shape of the
    // reference (one frame = 8 crops per call, lib/object_slam.py:1099).  Measured per block at 8 crops (tools/bench_res_block.py, us; per-layer
    // launches -> one launch on the bf16 pipe): 32x32 47 -> 29.6, 16x16 26.6 -> 25.0; at 8x8 and 4x4 the three per-layer launches (13.5) stay
    // faster -- a workgroup streams all 0.85 / 1.28 MB of the block's weights through ONE CU whatever its tile, 20-24 us at 35 bytes per clock.
    //   SUO_RES_FUSED = 0: never; 1: the fp32-pipe kernel (bit-identical to the per-layer launches); 2 (default with SUO_WINO_BF16X3): the bf16x3 kernel
    //   SUO_RES_FUSED_MAX_TILES: largest launch (4 x 8 pixel tiles) that takes it; beyond that the Winograd kernels' larger tiles win
    static const int mode = (int)SUO_TUNE("SUO_RES_FUSED", 2);
    static const long max_tiles = (long)SUO_TUNE("SUO_RES_FUSED_MAX_TILES", 768);
    static const int min_side = (int)SUO_TUNE("SUO_RES_FUSED_MIN_SIDE", 16);
    // Half a round to three rounds of 4 x 8 pixel tiles (one workgroup per CU): the bf16x3 kernel, whatever the map (one frame at 32x32; batched frames at 8x8
    // and 4x4, where it replaces three launches of 17-47 us by one or two rounds of 30).  Fewer tiles than CUs on a map of >= 16 pixels a
    // side: the fp32 kernel's 4 x 4 tiles (16x16 at 8 crops: 128 workgroups x 23.4 us against 64 x 28).  Everything else -- few tiles on
    // 8x8 / 4x4 maps (the three per-layer launches spread over all CUs, 13.5 us), many tiles (the Winograd kernels) -- stays per-layer.
    // (129 ... 255 tiles, e.g. the 5 crops of a SLAM pass at 32x32: one partial round of the bf16x3 kernel, 30 us, against 4 x 4 tiles
    //  that no longer fit one per CU, ~40)
    static const long x3_from_env = (long)SUO_TUNE("SUO_RES_FUSED_X3_FROM", 129);
    // the fp16 form of the 4 x 8-tile kernel streams a third less weight per workgroup (csrc/res_small_x3.hip, NP = 2): 16.8 us at 64 tiles (16x16, 8 crops) where the
    // fp32 kernel's 128 tiles of 4 x 4 take 23.4 and the bf16x3 form 23.1 -- it takes over from 33 tiles (tools/bench_res_block.py; 8x8 at 8 crops = 16 tiles: 16.6
    // against 13.4 for the three per-layer launches, which stay)
    static const long f16_from = (long)SUO_TUNE("SUO_RES_FUSED_F16_FROM", 33);
    static const int carry_next = (int)SUO_TUNE("SUO_FUSE_NEXT_CONV1", 1);           // 0: A/B
    int one = 0;                                              // 1: csrc/res_small.hip; 2: csrc/res_small_x3.hip
    if (mode > 0 && r.block[0].w[0] && H <= 32 && W <= 32) {
        const long t32 = (long)L * ((H + 3) / 4) * ((W + 7) / 8);
        const long x3_from = (pipe_ == 2 && r.block[0].w[2] && mode >= 2) ? std::min(f16_from, x3_from_env) : x3_from_env;
        if (mode >= 2 && r.block[0].w[1] && t32 >= x3_from && t32 <= max_tiles) one = 2;
        else if (H >= min_side && W >= min_side && (t32 < x3_from || (mode == 1 && t32 <= max_tiles))) one = 1;
    }
    const ConvArgs c2 = conv2_args(r, L, H, W);
    const long M = (long)L * H * W, tiles = (long)((W + 15) / 16) * ((H + 7) / 8) * L, fuse_tiles = wino_min_tiles();      // (tiles of 8 x 16 pixels)
    // conv2 -> conv3 + skip can be one launch: the 128-channel tensor between them never leaves the CU
    const bool tail_shape = !r.has_skip_conv && r.c3.N == 256 && r.c3.n_valid == 256 && r.c3.K1 == 128 && r.cin == 256;
    BlockPlan p;
    p.wino = r.c2.wino.w[0] && conv3x3_wino_pays(c2, pipe_ == 2 ? 32 : -1);       // 2.25x fewer MFMA MACs (csrc/conv_wino.hip)
    if (probe_) p.route = BlockPlan::PER_LAYER;               // the calibration probe: every operand of the block's three sites in memory
    else if (one) p.route = BlockPlan::ONE_LAUNCH;
    else if (!p.wino && tail_shape && conv3x3_fusable(c2)) p.route = BlockPlan::DIRECT_FUSED;      // (csrc/conv.hip: FUSE)
    else if (p.wino && fuse_tiles > 0 && tiles >= fuse_tiles && tail_shape) p.route = BlockPlan::WINO_FUSED;      // (933 vs 713 + 346 us at 64x64 / 128 crops, 257 vs 195 + 91 at 32x32)
    const bool tail = p.route == BlockPlan::WINO_FUSED;
    // one launch: two fp16 planes stream a third less weight per workgroup and take half the MFMAs; Winograd: both products as two fp16 terms (csrc/f16x2.h),
    // else on the bf16 pipe with 3-way split operands, else fp32
    if (p.route == BlockPlan::ONE_LAUNCH) p.form = one == 2 ? (pipe_ == 2 && r.block[0].w[2] ? 2 : 1) : 0;
    else if (p.wino) p.form = pipe_ == 2 && r.c2.wino.w[2] && (!tail || r.tail.w[2]) ? 2 : (r.c2.wino.w[1] && (!tail || r.tail.w[1]) ? 1 : 0);
    p.form1 = gemm_form(r.c1, M); p.form3 = gemm_form(r.c3, M);
    // the fused Winograd tail is the only epilogue of the per-layer kernels that can add an up-sampled tensor
    p.takes_up = p.route == BlockPlan::ONE_LAUNCH || tail;
    // The next block's conv1 on the fused fp16 tail's tile while it is in the CU: its 256-channel input is written once and not re-read by a GEMM launch.
    // (Not with an up-sampled addend: that variant has no registers left -- measured no gain, tools/bench_f16x2.py; the eight-wave form of small launches
    //  does not carry it.)  It can ride there when the separate launch would have been the fp16 GEMM on the same operands (256 -> 128 with a BatchNorm
    // prologue, >= SUO_GEMM_X3_MIN_ROWS pixels, not a one-launch block): then the two are bit-identical (tests/test_gpu_f16x2.py)
    p.can_carry_next_conv1 = carry_next && tail && p.form == 2 && !conv3x3_wino_f16x2_w8(tiles);
    const bool from_tail = p.form1 == 2 && r.cin == 256 && r.c1.w.osc && r.c1.N == 128 && r.c1.n_valid == 128 && r.c1.K1 == 256 && r.c1.K2 == 0;
    p.uses_producer_conv1 = p.route != BlockPlan::ONE_LAUNCH && (from_tail || (&r == &r1_ && stem_computes_r1_conv1()));
    return p;
}

// the operands of a Winograd 3x3 (tail: and of its fused conv3) in the given form; returns the bytes per weight element the accounting uses
static double wino_operands(ConvArgs& c, const ResidualW& r, int form, bool tail, unsigned* range_flag) {
    c.Wp = r.c2.wino.w[form];
    if (tail) { c.W3p = r.tail.w[form]; c.w3_bf16x3 = form == 1; }
    if (form == 2) {
        c.oscale = r.c2.wino.osc; c.range_flag = range_flag; c.xscale = r.c2.xs16;
        if (tail) { c.oscale3 = r.tail.osc; c.xscale3 = r.c3.xs16; }
    }
    return weight_bytes(form);
}
static int launch_wino(const ConvArgs& c, int form, bool tail, hipStream_t s) {
    static int (*const launch[2][3])(const ConvArgs&, hipStream_t) = {{launch_conv3x3_wino, launch_conv3x3_wino_x3, launch_conv3x3_wino_f16x2},
                                                                     {launch_conv3x3_wino_fused, launch_conv3x3_wino_x3_fused, launch_conv3x3_wino_f16x2_fused}};
    return launch[tail][form](c, s);
}

int Net::residual_one_launch(const ResidualW& r, const BlockPlan& p, const float* x, float* out, int L, int H, int W, hipStream_t s, const float* up, bool pool_in) {
    ResBlockArgs a = {};
    a.x = x; a.L = L; a.H = H; a.W = W; a.pool_in = pool_in ? 1 : 0; a.pro_scale = r.pro_scale; a.pro_shift = r.pro_shift;
    a.b1 = r.c1.bias; a.b2 = r.c2.bias; a.b3 = r.c3.bias; a.up = up; a.out = out;
    a.W1 = r.block[0].w[p.form]; a.W2 = r.block[1].w[p.form]; a.W3 = r.block[2].w[p.form];
    if (p.form == 2) {
        a.osc1 = r.block[0].osc; a.osc2 = r.block[1].osc; a.osc3 = r.block[2].osc; a.range_flag = range_flag_;
        a.xs1 = r.c1.xs16; a.xs2 = r.c2.xs16; a.xs3 = r.c3.xs16;
    }
    acct(ACCT_BLOCK, block_bytes(a, weight_bytes(p.form)));
    static int (*const launch[3])(const ResBlockArgs&, hipStream_t) = {launch_res_block, launch_res_block_x3, launch_res_block_f16x2};
    SUO_LAUNCH(launch[p.form](a, s));
    return SUO_OK;
}

int Net::maxpool(const float* in, float* out, int L, int H, int W, int C, hipStream_t s) {
    acct(ACCT_ELTWISE, 4.0 * L * H * W * C * 1.25);
    SUO_LAUNCH(launch_maxpool2(in, out, L, H, W, C, s));
    return SUO_OK;
}

// A 1x1 convolution on the form the caller's plan gives (gemm_form), whose result may also be wanted max-pooled (nn.MaxPool2d(2, 2)): pooled in the GEMM's epilogue
// when the launch would use the persistent 128x128 kernel anyway (csrc/gemm_persist.hip: POOL), else GEMM + max-pool kernel.  g.out may be nullptr
// when only the pooled tensor is wanted.
int Net::gemm_maybe_pooled(GemmArgs& g, int L, int H, int W, float* pool_out, hipStream_t s, const GemmW& gw, int form) {
    static const int fuse_pool = (int)suo::env_switch("SUO_FUSE_POOL", 1);                    // 0: A/B
    if (form) {
        GemmArgs gx = g;
        gx.pool_out = pool_out; gx.pool_H = H; gx.pool_W = W;                  // the pool in the epilogue (maps of 64-column multiples), `out` optional
        if (form == 2) { gx.oscale = gw.w.osc; gx.range_flag = range_flag_; gx.xscale = gw.xs16; }      // the two-term fp16 form of the same kernel (csrc/f16x2.h)
        auto launch = [&](const GemmArgs& a) { return (form == 2 ? launch_gemm_f16x2_args : launch_gemm_bf16x3_args)(a, reinterpret_cast<const uint16_t*>(gw.w.w[form]), s); };
        const bool pool_in_gemm = gemm_bf16x3_takes(gx);
        if (!pool_in_gemm) gx.pool_out = nullptr;                             // else the pool as its own launch
        if (pool_in_gemm || (g.out && gemm_bf16x3_takes(gx))) {
            acct(ACCT_GEMM, gemm_bytes(gx, weight_bytes(form)));
            SUO_LAUNCH(launch(gx));
            return !pool_in_gemm && pool_out ? maxpool(g.out, pool_out, L, H, W, g.N, s) : SUO_OK;
        }
    }
    if (!pool_out) { acct(ACCT_GEMM, gemm_bytes(g, 4)); SUO_LAUNCH(launch_gemm1x1(g, s)); return SUO_OK; }
    GemmArgs gp = g;
    gp.pool_out = pool_out; gp.pool_H = H; gp.pool_W = W;
    const long tiles128 = (long)(g.M / 128) * (g.N / 128);
    if (fuse_pool && g.M > 4096 && tiles128 >= 512 && gemm1x1_can_pool(gp)) { acct(ACCT_GEMM, gemm_bytes(gp, 4)); SUO_LAUNCH(launch_gemm1x1(gp, s)); return SUO_OK; }
    if (!g.out) g.out = alloc((size_t)g.M * g.ldo);
    acct(ACCT_GEMM, gemm_bytes(g, 4));
    SUO_LAUNCH(launch_gemm1x1(g, s));
    return maxpool(g.out, pool_out, L, H, W, g.N, s);
}

// Executes plan_block's plan; no decision of its own.  (The sequence of alloc calls per route is part of the behaviour: captured graphs hold the addresses.)
int Net::residual(const ResidualW& r, const float* x, float* out, int L, int H, int W, hipStream_t s, const float* up, float* pool_out, const ResidualW* next) {
    const BlockPlan p = plan_block(r, L, H, W);
    const int M = L * H * W;
    if (up && !p.takes_up) { suo_set_error("residual: an up-sampled addend needs a one-launch block or the fused Winograd tail"); return SUO_ERR_ARG; }
    if (p.route == BlockPlan::ONE_LAUNCH) {
        if (!out) out = alloc((size_t)M * 256);
        SUO_TRY(residual_one_launch(r, p, x, out, L, H, W, s, up, false));
        return pool_out ? maxpool(out, pool_out, L, H, W, 256, s) : SUO_OK;
    }
    float* mid1 = nullptr;
    for (size_t i = 0; p.uses_producer_conv1 && i < pre_.size(); ++i)
        if (pre_[i].x == x && pre_[i].r == &r) {              // conv1 came with the producer's launch (a fused tail's NEXT, the fused stem's)
            mid1 = pre_[i].mid1;
            pre_.erase(pre_.begin() + i);
            break;
        }
    if (!mid1) {
        mid1 = alloc((size_t)M * r.c1.N);
        GemmArgs g1 = {};
        g1.A1 = x; g1.lda1 = r.cin; g1.K1 = r.c1.K1; g1.pro_scale = r.pro_scale; g1.pro_shift = r.pro_shift;
        g1.Wp = r.c1.w.w[0]; g1.bias = r.c1.bias; g1.out = mid1; g1.ldo = r.c1.N; g1.M = M; g1.N = r.c1.N; g1.n_valid = r.c1.n_valid; g1.relu = 1;
        SUO_TRY(gemm_maybe_pooled(g1, L, H, W, nullptr, s, r.c1, p.form1));
    }
    float* mid2 = alloc((size_t)M * r.c2.N);
    ConvArgs c2 = conv2_args(r, L, H, W);
    c2.in = mid1; c2.out = mid2;
    const bool tail = p.route != BlockPlan::PER_LAYER;       // conv2 -> conv3 + skip in one launch
    if (tail) {
        if (!out) out = alloc((size_t)M * 256);
        c2.W3p = r.c3.w.w[0]; c2.bias3 = r.c3.bias; c2.R = x; c2.out2 = out; c2.N2 = 256; c2.up = up;
    }
    const double wb = p.wino ? wino_operands(c2, r, p.form, tail, range_flag_) : 4;
    if (next && !up && !pool_out && p.can_carry_next_conv1 && plan_block(*next, L, H, W).uses_producer_conv1) {
        float* nm = alloc((size_t)M * 128);
        c2.n_scale = next->pro_scale; c2.n_shift = next->pro_shift; c2.n_W1 = next->c1.w.w[2]; c2.n_osc1 = next->c1.w.osc; c2.n_b1 = next->c1.bias; c2.n_out = nm; c2.n_xscale = next->c1.xs16;
        pre_.push_back({out, next, nm});
    }
    acct(ACCT_CONV3, conv_bytes(c2, wb, p.wino ? 16 : 9, tail));
    SUO_LAUNCH(p.wino ? launch_wino(c2, p.form, tail, s) : tail ? launch_conv3x3_fused(c2, s) : launch_conv3x3(c2, s));
    if (tail) return pool_out ? maxpool(out, pool_out, L, H, W, 256, s) : SUO_OK;
    GemmArgs g3 = {};
    g3.A1 = mid2; g3.lda1 = r.c2.N; g3.K1 = r.c3.K1;
    if (r.has_skip_conv) { g3.A2 = x; g3.lda2 = r.cin; g3.K2 = r.c3.K2; }
    else { g3.R = x; g3.ldr = r.cin; }
    g3.Wp = r.c3.w.w[0]; g3.bias = r.c3.bias; g3.out = out; g3.ldo = r.cout; g3.M = M; g3.N = r.c3.N; g3.n_valid = r.c3.n_valid;
    if (probe_) {                                             // the calibration probe: every operand of the block's three sites is in memory here
        SUO_TRY(probe_site(r.c1.site, x, M, r.cin, r.cin, r.pro_scale, r.pro_shift, 1, s));
        SUO_TRY(probe_site(r.c2.site, mid1, M, r.c1.N, r.c1.N, nullptr, nullptr, 0, s));
        SUO_TRY(probe_site(r.c3.site, mid2, M, r.c2.N, r.c2.N, nullptr, nullptr, 0, s));
        if (r.has_skip_conv) SUO_TRY(probe_site(r.c3.site, x, M, r.cin, r.cin, nullptr, nullptr, 0, s));      // (conv4's segment of the same split operand)
    }
    return gemm_maybe_pooled(g3, L, H, W, pool_out, s, r.c3, p.form3);
}

// Hourglass.forward (hg.py:37-58).  The up1 branch is independent of the low branch until the
// final add: it can run on a side stream (fork/join with events) so the small, latency-bound low
// levels overlap with the large up1 kernels -- see n_side below for when that pays.
int Net::hourglass(const HourglassW& h, const float* x, float* out, int L, int H, int W, hipStream_t s, int depth_idx, const float* x_pooled) {
    const int C = 256;
    const size_t n_hi = (size_t)L * H * W * C, n_lo = n_hi / 4;
    // Side streams for the up1 branch are OFF by default (SUO_NET_SIDE_STREAMS=1|2 turns them on).  Measured on MI355X with the
    // harness's two network calls in flight: one frame (8 crops) per call 351 frames/s with two side streams, 415 with one, 426
    // with none; 32 frames per call 738 / 745 / 749.  The second call in flight already fills the gaps the fork was meant to fill,
    // and every extra stream competes for the 4 hardware queues with the other network and the geometry stream.  With a single
    // call in flight the fork is worth about 1 % (385 vs 381 frames/s at 8 crops).
    static const int n_side = std::max(0, std::min(kNumSide, (int)env_switch("SUO_NET_SIDE_STREAMS", 0)));
    // ... except on the SMALL maps of a call of few crops (the one-frame call: 16x16 and 8x8 at 8 crops): there every kernel is a handful of workgroups and a
    // dependent launch costs its latency, not its work -- the up1 blocks (16.8 / 2 x 13.4 us) run beside the low branch instead of in front of it.
    // SUO_NET_FORK_SMALL_PIXELS: largest L * H * W that forks (2048 = 16x16 at 8 crops); default 0 = never: MEASURED SLOWER -- one frame per call 2.010 ms with
    // the fork against 1.897 without (same box, tools/time_frame_chain.py): the captured graph's extra branch costs more than the two or three launches it hides.
    static const long fork_small = (long)SUO_TUNE("SUO_NET_FORK_SMALL_PIXELS", 0);
    const bool small_fork = !env_set("SUO_SERIAL") && fork_small > 0 && (long)L * H * W <= fork_small && H >= 8;
    const bool serial = (env_set("SUO_SERIAL") || n_side == 0) && !small_fork;     // one stream, kernels back to back
    hipStream_t side = serial ? s : side_[depth_idx % (n_side > 0 ? n_side : kNumSide)];
    hipEvent_t ev_fork = ev_[(ev_next_++) % (kNumEvents - 1)], ev_join = ev_[(ev_next_++) % (kNumEvents - 1)];      // (the last event is follow_null_stream's)
    float* up_a = alloc(n_hi);
    float* up_b = alloc(n_hi);
    SUO_HIP_LIVE(hipEventRecord(ev_fork, s));
    SUO_HIP_LIVE(hipStreamWaitEvent(side, ev_fork, 0));
    // "up1 + up2(low3)" (hg.py:56-58): when the last up1 block ends in the fused Winograd tail, that tail adds the up-sampled low
    // branch itself and writes `out` -- no up-sample kernel, no extra pass over the high-resolution tensor.  The block then has to
    // wait for the low branch; its predecessor still runs beside it on the side stream.
    static const int fuse_up = (int)suo::env_switch("SUO_FUSE_UPSAMPLE", 1);              // 0: A/B
    const bool up_in_tail = fuse_up && plan_block(h.up1[1], L, H, W).takes_up;
    SUO_TRY(residual(h.up1[0], x, up_a, L, H, W, side, nullptr, nullptr, &h.up1[1]));
    if (!up_in_tail) SUO_TRY(residual(h.up1[1], up_a, up_b, L, H, W, side));
    SUO_HIP_LIVE(hipEventRecord(ev_join, side));

    const float* pooled = x_pooled;                           // (the caller's producer kernel may have pooled x already)
    // max_pool2d(x) (hg.py:41) has ONE reader, the first low block: when that block runs in one launch it takes the pool while staging x
    static const int pool_in_block = (int)SUO_TUNE("SUO_RES_POOL_IN", 1);           // 0: A/B
    const BlockPlan low1 = plan_block(h.low1[0], L, H / 2, W / 2);
    const bool pool_by_block = !pooled && pool_in_block && low1.route == BlockPlan::ONE_LAUNCH && (H % 2 == 0) && (W % 2 == 0);
    if (!pooled && !pool_by_block) {
        float* p = alloc(n_lo);
        SUO_TRY(maxpool(x, p, L, H, W, C, s));
        pooled = p;
    }
    float* lo_a = alloc(n_lo);
    float* lo_b = alloc(n_lo);
    if (pool_by_block) SUO_TRY(residual_one_launch(h.low1[0], low1, x, lo_a, L, H / 2, W / 2, s, nullptr, true));
    else SUO_TRY(residual(h.low1[0], pooled, lo_a, L, H / 2, W / 2, s, nullptr, nullptr, &h.low1[1]));
    // (lo_b has two readers -- the inner hourglass's up1[0] and, pooled, its low1[0]: the first one's conv1 rides along)
    SUO_TRY(residual(h.low1[1], lo_a, lo_b, L, H / 2, W / 2, s, nullptr, nullptr, h.n > 1 ? &h.inner->up1[0] : &h.low2[0]));
    float* low2 = alloc(n_lo);
    if (h.n > 1) {
        SUO_TRY(hourglass(*h.inner, lo_b, low2, L, H / 2, W / 2, s, depth_idx + 1));
    } else {
        float* t = alloc(n_lo);
        SUO_TRY(residual(h.low2[0], lo_b, t, L, H / 2, W / 2, s, nullptr, nullptr, &h.low2[1]));
        SUO_TRY(residual(h.low2[1], t, low2, L, H / 2, W / 2, s, nullptr, nullptr, &h.low3[0]));
    }
    float* l3a = alloc(n_lo);
    float* l3b = alloc(n_lo);
    SUO_TRY(residual(h.low3[0], low2, l3a, L, H / 2, W / 2, s, nullptr, nullptr, &h.low3[1]));
    SUO_TRY(residual(h.low3[1], l3a, l3b, L, H / 2, W / 2, s));
    SUO_HIP_LIVE(hipStreamWaitEvent(s, ev_join, 0));
    if (up_in_tail) SUO_TRY(residual(h.up1[1], up_a, out, L, H, W, s, l3b));
    else { acct(ACCT_ELTWISE, 4.0 * L * H * W * C * 2.25); SUO_LAUNCH(launch_upsample2_add(up_b, l3b, out, L, H, W, C, s)); }
    return SUO_OK;
}

// HourglassNet.forward (hg.py:95-119) from the staged NHWC input to NCHW logits
int Net::backbone(const float* in0, int in_c, float* logits, int L, hipStream_t s, bool stem_done) {
    ws_used_ = ws_mark_;
    ev_next_ = 0;
    pre_.clear();
    float* stem = stem_slab_;
    if (stem_done && plan_block(r1_, L, 128, 128).uses_producer_conv1) pre_.push_back({stem, &r1_, stem_mid1_slab_});      // (the fused stem launch leaves r1's conv1 there)
    if (!stem_done) {                                          // (the fused stem of the prior-less pass has filled the slab already: csrc/stem_x3.hip)
        ConvArgs c = {};
        const ConvW& sw = in_c == IMG_C ? stem_img_ : stem_;
        c.in = in0; c.L = L; c.H = CROP; c.W = CROP; c.C = in_c; c.Wp = sw.Wp; c.bias = sw.bias;
        c.out = stem; c.OH = 128; c.OW = 128; c.N = 64; c.relu = 1;
        acct(ACCT_STAGE, conv_bytes(c, 4, 49, false));
        SUO_LAUNCH(launch_conv7x7s2(c, s));
    }
    // pool(r1(x)): the full-resolution r1 output has no other reader, so only its pooled form is written (csrc/gemm_persist.hip: POOL)
    float* p1 = alloc((size_t)L * 64 * 64 * 128);
    SUO_TRY(residual(r1_, stem, nullptr, L, 128, 128, s, nullptr, p1));
    float* r4o = alloc((size_t)L * 64 * 64 * 128);
    SUO_TRY(residual(r4_, p1, r4o, L, 64, 64, s));
    float* x = alloc((size_t)L * 64 * 64 * 256);
    float* xp = alloc((size_t)L * 32 * 32 * 256);             // max_pool2d(x): the first thing each Hourglass computes from x (hg.py:41)
    SUO_TRY(residual(r5_, r4o, x, L, 64, 64, s, nullptr, xp));
    const int M = L * 64 * 64;
    for (int i = 0; i < 2; ++i) {
        float* hg = alloc((size_t)M * 256);
        SUO_TRY(hourglass(hg_[i], x, hg, L, 64, 64, s, 0, xp));
        float* ra = alloc((size_t)M * 256);
        float* rb = alloc((size_t)M * 256);
        SUO_TRY(residual(post_[i][0], hg, ra, L, 64, 64, s, nullptr, nullptr, &post_[i][1]));
        SUO_TRY(residual(post_[i][1], ra, rb, L, 64, 64, s));
        // the last stack's lin -> head pair: `ll` has one reader, so it never leaves the CU (one launch, 1.2 GB of traffic instead of 3.3 at 256 crops)
        static const int chain_head = (int)SUO_TUNE("SUO_CHAIN_HEAD", 1);            // 0: A/B
        const long chain_min_rows = x3_min_rows();
        if (i == 1 && chain_head && pipe_ == 2 && lin_[i].w.w[2] && head_[i].w.w[2] && lin_[i].N == 256 && lin_[i].K1 == 256 && M >= chain_min_rows &&
            gemm_chain_head_takes(M, 256, NUM_KP, HEAT * HEAT)) {
            acct(ACCT_GEMM, 4.0 * M * 256 + 4.0 * M * NUM_KP + 4.0 * (256.0 * 256 + 64.0 * 256));
            SUO_LAUNCH(launch_gemm_chain_head(rb, 256, M, reinterpret_cast<const uint16_t*>(lin_[i].w.w[2]), lin_[i].w.osc, lin_[i].bias, reinterpret_cast<const uint16_t*>(head_[i].w.w[2]),
                                              head_[i].w.osc, head_[i].bias, logits, NUM_KP, HEAT * HEAT, range_flag_, s, lin_[i].xs16, head_[i].xs16));
            continue;
        }
        float* ll = alloc((size_t)M * 256);
        GemmArgs gl = {};
        gl.A1 = rb; gl.lda1 = 256; gl.K1 = 256; gl.Wp = lin_[i].w.w[0]; gl.bias = lin_[i].bias; gl.out = ll; gl.ldo = 256;
        gl.M = M; gl.N = 256; gl.n_valid = 256; gl.relu = 1;
        SUO_TRY(gemm_maybe_pooled(gl, L, 64, 64, nullptr, s, lin_[i], gemm_form(lin_[i], M)));
        if (probe_) {
            SUO_TRY(probe_site(lin_[i].site, rb, M, 256, 256, nullptr, nullptr, 0, s));
            SUO_TRY(probe_site(head_[i].site, ll, M, 256, 256, nullptr, nullptr, 0, s));
            if (i == 0) SUO_TRY(probe_site(reinject_.site, ll, M, 256, 256, nullptr, nullptr, 0, s));
        }
        GemmArgs gh = {};
        gh.A1 = ll; gh.lda1 = 256; gh.K1 = 256; gh.Wp = head_[i].w.w[0]; gh.bias = head_[i].bias; gh.M = M; gh.N = 64;
        if (i == 0) {
            // x <- x + ll_(ll) + tmpOut_(tmpOut(ll)) as one folded GEMM + residual (see the constructor)
            float* xn = alloc((size_t)M * 256);
            GemmArgs gr = {};
            gr.A1 = ll; gr.lda1 = 256; gr.K1 = 256;
            gr.Wp = reinject_.w.w[0]; gr.bias = reinject_.bias; gr.R = x; gr.ldr = 256; gr.out = xn; gr.ldo = 256;
            gr.M = M; gr.N = 256; gr.n_valid = 256;
            xp = alloc((size_t)L * 32 * 32 * 256);
            SUO_TRY(gemm_maybe_pooled(gr, L, 64, 64, xp, s, reinject_, gemm_form(reinject_, M)));
            x = xn;
        } else {
            gh.out = logits; gh.n_valid = NUM_KP; gh.nchw_hw = HEAT * HEAT;
            acct(ACCT_GEMM, gemm_bytes(gh, 4));
            SUO_LAUNCH(launch_gemm1x1(gh, s));
        }
    }
    return SUO_OK;
}

int Net::ensure_graph(float* in0, int in_c, float* logits, int L, hipStream_t s, hipGraphExec_t* exec, bool stem_done) {
    const int key = (L * 4 + (in_c == IMG_C ? 1 : 0) + (stem_done ? 2 : 0)) * 4 + pipe_;      // one captured graph per (crop count, staging layout, with / without the stem, pipe)
    auto it = graphs_.find(key);
    if (it == graphs_.end()) {
        GraphEntry ge;
        SUO_HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed));
        int r;
        try {
            r = backbone(in0, in_c, logits, L, s, stem_done);
        } catch (...) {                                   // (an exception inside the schedule must not leave the stream capturing)
            hipGraph_t dead = nullptr;
            (void)hipStreamEndCapture(s, &dead);
            if (dead) (void)hipGraphDestroy(dead);
            throw;
        }
        hipError_t e = hipStreamEndCapture(s, &ge.graph);
        if (r != SUO_OK) return r;
        SUO_HIP_CHECK(e);
        for (int i = 0; i < 2; ++i) SUO_HIP_CHECK(hipGraphInstantiate(&ge.exec[i], ge.graph, nullptr, nullptr, 0));
        it = graphs_.emplace(key, ge).first;
    }
    *exec = it->second.exec[it->second.next];
    it->second.next ^= 1;
    return SUO_OK;
}

int Net::run_backbone(float* in0, int in_c, float* logits, int L, hipStream_t s, bool stem_done) {
    if (use_graph_) {
        hipGraphExec_t exec = nullptr;
        SUO_TRY(ensure_graph(in0, in_c, logits, L, s, &exec, stem_done));
        SUO_HIP_CHECK(hipGraphLaunch(exec, s));
        return SUO_OK;
    }
    return backbone(in0, in_c, logits, L, s, stem_done);
}

// A NULL-stream call runs on an internal NON-BLOCKING stream, which the legacy NULL stream does not order: whatever the caller enqueued there before the call
// (the frame's upload kernel, torch ops that produced the boxes) must have run before this call's first kernel reads it.
int Net::follow_null_stream() {
    hipEvent_t ev = ev_[kNumEvents - 1];
    SUO_HIP_CHECK(hipEventRecord(ev, nullptr));
    SUO_HIP_CHECK(hipStreamWaitEvent(own_stream_, ev, 0));
    return SUO_OK;
}

int Net::set_pipe(int p) {
    if (p < 0 || p > pipe_built_ || (p == 0 && pipe_built_ != 0)) {
        suo_set_error("suo_net_set_pipe: pipe %d not available (this network was built for pipe %d; the fp32 pipe needs SUO_WINO_BF16X3=0 at creation)", p, pipe_built_);
        return SUO_ERR_ARG;
    }
    pipe_ = p;
    return SUO_OK;
}

// ---- per-site activation exponents (csrc/f16x2.h) ----------------------------------------------------------------------------------------------------------
int Net::get_f16x2_shifts(int* out, int n) const {
    if (!out || n != (int)sites_.size()) { suo_set_error("suo_net_get_f16x2_shifts: %d entries asked, the network has %d sites", n, (int)sites_.size()); return SUO_ERR_ARG; }
    for (int i = 0; i < n; ++i) out[i] = sites_[i].shift;
    return SUO_OK;
}

// Rewrites every site's 2^s and its convolution's per-channel factors 2^-(t_n + s) in place, after the device has finished whatever used them.  A network built for
// the fp16 form returns to it (the only way up: the factors now fit the data the caller calibrated on / vouches for).
int Net::apply_shifts(const std::vector<int>& sh) {
    SUO_HIP_CHECK(hipDeviceSynchronize());
    std::vector<float> xs(kMaxSites, S2_XSCALE);
    for (size_t i = 0; i < sites_.size(); ++i) xs[i] = ldexpf(1.f, sh[i]);
    SUO_HIP_CHECK(hipMemcpy(site_xs_, xs.data(), xs.size() * sizeof(float), hipMemcpyHostToDevice));
    for (size_t i = 0; i < sites_.size(); ++i) {
        for (auto& o : sites_[i].osc) {
            std::vector<float> v(o.second.size());
            for (size_t k = 0; k < v.size(); ++k) v[k] = ldexpf(o.second[k], S2_XSHIFT - sh[i]);      // exact: 2^-(t_n + 4) -> 2^-(t_n + s), both normal
            SUO_HIP_CHECK(hipMemcpy(o.first, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        sites_[i].shift = sh[i];
    }
    if (pipe_built_ == 2) pipe_ = 2;
    return SUO_OK;
}

int Net::set_f16x2_shifts(const int* s, int n) {
    if (sites_.empty()) { suo_set_error("suo_net_set_f16x2_shifts: this network has no fp16 form (built with SUO_F16X2=0 or SUO_WINO_BF16X3=0)"); return SUO_ERR_ARG; }
    if (!s || n != (int)sites_.size()) { suo_set_error("suo_net_set_f16x2_shifts: %d shifts given, the network has %d sites", n, (int)sites_.size()); return SUO_ERR_ARG; }
    for (int i = 0; i < n; ++i)
        if (s[i] < S2_SHIFT_MIN || s[i] > S2_SHIFT_MAX) {
            suo_set_error("suo_net_set_f16x2_shifts: shift %d of site %s outside [%d, %d]", s[i], sites_[i].name.c_str(), S2_SHIFT_MIN, S2_SHIFT_MAX);
            return SUO_ERR_ARG;
        }
    return apply_shifts(std::vector<int>(s, s + n));
}

int Net::probe_site(int site, const float* x, long rows, int C, int ld, const float* scale, const float* shift, int relu, hipStream_t s) {
    if (site < 0) return SUO_OK;
    if (!dry_run_) probed_[site] = 1;
    SUO_LAUNCH(launch_absmax(x, rows, C, ld, scale, shift, relu, probe_max_ + site, s));
    return SUO_OK;
}

// The probe: the prior-less pass of suo_net_forward_frames on the bf16x3 form (fp32's range: an operand far beyond fp16's cannot corrupt what follows it) with
// every block on its per-layer launches, so each site's operand is in memory once -- whichever kernel would compute it on the fp16 form at whatever crop count --
// and one reduction per site measures it.  Its intermediates get a workspace of their own; nothing of the network's numbered calls or range record changes.
int Net::calibrate(const void* img, int fmt, int H, int W, const float* boxes, const int* box_img, int L, hipStream_t s) {
    if (sites_.empty()) { suo_set_error("suo_net_calibrate: this network has no fp16 form (built with SUO_F16X2=0 or SUO_WINO_BF16X3=0)"); return SUO_ERR_ARG; }
    if (L <= 0 || L > max_crops_) { suo_set_error("suo_net_calibrate: L=%d outside [1,%d]", L, max_crops_); return SUO_ERR_ARG; }
    const bool own = (s == nullptr);
    if (own) { s = own_stream_; SUO_TRY(follow_null_stream()); }
    SUO_HIP_CHECK(hipDeviceSynchronize());                    // the network's calls in flight have finished with the factors and the slabs
    float* const ws = ws_; const size_t ws_floats = ws_floats_, ws_used = ws_used_, ws_mark = ws_mark_;
    float* const stem_slab = stem_slab_; float* const mid1_slab = stem_mid1_slab_;
    const int pipe = pipe_;
    float* pws = nullptr;
    auto restore = [&]() {
        ws_ = ws; ws_floats_ = ws_floats; ws_used_ = ws_used; ws_mark_ = ws_mark; stem_slab_ = stem_slab; stem_mid1_slab_ = mid1_slab;
        pipe_ = pipe; probe_ = false; dry_run_ = false;
        if (pws) { (void)hipStreamSynchronize(s); (void)hipFree(pws); }
    };
    std::vector<unsigned> bits(sites_.size(), 0u);
    auto run = [&]() -> int {
        probe_ = true;
        pipe_ = 1;
        probed_.assign(sites_.size(), 0);
        for (int pass = 0; pass < 2; ++pass) {                // pass 0: a dry run sizes the workspace; pass 1 runs
            dry_run_ = pass == 0;
            if (pass == 0) ws_floats_ = (size_t)-1 / sizeof(float) / 2;
            else {
                const size_t need = ws_used_;
                SUO_HIP_CHECK(hipMalloc(&pws, need * sizeof(float)));
                ws_ = pws; ws_floats_ = need;
            }
            ws_used_ = 0;
            float* in0 = alloc((size_t)L * CROP * CROP * IN_C);
            float* logits = alloc((size_t)L * NUM_KP * HEAT * HEAT);
            stem_slab_ = alloc((size_t)L * 128 * 128 * 64);
            stem_mid1_slab_ = nullptr;
            ws_mark_ = ws_used_;
            if (pass == 1) {
                SUO_HIP_CHECK(hipMemsetAsync(probe_max_, 0, sites_.size() * sizeof(unsigned), s));
                SUO_TRY(launch_roi_align_concat(img, fmt, H, W, boxes, box_img, L, IMG_C, nullptr, nullptr, nullptr, in0, s));
            }
            SUO_TRY(backbone(in0, IMG_C, logits, L, s, false));
        }
        SUO_HIP_CHECK(hipMemcpyAsync(bits.data(), probe_max_, bits.size() * sizeof(unsigned), hipMemcpyDeviceToHost, s));
        SUO_HIP_CHECK(hipStreamSynchronize(s));
        return SUO_OK;
    };
    int rc;
    try {
        rc = run();
    } catch (const std::exception& e) {
        suo_set_error("suo_net_calibrate: %s", e.what());
        rc = SUO_ERR_ARG;
    }
    restore();
    if (rc != SUO_OK) return rc;
    std::vector<int> sh(sites_.size());
    for (size_t i = 0; i < sites_.size(); ++i) {
        float m;
        memcpy(&m, &bits[i], sizeof(float));
        if (!probed_[i]) { suo_set_error("suo_net_calibrate: the probe did not measure site %s", sites_[i].name.c_str()); return SUO_ERR_ARG; }
        if (!s2_site_shift(m, sites_[i].ksize, &sh[i])) { suo_set_error("suo_net_calibrate: site %s has max |x| = %g", sites_[i].name.c_str(), (double)m); return SUO_ERR_ARG; }
    }
    return apply_shifts(sh);
}

// The contract of the fp16 form (csrc/f16x2.h): a forward whose activations left fp16's range has INVALID outputs.  Whoever synchronised on them asks before
// using them -- per call (call_range_exceeded) or for every forward since the last time it asked (range_exceeded); on 1 the network has already been moved to
// the bf16 form (which has fp32's range) and the caller re-issues the call.  The blocking entries (stream == NULL) do this themselves.
void Net::leave_fp16_form() {
    if (pipe_ != 2) return;
    pipe_ = 1;
    fprintf(stderr, "libsuo_hip: an activation left the fp16 range of its site; this network now runs the three-term bf16 form -- re-issue the call\n");
}

int Net::range_exceeded() {
    const unsigned f = __atomic_exchange_n(range_flag_ + kStickyWord, 0u, __ATOMIC_RELAXED);
    if (!f) return 0;
    leave_fp16_form();
    return 1;
}

static unsigned call_tag(uint64_t call) { return (unsigned)(call & 0x7fffffffu); }

// Ends every forward, behind its last launch on its stream: numbers the call and, on the fp16 form, enqueues the one-lane launch that moves the live flag into
// the call's slot (csrc/misc.hip: range_commit_kernel).  In stream order the slot holds exactly this call's raises -- a later call still running cannot reach it.
// The other forms cannot leave the range: their calls get no launch, the host remembers the pipe.
int Net::commit_call(hipStream_t s) {
    const uint64_t c = ++calls_;
    const int i = (int)(c % kCallRing);
    call_pipe_[i] = pipe_;
    if (pipe_ != 2) return SUO_OK;
    return launch_range_commit(range_flag_ + kLiveWord, range_flag_ + kStickyWord, range_flag_ + kSlotWord + i, call_tag(c), s);
}

int Net::call_range_exceeded(uint64_t call) {
    if (call == 0 || call > calls_ || calls_ - call >= (uint64_t)kCallRing) {
        suo_set_error("suo_net_call_range_exceeded: call %llu is not one of the last %d forwards of this network (calls issued: %llu)", (unsigned long long)call,
                      kCallRing, (unsigned long long)calls_);
        return -1;
    }
    const int i = (int)(call % kCallRing);
    if (call_pipe_[i] != 2) return 0;
    const unsigned v = __atomic_load_n(range_flag_ + kSlotWord + i, __ATOMIC_ACQUIRE);
    if ((v >> 1) != call_tag(call)) {
        suo_set_error("suo_net_call_range_exceeded: call %llu has not finished -- synchronise on its outputs first", (unsigned long long)call);
        return -1;
    }
    if (!(v & 1u)) return 0;
    leave_fp16_form();
    return 1;
}

// A blocking entry (synchronised) asks about its own call; it re-issues an invalid one itself, so the raise is answered for range_exceeded()'s readers as well
// (as it always was).
bool Net::own_call_invalid() {
    if (call_range_exceeded(calls_) != 1) return false;
    (void)range_exceeded();
    return true;
}

// The launch schedule of ONE call of L crops cut from n_frames frames of H x W (with_priors: the 48-channel staging + full stem) walked as a dry run (nothing is
// launched, nothing allocated): algorithmic HBM bytes per kind of launch -- out[0..5] = staging / stem, 3x3 (+ fused tails), 1x1 GEMMs, one-launch blocks,
// pool / up-sample, decode + classifier -- and the number of launches.
int Net::schedule_bytes(int L, int n_frames, int H, int W, int with_priors, double* out, int* n_launches) {
    if (L <= 0 || L > max_crops_ || !out) { suo_set_error("suo_net_schedule_bytes: L=%d outside [1,%d] or null output", L, max_crops_); return SUO_ERR_ARG; }
    const bool was_dry = dry_run_;
    dry_run_ = true; acct_on_ = true; acct_launches_ = 0;
    for (int k = 0; k < ACCT_KINDS; ++k) acct_[k] = 0.0;
    int rc = SUO_OK;
    try {
        const double frame_bytes = (double)n_frames * H * W * 3;
        const int in_c = with_priors ? IN_C : IMG_C;
        const bool fstem = !with_priors && fused_stem();
        if (fstem) {
            acct(ACCT_STAGE, frame_bytes + 4.0 * L * 128 * 128 * 64 * (stem_computes_r1_conv1() ? 2 : 1) + 4.0 * 64 * 147);
            ++acct_launches_;
        } else {
            acct(ACCT_STAGE, frame_bytes + 4.0 * L * CROP * CROP * in_c + (with_priors ? 8.0 * L * NUM_KP : 0.0));
            ++acct_launches_;
        }
        rc = backbone(nullptr, in_c, nullptr, L, nullptr, fstem);
        acct(ACCT_DECODE, 4.0 * L * NUM_KP * (HEAT * HEAT + 2 + 4 + 1) + 4.0 * L * NUM_KP * 3 + 4.0 * NUM_KP * (NUM_KP + 1));
        acct_launches_ += 2;
    } catch (const std::exception& e) {
        suo_set_error("suo_net_schedule_bytes: %s", e.what());
        rc = SUO_ERR_ARG;
    }
    dry_run_ = was_dry; acct_on_ = false;
    for (int k = 0; k < ACCT_KINDS; ++k) out[k] = acct_[k];
    if (n_launches) *n_launches = acct_launches_;
    return rc;
}

// SUO_STEM_X3=0: the prior-less pass stages the crop (roi_align_concat_kernel) and runs the stem on the fp32 pipe inside the backbone, as rounds 1-3 did
// the fused stem launch of the fp16 pipe also computes r1's conv1 on its tile (csrc/stem_x3.hip: NEXT); a function of the network's state only -- suo_net_prepare captures the
// backbone without launching the stem
bool Net::stem_computes_r1_conv1() const {
    static const int on = (int)SUO_TUNE("SUO_STEM_NEXT", 1);              // 0: A/B
    return on && fused_stem() && pipe_ == 2 && stem_x3_.w[2] && r1_.c1.w.w[2] && r1_.c1.w.osc && r1_.cin == 64 && r1_.c1.N == 64 && r1_.c1.K1 == 64 && r1_.c1.K2 == 0;
}
bool Net::fused_stem() const {
    static const int on = (int)suo::env_switch("SUO_STEM_X3", 1);
    return on != 0 && stem_x3_.w[1] != nullptr;
}

// Capture the backbone graph for L crops ahead of time (nothing runs): a stream of frames with a varying number of
// detections then never pays a capture inside a timed / latency-critical call.
int Net::prepare(int L, int with_priors, hipStream_t s) {
    if (L <= 0 || L > max_crops_) { suo_set_error("suo_net_prepare: L=%d outside [1,%d]", L, max_crops_); return SUO_ERR_ARG; }
    if (!use_graph_) return SUO_OK;
    const bool own = (s == nullptr);
    if (own) s = own_stream_;
    try {
        auto [in0, logits] = layout_slabs();
        hipGraphExec_t exec = nullptr;
        SUO_TRY(ensure_graph(in0, with_priors ? IN_C : IMG_C, logits, L, s, &exec, !with_priors && fused_stem()));
    } catch (const std::exception& e) {
        suo_set_error("suo_net_prepare: %s", e.what());
        return SUO_ERR_ARG;
    }
    return SUO_OK;
}

// Backbone only, from an already staged NHWC [L,256,256,48] input (test / profiling entry).
int Net::forward_staged(const float* in0_user, int L, float* logits_out, hipStream_t s) {
    if (L <= 0 || L > max_crops_) { suo_set_error("suo_net_backbone: L=%d outside [1,%d]", L, max_crops_); return SUO_ERR_ARG; }
    const bool own = (s == nullptr);
    if (own) { s = own_stream_; SUO_TRY(follow_null_stream()); }
    try {
        auto [in0, logits] = layout_slabs();
        if (in0_user)
            SUO_HIP_CHECK(hipMemcpyAsync(in0, in0_user, (size_t)L * CROP * CROP * IN_C * sizeof(float), hipMemcpyDeviceToDevice, s));
        SUO_TRY(run_backbone(in0, IN_C, logits, L, s));
        if (logits_out)
            SUO_HIP_CHECK(hipMemcpyAsync(logits_out, logits, (size_t)L * NUM_KP * HEAT * HEAT * sizeof(float), hipMemcpyDeviceToDevice, s));
        SUO_TRY(commit_call(s));
    } catch (const std::exception& e) {
        suo_set_error("suo_net_backbone: %s", e.what());
        return SUO_ERR_ARG;
    }
    if (own) {
        SUO_HIP_CHECK(hipStreamSynchronize(s));
        if (own_call_invalid()) return forward_staged(in0_user, L, logits_out, nullptr);      // (now on the bf16 form: cannot recurse twice)
    }
    return SUO_OK;
}

int Net::forward(const void* img, int fmt, int H, int W, const float* boxes, const int* box_img, int L, const float* priors,
                 const float* prior_uv, const uint8_t* prior_mask, float* uv, float* cov,
                 float* kp_prob, float* kp_logit, float* logits_out, hipStream_t s) {
    if (L <= 0 || L > max_crops_) { suo_set_error("suo_net_forward: L=%d outside [1,%d]", L, max_crops_); return SUO_ERR_ARG; }
    const bool own = (s == nullptr);
    if (own) { s = own_stream_; SUO_TRY(follow_null_stream()); }   // the legacy NULL stream cannot be captured: run on an internal stream and block
    try {
        auto [in0, logits] = layout_slabs();
        const int in_c = (priors || prior_uv) ? IN_C : IMG_C;     // the slab is sized for IN_C; the prior-less layout uses a sixth of it
        if (in_c == IMG_C && fused_stem()) {
            // prior-less pass: RoIAlign + stem in one launch on the bf16 pipe (csrc/stem_x3.hip), ahead of the captured backbone (the frame and
            // the boxes are the caller's buffers: their addresses change from call to call, a captured launch could not take them)
            // fp16 form: also r1's conv1 on the tile while the stem has it, where the plan takes it (the stem's output is then read by r1's skip convolution only)
            const bool f16 = pipe_ == 2 && stem_x3_.w[2];
            const StemNext nx = {r1_.pro_scale, r1_.pro_shift, reinterpret_cast<const uint16_t*>(r1_.c1.w.w[2]), r1_.c1.w.osc, r1_.c1.bias, stem_mid1_slab_, r1_.c1.xs16};
            SUO_LAUNCH(launch_stem_x3(img, fmt, H, W, boxes, box_img, L, reinterpret_cast<const uint16_t*>(stem_x3_.w[f16 ? 2 : 1]), stem_x3_bias_, stem_slab_, s,
                                      f16 ? stem_x3_.osc : nullptr, f16 ? range_flag_ : nullptr, stem_computes_r1_conv1() ? &nx : nullptr));
            SUO_TRY(run_backbone(in0, in_c, logits, L, s, true));
        } else {
            SUO_LAUNCH(launch_roi_align_concat(img, fmt, H, W, boxes, box_img, L, in_c, priors, prior_uv, prior_mask, in0, s));
            SUO_TRY(run_backbone(in0, in_c, logits, L, s, false));
        }
        SUO_LAUNCH(launch_decode(logits, L, uv, cov, d_mean_logit_, nullptr, nullptr, s));
        SUO_LAUNCH(launch_classifier(d_mean_logit_, cls_w_, cls_b_, L, kp_logit, kp_prob, s));
        if (logits_out)
            SUO_HIP_CHECK(hipMemcpyAsync(logits_out, logits, (size_t)L * NUM_KP * HEAT * HEAT * sizeof(float), hipMemcpyDeviceToDevice, s));
        SUO_TRY(commit_call(s));
    } catch (const std::exception& e) {
        suo_set_error("suo_net_forward: %s", e.what());
        return SUO_ERR_ARG;
    }
    if (own) {
        SUO_HIP_CHECK(hipStreamSynchronize(s));
        if (own_call_invalid()) return forward(img, fmt, H, W, boxes, box_img, L, priors, prior_uv, prior_mask, uv, cov, kp_prob, kp_logit, logits_out, nullptr);
    }
    return SUO_OK;
}

}  // namespace suo
