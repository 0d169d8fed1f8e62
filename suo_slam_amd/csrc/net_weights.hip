// The keypoint CNN's weights: a state_dict with the reference's key names (backbone.* / classifier.2.*, see suo_slam_amd/weights.py) checked, BatchNorm-folded,
// packed for every matrix-pipe form the network is built for (PipeW, csrc/net.h) and uploaded; the fp16 form's activation sites.  csrc/net.hip runs them.
#include "net.h"
#include "f16x2.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include "tune.h"

namespace suo {

static constexpr float BN_EPS = 1e-5f;

// ------------------------------------------------------------------------------------------------
// weight lookup helpers
const HostTensor& Net::T(const std::string& name) const {
    auto it = tensors_.find(name);
    if (it == tensors_.end()) throw std::runtime_error("missing tensor: " + name);
    return it->second;
}

// A checkpoint tensor must have exactly the shape the architecture (lib/models/hg.py:61-93, layers/Residual.py:7-18)
// gives it: anything else would be read out of bounds or silently zero-padded.
static void expect_shape(const Net& net, const std::string& name, std::initializer_list<int64_t> dims) {
    const HostTensor& t = net.T(name);
    if (t.shape.size() == dims.size() && std::equal(dims.begin(), dims.end(), t.shape.begin())) return;
    std::string got, want;
    for (int64_t d : t.shape) got += (got.empty() ? "" : ",") + std::to_string(d);
    for (int64_t d : dims) want += (want.empty() ? "" : ",") + std::to_string(d);
    throw std::runtime_error("tensor " + name + " has shape [" + got + "], expected [" + want + "]");
}
static void expect_bn(const Net& net, const std::string& p, int64_t c) {
    for (const char* f : {".weight", ".bias", ".running_mean", ".running_var"}) expect_shape(net, p + f, {c});
}
static void expect_conv(const Net& net, const std::string& p, int64_t cout, int64_t cin, int64_t k) {
    expect_shape(net, p + ".weight", {cout, cin, k, k});
    expect_shape(net, p + ".bias", {cout});
}

// BN(eval) as y = x*scale + shift
static void bn_affine(const Net& net, const std::string& p, std::vector<float>& scale, std::vector<float>& shift) {
    const HostTensor& g = net.T(p + ".weight");
    const HostTensor& b = net.T(p + ".bias");
    const HostTensor& m = net.T(p + ".running_mean");
    const HostTensor& v = net.T(p + ".running_var");
    const size_t c = g.numel;
    scale.resize(c);
    shift.resize(c);
    for (size_t i = 0; i < c; ++i) {
        const float s = g.data[i] / sqrtf(v.data[i] + BN_EPS);
        scale[i] = s;
        shift[i] = b.data[i] - m.data[i] * s;
    }
}

// Pack W[n][k] (n < N, k < K; zero beyond) into the MFMA B-operand layouts.  `out` holds 2*Np*Kp floats:
//   [0, Np*Kp)        32x32x2 form  [Kp/8][Np/32][64][4]:  W[nb*32+(lane&31)][kb*8 +(lane>>5)*4+t]
//   [Np*Kp, 2*Np*Kp)  16x16x4 form  [Kp/16][Np/16][64][4]: W[nb*16+(lane&15)][kg*16+(lane>>4)*4+t]   (small-map kernels)
void pack_gemm_weight(const float* W, int N, int K, int ldw, int Np, int Kp, float* out) {
    {
        float* o16 = out + (size_t)Np * Kp;
        const int NB16 = Np / 16;
        for (int kg = 0; kg < Kp / 16; ++kg)
            for (int nb = 0; nb < NB16; ++nb)
                for (int lane = 0; lane < 64; ++lane)
                    for (int t = 0; t < 4; ++t) {
                        const int n = nb * 16 + (lane & 15), k = kg * 16 + (lane >> 4) * 4 + t;
                        o16[(((size_t)kg * NB16 + nb) * 64 + lane) * 4 + t] = (n < N && k < K) ? W[(size_t)n * ldw + k] : 0.f;
                    }
    }
    const int NB = Np / 32;
    for (int kb = 0; kb < Kp / 8; ++kb)
        for (int nb = 0; nb < NB; ++nb)
            for (int lane = 0; lane < 64; ++lane)
                for (int t = 0; t < 4; ++t) {
                    const int n = nb * 32 + (lane & 31), k = kb * 8 + (lane >> 5) * 4 + t;
                    out[(((size_t)kb * NB + nb) * 64 + lane) * 4 + t] = (n < N && k < K) ? W[(size_t)n * ldw + k] : 0.f;
                }
}

// Conv weight W[n][c][ky][kx] -> GEMM weight with K' = [chunk][ky][kx][kk] (kk < CK), then packed.
void pack_conv_weight(const float* W, int N, int C, int KS, int Np, int Cp, int CK, const float* out_scale, float* out) {
    const int nch = Cp / CK, Kraw = nch * KS * KS * CK, Kp = (Kraw + 15) / 16 * 16;
    std::vector<float> g((size_t)Np * Kp, 0.f);
    if (CK == 4) {
        // image-only stem (csrc/conv.hip, PAIR mode): dense K axis kk = tap * 3 + channel; MFMA k-step t of group kb multiplies
        // kk = 8 kb + 2 t (lanes 0-31) and 8 kb + 2 t + 1 (lanes 32-63), which pack_gemm_weight reads from column kb*8 + half*4 + t
        for (int n = 0; n < N; ++n)
            for (int kk = 0; kk < KS * KS * 3; ++kk) {
                const int tap = kk / 3, c = kk % 3;
                if (c >= C) continue;
                const int kb = kk / 8, r = kk % 8, t = r / 2, half = r % 2;
                const float s = out_scale ? out_scale[n] : 1.f;
                g[(size_t)n * Kp + kb * 8 + half * 4 + t] = W[(((size_t)n * C + c) * KS + tap / KS) * KS + tap % KS] * s;
            }
        pack_gemm_weight(g.data(), Np, Kp, Kp, Np, Kp, out);
        return;
    }
    for (int n = 0; n < N; ++n)
        for (int ch = 0; ch < nch; ++ch)
            for (int ky = 0; ky < KS; ++ky)
                for (int kx = 0; kx < KS; ++kx)
                    for (int kk = 0; kk < CK; ++kk) {
                        const int c = ch * CK + kk;
                        if (c >= C) continue;
                        const float s = out_scale ? out_scale[n] : 1.f;
                        g[(size_t)n * Kp + ((ch * KS + ky) * KS + kx) * CK + kk] = W[(((size_t)n * C + c) * KS + ky) * KS + kx] * s;
                    }
    pack_gemm_weight(g.data(), Np, Kp, Kp, Np, Kp, out);
}

float* Net::upload(const std::vector<float>& v) {
    float* d = nullptr;
    if (hipMalloc(&d, v.size() * sizeof(float)) != hipSuccess) throw std::runtime_error("hipMalloc(weights) failed");
    if (hipMemcpy(d, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        throw std::runtime_error("hipMemcpy(weights) failed");
    owned_.push_back(d);
    return d;
}

#ifndef SUO_WINO_BF16X3_DEFAULT
#define SUO_WINO_BF16X3_DEFAULT 1
#endif
static int round_up(int v, int m) { return (v + m - 1) / m * m; }

// SUO_WINO_BF16X3=0: the Residual blocks' 3x3 convolution + fused tail on the fp32 matrix pipe (csrc/conv_wino.hip) instead of the bf16 pipe
// with 3-way split operands (csrc/conv_wino_x3.hip: same accuracy, ~1.2x faster)
// (read when a network is built, not cached: one process can hold networks of both kinds)
static bool wino_bf16x3() {
    return env_switch("SUO_WINO_BF16X3", SUO_WINO_BF16X3_DEFAULT) != 0;
}
// SUO_F16X2=0: stay on the three-term bf16 form; default: the large launches run the two-term fp16 form (csrc/f16x2.h: half the MFMAs per product, range-guarded --
// a call that leaves fp16's range is reported by Net::range_exceeded and the network falls back to the bf16 form, whose planes are packed as well)
static bool pipe_f16x2() {
    return wino_bf16x3() && env_switch("SUO_F16X2", 1) != 0;
}

// The split-operand forms of one operator, the only place that decides which of them a network carries: three bf16 planes (pack3(src, planes); with_bf16 = false:
// an operator only the fp16 kernels compute) and, on a network built for the fp16 form, two fp16 planes + ncol per-column factors (pack2(src, planes, factors)).
// numel: elements of the packed operator -- the planes are uint16, 3 * numel and 2 * numel of them.
template <class Pack3, class Pack2>
void Net::fill_pipes(PipeW& pw, const float* src, size_t numel, int ncol, Pack3 pack3, Pack2 pack2, bool with_bf16) {
    if (!wino_bf16x3()) return;
    if (with_bf16) {
        std::vector<float> x3(3 * numel / 2);
        pack3(src, reinterpret_cast<uint16_t*>(x3.data()));
        pw.w[1] = upload(x3);
    }
    if (!pipe_f16x2()) return;
    std::vector<float> h2(numel), osc(ncol);
    pack2(src, reinterpret_cast<uint16_t*>(h2.data()), osc.data());
    pw.w[2] = upload(h2);
    pw.osc = upload(osc);
}

// 1x1 conv W[N][K] with optional per-output scale (BN folded), optionally a second K segment (conv2 on another operand) -> device packed weight + bias
void Net::make_gemm(const std::string& conv, const std::string& bn_after, const std::string& conv2, GemmW& g) {
    const HostTensor& w = T(conv + ".weight");
    const HostTensor& b = T(conv + ".bias");
    const int N = (int)w.shape[0], K1 = (int)w.shape[1];
    const int Np = round_up(N, 64), K1p = round_up(K1, 32);
    int K2 = 0, K2p = 0;
    if (!conv2.empty()) { K2 = (int)T(conv2 + ".weight").shape[1]; K2p = round_up(K2, 32); }
    std::vector<float> scale, shift;
    if (!bn_after.empty()) bn_affine(*this, bn_after, scale, shift);
    const int Kp = K1p + K2p;
    std::vector<float> full((size_t)Np * Kp, 0.f), bias(Np, 0.f);
    for (int n = 0; n < N; ++n) {
        const float s = scale.empty() ? 1.f : scale[n];
        for (int k = 0; k < K1; ++k) full[(size_t)n * Kp + k] = w.data[(size_t)n * K1 + k] * s;
        bias[n] = scale.empty() ? b.data[n] : b.data[n] * s + shift[n];
    }
    if (K2) {
        const HostTensor& w2 = T(conv2 + ".weight");
        const HostTensor& b2 = T(conv2 + ".bias");
        for (int n = 0; n < N; ++n) {
            for (int k = 0; k < K2; ++k) full[(size_t)n * Kp + K1p + k] = w2.data[(size_t)n * K2 + k];
            bias[n] += b2.data[n];
        }
    }
    pack_gemm(full, bias, N, K1, K2, g);
}

// full: [round_up(N, 64)][round_up(K1, 32) + round_up(K2, 32)], zero beyond N / K1 / K2; bias: [round_up(N, 64)]
void Net::pack_gemm(const std::vector<float>& full, const std::vector<float>& bias, int N, int K1, int K2, GemmW& g) {
    const int Np = round_up(N, 64), K1p = round_up(K1, 32), K2p = round_up(K2, 32), Kp = K1p + K2p;
    std::vector<float> packed(2 * (size_t)Np * Kp);
    pack_gemm_weight(full.data(), Np, Kp, Kp, Np, Kp, packed.data());
    g.w.w[0] = upload(packed);
    g.bias = upload(bias);
    g.N = Np; g.n_valid = N; g.K1 = K1p; g.K2 = K2p;
    // the same operator on the bf16 pipe at fp32 accuracy, and as two fp16 terms
    // (N = 64 -- conv1 of r1 / r4 -- stays on the persistent fp32-pipe kernel: these launches are HBM-streaming, 430 / 180 us there against 563 / 194
    //  in the bf16x3 kernel's 64-column tiles at 256 crops)
    const bool split = N % 128 == 0 && Np == N && K1 == K1p && K2 == K2p && K1 % 64 == 0 && K2 % 64 == 0 && K1 <= 512;
    // fp16 planes only: r1's conv1 (64 -> 64) for the stem launch that computes it on the tile (csrc/stem_x3.hip: NEXT), and the output head (tmpOut: 256 -> 41,
    // padded to 64 rows of zeros) for the lin + head launch (csrc/gemm_bf16x3.hip: gemm_chain_head_kernel)
    const bool f16_only = Np == 64 && K1 == K1p && K2 == 0 && ((N == 64 && K1 == 64) || K1 == 256);
    if (split || f16_only)
        fill_pipes(g.w, full.data(), (size_t)Np * Kp, Np, [&](const float* W, uint16_t* o) { pack_gemm_weight_bf16x3(W, Np, Kp, o); },
                   [&](const float* W, uint16_t* o, float* osc) { pack_gemm_weight_f16x2(W, Np, Kp, o, osc); }, split);
}

// c_used > 0: keep only the first c_used input channels of the filter (the others multiply structural zeros)
void Net::make_conv(const std::string& conv, const std::string& bn_after, int CK, ConvW& c, int c_used) {
    const HostTensor& w = T(conv + ".weight");
    const HostTensor& b = T(conv + ".bias");
    const int N = (int)w.shape[0], Cw = (int)w.shape[1], KS = (int)w.shape[2];
    const int C = c_used > 0 ? c_used : Cw;
    const int Np = round_up(N, 64), Cp = round_up(C, CK);
    std::vector<float> scale, shift;
    if (!bn_after.empty()) bn_affine(*this, bn_after, scale, shift);
    std::vector<float> packed(2 * (size_t)Np * ((Cp * KS * KS + 15) / 16 * 16)), bias(Np, 0.f);
    std::vector<float> sliced;
    const float* wdata = w.data;
    if (C != Cw) {
        sliced.resize((size_t)N * C * KS * KS);
        for (int n = 0; n < N; ++n)
            memcpy(&sliced[(size_t)n * C * KS * KS], w.data + (size_t)n * Cw * KS * KS, (size_t)C * KS * KS * sizeof(float));
        wdata = sliced.data();
    }
    const float* sc = scale.empty() ? nullptr : scale.data();
    pack_conv_weight(wdata, N, C, KS, Np, Cp, CK, sc, packed.data());
    for (int n = 0; n < N; ++n) bias[n] = scale.empty() ? b.data[n] : b.data[n] * scale[n] + shift[n];
    c.Wp = upload(packed);
    c.bias = upload(bias);
    c.N = Np; c.C = Cp; c.KS = KS;
    if (KS == 3 && N == C && (N == 128 || N == 64) && c_used <= 0) {       // the Residual blocks' 128 -> 128 / 64 -> 64 convolutions: also in Winograd form
        std::vector<float> wq((size_t)16 * N * C);
        pack_wino_weight(w.data, N, C, N, C, sc, wq.data());
        c.wino.w[0] = upload(wq);
        fill_pipes(c.wino, w.data, (size_t)16 * N * C, N, [&](const float* W, uint16_t* o) { pack_wino_weight_bf16x3(W, N, C, N, C, sc, o); },
                   [&](const float* W, uint16_t* o, float* osc) { pack_wino_weight_f16x2(W, N, C, N, C, sc, o, osc); });
    }
}

void Net::make_residual(const std::string& p, ResidualW& r) {
    {   // Residual(cin, cout): bn[cin] conv1[cout/2,cin,1] bn1 conv2[cout/2,cout/2,3] bn2 conv3[cout,cout/2,1] (+conv4[cout,cin,1] iff cin != cout)
        const int64_t cin = (int64_t)T(p + ".bn.weight").numel, cout = T(p + ".conv3.weight").shape.empty() ? 0 : T(p + ".conv3.weight").shape[0];
        const int64_t h = cout / 2;
        expect_bn(*this, p + ".bn", cin);
        expect_conv(*this, p + ".conv1", h, cin, 1);
        expect_bn(*this, p + ".bn1", h);
        expect_conv(*this, p + ".conv2", h, h, 3);
        expect_bn(*this, p + ".bn2", h);
        expect_conv(*this, p + ".conv3", cout, h, 1);
        if (tensors_.count(p + ".conv4.weight")) expect_conv(*this, p + ".conv4", cout, cin, 1);
        else if (cin != cout) throw std::runtime_error("residual " + p + ": " + std::to_string(cin) + " -> " + std::to_string(cout) + " channels needs conv4");
    }
    std::vector<float> sc, sh;
    bn_affine(*this, p + ".bn", sc, sh);
    r.cin = (int)sc.size();
    r.pro_scale = upload(sc);
    r.pro_shift = upload(sh);
    make_gemm(p + ".conv1", p + ".bn1", "", r.c1);
    make_conv(p + ".conv2", p + ".bn2", 32, r.c2);
    r.has_skip_conv = tensors_.count(p + ".conv4.weight") > 0;
    // conv3 (+ conv4 on the raw input as a second K segment: out = W3*mid + W4*x + b3 + b4)
    make_gemm(p + ".conv3", "", r.has_skip_conv ? p + ".conv4" : "", r.c3);
    r.cout = r.c3.n_valid;
    r.tail.w[0] = r.c3.w.w[0];
    const HostTensor& w3 = T(p + ".conv3.weight");
    const auto gemm3 = [](int N, int K) { return [=](const float* W, uint16_t* o) { pack_gemm_weight_bf16x3(W, N, K, o); }; };
    const auto gemm2 = [](int N, int K) { return [=](const float* W, uint16_t* o, float* osc) { pack_gemm_weight_f16x2(W, N, K, o, osc); }; };
    if (r.cin == 256 && r.cout == 256 && !r.has_skip_conv) {
        // the block in one launch (small maps): bn1 folded into W1's rows and bn2 into W2's exactly as make_gemm / make_conv fold them
        // (float products w * s), so the fp32 form is bit-identical to the per-layer launches
        const HostTensor& w1 = T(p + ".conv1.weight");
        const HostTensor& w2 = T(p + ".conv2.weight");
        std::vector<float> s1, t1, s2, t2;
        bn_affine(*this, p + ".bn1", s1, t1);
        bn_affine(*this, p + ".bn2", s2, t2);
        std::vector<float> w1f((size_t)128 * 256);
        for (int n = 0; n < 128; ++n)
            for (int k = 0; k < 256; ++k) w1f[(size_t)n * 256 + k] = w1.data[(size_t)n * 256 + k] * s1[n];
        std::vector<float> p1((size_t)128 * 256), p2((size_t)128 * 128 * 9), p3((size_t)256 * 128);
        pack_res16_gemm(w1f.data(), 128, 256, p1.data());
        pack_res16_conv3x3(w2.data, 128, 128, s2.data(), p2.data());
        pack_res16_gemm(w3.data, 256, 128, p3.data());
        r.block[0].w[0] = upload(p1); r.block[1].w[0] = upload(p2); r.block[2].w[0] = upload(p3);
        fill_pipes(r.block[0], w1f.data(), (size_t)128 * 256, 128, gemm3(128, 256), gemm2(128, 256));
        fill_pipes(r.block[1], w2.data, (size_t)128 * 128 * 9, 128, [&](const float* W, uint16_t* o) { pack_res_conv3x3_bf16x3(W, s2.data(), o); },
                   [&](const float* W, uint16_t* o, float* osc) { pack_res_conv3x3_f16x2(W, s2.data(), o, osc); });
        fill_pipes(r.block[2], w3.data, (size_t)256 * 128, 256, gemm3(256, 128), gemm2(256, 128));
    }
    if (r.c2.wino.w[1] && !r.has_skip_conv && w3.shape[0] == 256 && w3.shape[1] == 128)
        fill_pipes(r.tail, w3.data, (size_t)256 * 128, 256, [](const float* W, uint16_t* o) { pack_tail_weight_bf16x3(W, 256, 128, o); },
                   [](const float* W, uint16_t* o, float* osc) { pack_tail_weight_f16x2(W, 256, 128, o, osc); });
    register_residual_sites(p, r);
}

// ------------------------------------------------------------------------------------------------
// fp16 activation sites (csrc/f16x2.h): one per convolution with fp16 planes, whichever kernel computes it.  Its factor 2^s lives at site_xs_[i], which every
// fp16 launch splitting that operand reads; the per-channel factors 2^-(t_n + s) of the convolution's epilogues are kept at s = S2_XSHIFT on the host as well,
// so a new s rewrites them in place (no pointer changes: captured graphs stay valid).
int Net::add_site(const std::string& name, int ksize) {
    if ((int)sites_.size() >= kMaxSites) throw std::runtime_error("too many fp16 activation sites");
    Site st;
    st.name = name; st.ksize = ksize; st.shift = S2_XSHIFT;
    sites_.push_back(st);
    return (int)sites_.size() - 1;
}
void Net::site_osc(int site, float* dev, int n) {
    if (!dev) return;
    std::vector<float> h(n);
    if (hipMemcpy(h.data(), dev, (size_t)n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("hipMemcpy(factors) failed");
    sites_[site].osc.emplace_back(dev, std::move(h));
}
void Net::register_gemm_site(const std::string& p, GemmW& g) {
    if (!g.w.w[2]) return;
    g.site = add_site(p, 1);
    g.xs16 = site_xs_ + g.site;
    site_osc(g.site, g.w.osc, g.N);
}
void Net::register_residual_sites(const std::string& p, ResidualW& r) {
    if (r.c1.w.w[2] || r.block[0].w[2]) {                           // relu(bn(x)): the GEMM's prologue, the one-launch block's staging, the stem's / a fused tail's NEXT
        r.c1.site = add_site(p + ".conv1", 1);
        r.c1.xs16 = site_xs_ + r.c1.site;
        site_osc(r.c1.site, r.c1.w.osc, r.c1.N);
        site_osc(r.c1.site, r.block[0].osc, 128);
    }
    if (r.c2.wino.w[2] || r.block[1].w[2]) {                          // conv1's output: the Winograd staging, the one-launch block's conv1 epilogue
        r.c2.site = add_site(p + ".conv2", 3);
        r.c2.xs16 = site_xs_ + r.c2.site;
        site_osc(r.c2.site, r.c2.wino.osc, r.c2.N);
        site_osc(r.c2.site, r.block[1].osc, 128);
    }
    if (r.c3.w.w[2] || r.tail.w[2] || r.block[2].w[2]) {                // conv2's output (+ the block input of a skip conv4): the GEMM, the fused tail, the one-launch block
        r.c3.site = add_site(p + ".conv3", 1);
        r.c3.xs16 = site_xs_ + r.c3.site;
        site_osc(r.c3.site, r.c3.w.osc, r.c3.N);
        site_osc(r.c3.site, r.tail.osc, 256);
        site_osc(r.c3.site, r.block[2].osc, 256);
    }
}

void Net::make_hourglass(const std::string& p, int n, HourglassW& h) {
    h.n = n;
    auto check256 = [&](const ResidualW& r, const std::string& name) {
        if (r.cin != 256 || r.cout != 256) throw std::runtime_error("residual " + name + " must be 256 -> 256 channels");
    };
    for (int j = 0; j < 2; ++j) {
        make_residual(p + ".up1_." + std::to_string(j), h.up1[j]);
        make_residual(p + ".low1_." + std::to_string(j), h.low1[j]);
        make_residual(p + ".low3_." + std::to_string(j), h.low3[j]);
        check256(h.up1[j], p + ".up1_"); check256(h.low1[j], p + ".low1_"); check256(h.low3[j], p + ".low3_");
    }
    if (n > 1) {
        h.inner.reset(new HourglassW());
        make_hourglass(p + ".low2", n - 1, *h.inner);
    } else {
        for (int j = 0; j < 2; ++j) make_residual(p + ".low2_." + std::to_string(j), h.low2[j]);
    }
}

// ------------------------------------------------------------------------------------------------
// The weight half of the constructor: every tensor checked against the architecture, then stem, blocks, heads, the re-injection fold and the classifier, with the
// fp16 sites registered in this order (it is visible: suo_net_f16x2_site_name).  Host pointers are not retained past it.
void Net::build_weights(int n, const char* const* names, const float* const* data, const int64_t* const* shapes, const int* ndims) {
    for (int i = 0; i < n; ++i) {
        HostTensor t;
        t.data = data[i];
        t.numel = 1;
        for (int d = 0; d < ndims[i]; ++d) { t.shape.push_back(shapes[i][d]); t.numel *= (size_t)shapes[i][d]; }
        tensors_[names[i]] = t;
    }
    const std::string b = "backbone";
    auto expect_io = [&](const std::string& p, int cin, int cout) {
        expect_shape(*this, p + ".bn.weight", {cin});
        expect_shape(*this, p + ".conv3.bias", {cout});
    };
    expect_conv(*this, b + ".conv1_", 64, 3 + NUM_KP, 7);
    expect_bn(*this, b + ".bn1", 64);
    expect_io(b + ".r1", 64, 128);
    expect_io(b + ".r4", 128, 128);
    expect_io(b + ".r5", 128, 256);
    for (int i = 0; i < 2; ++i) {
        const std::string si = std::to_string(i);
        expect_conv(*this, b + ".lin_." + si + ".0", 256, 256, 1);
        expect_bn(*this, b + ".lin_." + si + ".1", 256);
        expect_conv(*this, b + ".tmpOut." + si, NUM_KP, 256, 1);
    }
    expect_conv(*this, b + ".ll_.0", 256, 256, 1);
    expect_conv(*this, b + ".tmpOut_.0", 256, NUM_KP, 1);
    expect_shape(*this, "classifier.2.weight", {NUM_KP, NUM_KP});
    expect_shape(*this, "classifier.2.bias", {NUM_KP});
    site_xs_ = upload(std::vector<float>(kMaxSites, S2_XSCALE));
    probe_max_ = reinterpret_cast<unsigned*>(upload(std::vector<float>(kMaxSites, 0.f)));
    make_conv(b + ".conv1_", b + ".bn1", 16, stem_);
    // Without priors (every single-view pass and the first SLAM pass, lib/object_slam.py:1094-1097) the 41 prior
    // channels are zeros: multiply only the 3 image channels.  Same taps, same order, so the result is bit-identical
    // to feeding zero priors through the full filter; 13 % of the network's MACs (41/44 of the stem) are never issued.
    make_conv(b + ".conv1_", b + ".bn1", IMG_C, stem_img_, 3);
    {   // ... and for the fused RoIAlign + stem launch on the split-operand pipes (csrc/stem_x3.hip)
        const HostTensor& w = T(b + ".conv1_.weight");
        const HostTensor& bb = T(b + ".conv1_.bias");
        const int Cw = (int)w.shape[1];
        std::vector<float> sc, sh, bias(64);
        bn_affine(*this, b + ".bn1", sc, sh);
        fill_pipes(stem_x3_, w.data, (size_t)14 * 2 * 64 * 8, 64, [&](const float* W, uint16_t* o) { pack_stem_weight_bf16x3(W, Cw, sc.data(), o); },
                   [&](const float* W, uint16_t* o, float* osc) { pack_stem_weight_f16x2(W, Cw, sc.data(), o, osc); });
        for (int n = 0; n < 64; ++n) bias[n] = bb.data[n] * sc[n] + sh[n];
        if (stem_x3_.w[1]) stem_x3_bias_ = upload(bias);
    }
    make_residual(b + ".r1", r1_);
    make_residual(b + ".r4", r4_);
    make_residual(b + ".r5", r5_);
    for (int i = 0; i < 2; ++i) {
        make_hourglass(b + ".hourglass." + std::to_string(i), 4, hg_[i]);
        for (int j = 0; j < 2; ++j) make_residual(b + ".Residual." + std::to_string(i * 2 + j), post_[i][j]);
        make_gemm(b + ".lin_." + std::to_string(i) + ".0", b + ".lin_." + std::to_string(i) + ".1", "", lin_[i]);
        make_gemm(b + ".tmpOut." + std::to_string(i), "", "", head_[i]);
        register_gemm_site(b + ".lin_." + std::to_string(i) + ".0", lin_[i]);
        register_gemm_site(b + ".tmpOut." + std::to_string(i), head_[i]);
    }
    // inter-stack re-injection (hg.py:112-117): x + ll_(ll) + tmpOut_(tmpOut(ll)).  tmpOut and tmpOut_ are both plain 1x1
    // convolutions with nothing between them, so the sum is ONE 256 -> 256 GEMM on ll with
    //     W' = W_ll + W_tmpOut_ W_tmpOut ,   b' = b_ll + b_tmpOut_ + W_tmpOut_ b_tmpOut      (folded here in fp64, rounded once)
    // + the residual x: the 41-channel stack-0 heat-maps -- which nothing else reads (only the last stack is returned,
    // pkpnet.py:103-105) -- are never materialised and the 64 extra K columns of the dual-operand form are not multiplied.
    {
        const HostTensor& wl = T(b + ".ll_.0.weight");   const HostTensor& bl = T(b + ".ll_.0.bias");
        const HostTensor& wt_ = T(b + ".tmpOut_.0.weight"); const HostTensor& bt_ = T(b + ".tmpOut_.0.bias");
        const HostTensor& wh = T(b + ".tmpOut.0.weight");  const HostTensor& bh = T(b + ".tmpOut.0.bias");
        const int N = (int)wl.shape[0], K = (int)wl.shape[1], J = (int)wh.shape[0];      // 256, 256, 41
        if ((int)wt_.shape[0] != N || (int)wt_.shape[1] != J || (int)wh.shape[1] != K) throw std::runtime_error("re-injection convolutions have unexpected shapes");
        std::vector<float> full((size_t)N * K), bias(N);
        for (int n = 0; n < N; ++n) {
            double bb = (double)bl.data[n] + (double)bt_.data[n];
            for (int j = 0; j < J; ++j) bb += (double)wt_.data[(size_t)n * J + j] * (double)bh.data[j];
            bias[n] = (float)bb;
            for (int k = 0; k < K; ++k) {
                double v = wl.data[(size_t)n * K + k];
                for (int j = 0; j < J; ++j) v += (double)wt_.data[(size_t)n * J + j] * (double)wh.data[(size_t)j * K + k];
                full[(size_t)n * K + k] = (float)v;
            }
        }
        pack_gemm(full, bias, N, K, 0, reinject_);
        register_gemm_site(b + ".ll_.0", reinject_);          // (ll_ + tmpOut_ tmpOut folded: one operand, ll)
    }
    {
        const HostTensor& w = T("classifier.2.weight");
        const HostTensor& bb = T("classifier.2.bias");
        cls_w_ = upload(std::vector<float>(w.data, w.data + w.numel));
        cls_b_ = upload(std::vector<float>(bb.data, bb.data + bb.numel));
    }
    tensors_.clear();   // host pointers are not retained past construction
    pipe_built_ = pipe_f16x2() ? 2 : (wino_bf16x3() ? 1 : 0);
    pipe_ = pipe_built_;
}

}  // namespace suo
