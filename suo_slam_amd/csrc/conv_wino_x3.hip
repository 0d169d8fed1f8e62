// The split-operand Winograd 3x3 convolution (kernel and its story: csrc/conv_wino_x3_kernel.h): the host-side weight packers, the two launch
// predicates and the launchers of the register-staged forms.  The LDS-DMA forms are instantiated in csrc/conv_wino_x3_dma.hip.
#include <stdlib.h>

#include "conv_wino_x3_kernel.h"

namespace suo {

// host: U[n][c][comp] = wino_weight_transform of filter (n, c) (csrc/conv_wino.hip: fp64, BN scale folded in, rounded once to fp32, row xi = 3 negated),
// split into three bf16 terms (csrc/bf16x3.h);
//   Up3[chunk][comp][nb][plane][lane][e] = term `plane` of U[nb*32 + (lane&31)][chunk*16 + 8*(lane>>5) + e][comp]     (B operand of
//   v_mfma_f32_32x32x16_bf16: lane l supplies k = 8 (l >> 5) .. + 7 of column l & 31)
void pack_wino_weight_bf16x3(const float* W, int N, int C, int Np, int Cp, const float* out_scale, uint16_t* out) {
    const int NB = Np / 32;
    memset(out, 0, (size_t)Np * Cp * 16 * 3 * sizeof(uint16_t));
    for (int n = 0; n < N; ++n)
        for (int c = 0; c < C; ++c) {
            float U[16];
            wino_weight_transform(W + ((size_t)n * C + c) * 9, out_scale ? (double)out_scale[n] : 1.0, U);
            const int chunk = c / X_CK, cc = c % X_CK, nb = n / 32, lane = (cc / 8) * 32 + (n % 32), e = cc % 8;
            for (int comp = 0; comp < 16; ++comp) {
                uint16_t t[3];
                s3_split_host(U[comp], t);
                for (int p = 0; p < 3; ++p) out[((((size_t)(chunk * 16 + comp) * NB + nb) * 3 + p) * 64 + lane) * 8 + e] = t[p];
            }
        }
}

// host: conv3 weight W3[N2][K] (1x1) -> three bf16 terms (csrc/bf16x3.h) in B-operand order of v_mfma_f32_32x32x16_bf16:
//   W3x[(ks * NB + nb) * 3 + plane][lane][e] = term `plane` of W3[nb*32 + (lane&31)][ks*16 + 8*(lane>>5) + e]
void pack_tail_weight_bf16x3(const float* W3, int N2, int K, uint16_t* out) {
    const int NB = N2 / 32;
    for (int n = 0; n < N2; ++n)
        for (int k = 0; k < K; ++k) {
            const int ks = k / 16, kk = k % 16, lane = (kk / 8) * 32 + (n % 32), e = kk % 8, nb = n / 32;
            uint16_t t[3];
            s3_split_host(W3[(size_t)n * K + k], t);
            for (int p = 0; p < 3; ++p) out[((((size_t)(ks * NB + nb) * 3 + p) * 64 + lane) * 8) + e] = t[p];
        }
}

// host, two-term fp16 form (csrc/f16x2.h): the same U in the same layout with two planes, every output channel n times 2^t_n (max over its C x 16 entries
// in [2^12, 2^13)); oscale_out[n] = 2^-(t_n + S2_XSHIFT) for the kernel's epilogue
void pack_wino_weight_f16x2(const float* W, int N, int C, int Np, int Cp, const float* out_scale, uint16_t* out, float* oscale_out) {
    const int NB = Np / 32;
    memset(out, 0, (size_t)Np * Cp * 16 * 2 * sizeof(uint16_t));
    for (int n = 0; n < Np; ++n) oscale_out[n] = ldexpf(1.f, -S2_XSHIFT);
    float* Un = (float*)malloc((size_t)C * 16 * sizeof(float));
    for (int n = 0; n < N; ++n) {
        float mx = 0.f;
        for (int c = 0; c < C; ++c) {
            wino_weight_transform(W + ((size_t)n * C + c) * 9, out_scale ? (double)out_scale[n] : 1.0, Un + c * 16);
            for (int comp = 0; comp < 16; ++comp) mx = fmaxf(mx, fabsf(Un[c * 16 + comp]));
        }
        const int t = s2_row_shift(mx);
        oscale_out[n] = ldexpf(1.f, -(t + S2_XSHIFT));
        for (int c = 0; c < C; ++c) {
            const int chunk = c / X_CK, cc = c % X_CK, nb = n / 32, lane = (cc / 8) * 32 + (n % 32), e = cc % 8;
            for (int comp = 0; comp < 16; ++comp) {
                uint16_t h[2];
                s2_split_host(ldexpf(Un[c * 16 + comp], t), h);
                for (int p = 0; p < 2; ++p) out[((((size_t)(chunk * 16 + comp) * NB + nb) * 2 + p) * 64 + lane) * 8 + e] = h[p];
            }
        }
    }
    free(Un);
}

// host: conv3 weight of the fused tail, two fp16 planes: the layout of pack_gemm_weight_f16x2 (csrc/gemm_bf16x3.hip)
void pack_tail_weight_f16x2(const float* W3, int N2, int K, uint16_t* out, float* oscale_out) { pack_gemm_weight_f16x2(W3, N2, K, out, oscale_out); }

// Launches of at most one workgroup per CU (<= 256 tiles: a one-frame call, a SLAM pass) take the eight-wave form of the fp16 kernel (W8): there the
// workgroup's latency IS the launch's duration.  SUO_WINO_W8=0 (supported switch, include/suo_hip.h; read when a launch is issued -- a network's captured
// graph keeps the form it was captured with, whatever the variable says at a replay): the four-wave form everywhere (A/B);
// SUO_WINO_W8_TILES (tuning builds): largest such launch.
bool conv3x3_wino_f16x2_w8(long tiles) {
    static const long upto = SUO_TUNE("SUO_WINO_W8_TILES", 256);
    return tiles > 0 && tiles <= upto && env_switch("SUO_WINO_W8", 1) != 0;
}

// The four-wave fp16 kernels stage their halo by LDS-DMA (the kernel's comment: DMA).  SUO_WINO_HALO_DMA=0 (supported switch, include/suo_hip.h; read when a launch is
// issued, like SUO_WINO_W8 -- a network's captured graph keeps the path it was captured with): the register-staged path (A/B, tests/test_gpu_wino_halo_dma.py: the two
// paths agree bit for bit).  The DMA kernels and their launchers (arguments checked here): csrc/conv_wino_x3_dma.hip.
bool conv3x3_wino_f16x2_dma() { return env_switch("SUO_WINO_HALO_DMA", 1) != 0; }
int launch_conv3x3_wino_f16x2_dma(const ConvArgs& a, hipStream_t s, int tiles);          // 64 -> 64 or 128 -> 128 by a.N
int launch_conv3x3_wino_f16x2_fused_dma(const ConvArgs& a, hipStream_t s, int tiles);    // with / without a.up, a.n_W1
// The LDS-DMA form's tail with the up-sampled addend fetches its skip rows by LDS-DMA as well, a block of the epilogue ahead (the kernel's comment: SKD).
// SUO_WINO_SKIP_DMA=0 (supported switch, include/suo_hip.h; read when a launch is issued, like SUO_WINO_HALO_DMA): the register loads (A/B,
// tests/test_gpu_wino_skip_dma.py: bit for bit the same).  The other tails have no such form (profiles/REJECTED.md); with SUO_WINO_HALO_DMA=0 none has.
// Kernel and launcher: csrc/conv_wino_x3_skip_dma.hip.
bool conv3x3_wino_f16x2_skip_dma() { return env_switch("SUO_WINO_SKIP_DMA", 1) != 0; }
int launch_conv3x3_wino_f16x2_fused_up_skip_dma(const ConvArgs& a, hipStream_t s, int tiles);
// The LDS-DMA form's tail with the next block's conv1 runs its 1x1 stages in ONE pass over the 128-pixel tile (the kernel's comment: ONEP): W3 and the next W1
// are streamed once per tile, not once per 64-pixel pass.  SUO_WINO_TAIL_ONE_PASS=0 (supported switch, include/suo_hip.h; read when a launch is issued, like
// SUO_WINO_HALO_DMA): the two passes (A/B, tests/test_gpu_wino_tail_one_pass.py: bit for bit the same).  The other tails have no such form
// (profiles/REJECTED.md); with SUO_WINO_HALO_DMA=0 none has.  Kernel and launcher: csrc/conv_wino_x3_one_pass.hip.
bool conv3x3_wino_f16x2_tail_one_pass() { return env_switch("SUO_WINO_TAIL_ONE_PASS", 1) != 0; }
int launch_conv3x3_wino_f16x2_fused_next_one_pass(const ConvArgs& a, hipStream_t s, int tiles);

// a.Wp = weights packed by pack_wino_weight_bf16x3 / _f16x2 (uint16 under a float pointer); 128 -> 128 or 64 -> 64 channels
template <int NP>
static int launch_wino_split(const ConvArgs& a, hipStream_t s) {
    if (NP == 2 && (!a.oscale || !a.range_flag)) { suo_set_error("conv3x3_wino_f16x2: oscale / range_flag missing"); return SUO_ERR_ARG; }
    if (a.OH == a.H && a.OW == a.W && a.N == 64 && a.C == 64) {
        const int tiles64 = ((a.OW + X_TW - 1) / X_TW) * ((a.OH + X_TH - 1) / X_TH) * a.L;
        if (NP == 2 && conv3x3_wino_f16x2_dma()) return launch_conv3x3_wino_f16x2_dma(a, s, tiles64);
        hipLaunchKernelGGL((wino3x3_x3_kernel<false, false, false, 2, NP>), dim3(tiles64), dim3(256), 0, s, a);
        SUO_HIP_CHECK(hipGetLastError());
        return SUO_OK;
    }
    if (a.OH != a.H || a.OW != a.W || a.N != 128 || a.C != 128) {
        suo_set_error("conv3x3_wino_x3: unsupported shape H=%d W=%d C=%d N=%d", a.H, a.W, a.C, a.N);
        return SUO_ERR_ARG;
    }
    const int tiles = ((a.OW + X_TW - 1) / X_TW) * ((a.OH + X_TH - 1) / X_TH) * a.L;
    if (NP == 2 && conv3x3_wino_f16x2_w8(tiles)) hipLaunchKernelGGL((wino3x3_x3_kernel<false, false, false, 4, 2, false, false, true>), dim3(tiles), dim3(512), 0, s, a);
    else if (NP == 2 && conv3x3_wino_f16x2_dma()) return launch_conv3x3_wino_f16x2_dma(a, s, tiles);
    else hipLaunchKernelGGL((wino3x3_x3_kernel<false, false, false, 4, NP>), dim3(tiles), dim3(256), 0, s, a);
    SUO_HIP_CHECK(hipGetLastError());
    return SUO_OK;
}
int launch_conv3x3_wino_x3(const ConvArgs& a, hipStream_t s) { return launch_wino_split<3>(a, s); }
int launch_conv3x3_wino_f16x2(const ConvArgs& a, hipStream_t s) { return launch_wino_split<2>(a, s); }

// the fused Residual tail on two fp16 planes: a.Wp = pack_wino_weight_f16x2, a.W3p = pack_tail_weight_f16x2, a.oscale / a.oscale3 their factors
int launch_conv3x3_wino_f16x2_fused(const ConvArgs& a, hipStream_t s) {
    if (a.OH != a.H || a.OW != a.W || a.N != 128 || a.C != 128 || a.N2 != 256 || !a.W3p || !a.bias3 || !a.R || !a.out2 || !a.oscale || !a.oscale3 || !a.range_flag) {
        suo_set_error("conv3x3_wino_f16x2_fused: unsupported shape C=%d N=%d N2=%d", a.C, a.N, a.N2);
        return SUO_ERR_ARG;
    }
    const int tiles = ((a.OW + X_TW - 1) / X_TW) * ((a.OH + X_TH - 1) / X_TH) * a.L;
    const bool dma = conv3x3_wino_f16x2_dma();
    if (a.n_W1) {                                      // ... with the next block's conv1 on the tile (all of n_* set)
        if (!a.n_scale || !a.n_shift || !a.n_osc1 || !a.n_b1 || !a.n_out) { suo_set_error("conv3x3_wino_f16x2_fused: incomplete next-block arguments"); return SUO_ERR_ARG; }
        // (with an up-sampled addend the kernel would need 14-23 registers more than the 256 a two-workgroup-per-CU kernel has: it spilled and measured
        //  SLOWER than the two launches, profiles/REJECTED.md -- not built; csrc/net.hip does not ask for it)
        if (a.up) { suo_set_error("conv3x3_wino_f16x2_fused: the next block's conv1 cannot ride on a tail with an up-sampled addend"); return SUO_ERR_ARG; }
        if (dma) return conv3x3_wino_f16x2_tail_one_pass() ? launch_conv3x3_wino_f16x2_fused_next_one_pass(a, s, tiles) : launch_conv3x3_wino_f16x2_fused_dma(a, s, tiles);
        hipLaunchKernelGGL((wino3x3_x3_kernel<true, false, true, 4, 2, true>), dim3(tiles), dim3(256), 0, s, a);
    } else if (conv3x3_wino_f16x2_w8(tiles)) {
        if (a.up) hipLaunchKernelGGL((wino3x3_x3_kernel<true, true, true, 4, 2, false, false, true>), dim3(tiles), dim3(512), 0, s, a);
        else hipLaunchKernelGGL((wino3x3_x3_kernel<true, false, true, 4, 2, false, false, true>), dim3(tiles), dim3(512), 0, s, a);
    } else if (dma) return a.up && conv3x3_wino_f16x2_skip_dma() ? launch_conv3x3_wino_f16x2_fused_up_skip_dma(a, s, tiles) : launch_conv3x3_wino_f16x2_fused_dma(a, s, tiles);
    else if (a.up) hipLaunchKernelGGL((wino3x3_x3_kernel<true, true, true, 4, 2>), dim3(tiles), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((wino3x3_x3_kernel<true, false, true, 4, 2>), dim3(tiles), dim3(256), 0, s, a);
    SUO_HIP_CHECK(hipGetLastError());
    return SUO_OK;
}

int launch_conv3x3_wino_x3_fused(const ConvArgs& a, hipStream_t s) {
    if (a.OH != a.H || a.OW != a.W || a.N != 128 || a.C != 128 || a.N2 != 256 || !a.W3p || !a.bias3 || !a.R || !a.out2) {
        suo_set_error("conv3x3_wino_x3_fused: unsupported shape C=%d N=%d N2=%d", a.C, a.N, a.N2);
        return SUO_ERR_ARG;
    }
    const int tiles = ((a.OW + X_TW - 1) / X_TW) * ((a.OH + X_TH - 1) / X_TH) * a.L;
    if (a.w3_bf16x3) {                                 // W3p packed by pack_tail_weight_bf16x3: the tail on the bf16 pipe too
        if (a.up) hipLaunchKernelGGL((wino3x3_x3_kernel<true, true, true>), dim3(tiles), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((wino3x3_x3_kernel<true, false, true>), dim3(tiles), dim3(256), 0, s, a);
    } else {
        if (a.up) hipLaunchKernelGGL((wino3x3_x3_kernel<true, true, false>), dim3(tiles), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((wino3x3_x3_kernel<true, false, false>), dim3(tiles), dim3(256), 0, s, a);
    }
    SUO_HIP_CHECK(hipGetLastError());
    return SUO_OK;
}

}  // namespace suo
