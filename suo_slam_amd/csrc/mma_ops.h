// The matrix-pipe idioms the CNN kernels share, each defined once: operand / accumulator vector types, the cross terms of a split product
// (csrc/bf16x3.h, csrc/f16x2.h), the split of four fp32 values into operand planes, the accumulator's row layout and its transposition patch,
// and the XCD-aware workgroup order.  Several contracts rest on the kernels agreeing here bit for bit (the fused tails' NEXT conv1, the chain
// head's y1 and the fused stem's conv1 equal the separate GEMM launch): same term order, same rounding chain.  No host state; device code only.
#pragma once
#include "bf16x3.h"
#include "f16x2.h"

namespace suo {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// fp32 pipe: one k-pair of a 32 x 32 block
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// ---- split product: NP = 3 bf16 terms per operand (six cross terms i + j <= 2) or NP = 2 fp16 terms (hi lo, lo hi, hi hi), smallest first ----
template <int NP>
constexpr int split_terms() { return NP == 3 ? 6 : 3; }

// term t of a (32 x 16, planes as 16-byte A fragments; fp16 planes travel under the bf16 type) times b (16 x 32, planes as loaded) onto acc
template <int NP>
__device__ __forceinline__ f32x16 split_mma(int t, const bf16x8 (&a)[NP], const u32x4 (&b)[NP], f32x16 acc) {
    static_assert(NP == 2 || NP == 3, "operand planes");
    constexpr int TI[6] = {0, 1, 2, 0, 1, 0}, TJ[6] = {2, 1, 0, 1, 0, 0};
    constexpr int UI[3] = {0, 1, 0}, UJ[3] = {1, 0, 0};
    if constexpr (NP == 3) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[TI[t]], __builtin_bit_cast(bf16x8, b[TJ[t]]), acc, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a[UI[t]]), __builtin_bit_cast(f16x8, b[UJ[t]]), acc, 0, 0, 0);
}

// ---- plane split: x0 .. x3 -> NP planes of four 16-bit terms (8 bytes each) at base + p * STRIDE, STRIDE in elements of E.
// NP = 3: round-to-nearest bf16 of the value and of its two exact residuals (the last conversion is exact); NP = 2: hi = rn16(x), lo = rn16(x - hi),
// the residual exact.  The caller scales and tracks the range guard's maximum before it calls.  (STRIDE a template argument and no loop in here: with
// either, the kernels' code differed from the hand-written form.)
template <int NP, int STRIDE, typename E>
__device__ __forceinline__ void split_store4(E* base, float x0, float x1, float x2, float x3) {
    static_assert(NP == 2 || NP == 3, "operand planes");
    if constexpr (NP == 3) {
        const unsigned a0 = s3_pack_rn(x0, x1), a1 = s3_pack_rn(x2, x3);
        *(u32x2*)base = u32x2{a0, a1};
        x0 -= s3_lo(a0); x1 -= s3_hi(a0); x2 -= s3_lo(a1); x3 -= s3_hi(a1);
        const unsigned b0 = s3_pack_rn(x0, x1), b1 = s3_pack_rn(x2, x3);
        *(u32x2*)(base + STRIDE) = u32x2{b0, b1};
        x0 -= s3_lo(b0); x1 -= s3_hi(b0); x2 -= s3_lo(b1); x3 -= s3_hi(b1);
        *(u32x2*)(base + 2 * STRIDE) = u32x2{s3_pack_rn(x0, x1), s3_pack_rn(x2, x3)};
    } else {
        const unsigned h0 = s2_pack_rn(x0, x1), h1 = s2_pack_rn(x2, x3);
        *(u32x2*)base = u32x2{h0, h1};
        const unsigned l0 = s2_lo_pack(x0, x1, h0), l1 = s2_lo_pack(x2, x3, h1);
        *(u32x2*)(base + STRIDE) = u32x2{l0, l1};
    }
}

// ---- accumulator of a 32 x 32 MFMA: register r of a lane holds row acc_row(r, lane), column lane & 31 ----
__device__ __forceinline__ int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// transposition through a wave-private patch T[32][PITCH]: register r goes to T[patch_at(r, lane)]; after a wave barrier the lane reads rows (lane >> 3) + 8 k,
// k = 0 .. 3, four columns at 4 (lane & 7).  (The store loop stays with the caller: inside a helper it changed the code of every kernel that used it.)
template <int PITCH = 36>
__device__ __forceinline__ int patch_at(int r, int lane) { return acc_row(r, lane) * PITCH + (lane & 31); }
template <int PITCH = 36>
__device__ __forceinline__ f32x4 patch_row4_at(const float* T, int row, int lane) { return *(const f32x4*)&T[row * PITCH + (lane & 7) * 4]; }      // row = (lane >> 3) + 8 k, where the caller holds it
template <int PITCH = 36>
__device__ __forceinline__ f32x4 patch_row4(const float* T, int lane, int k) { return patch_row4_at<PITCH>(T, (lane >> 3) + 8 * k, lane); }

// ---- workgroup order: consecutive ids land on the eight XCDs round-robin; give each XCD a contiguous run of tiles (shared L2) ----
__device__ __forceinline__ int xcd_block_id() {
    int bid = blockIdx.x;
    if ((gridDim.x & 7) == 0) bid = (bid & 7) * (gridDim.x >> 3) + (bid >> 3);
    return bid;
}

}  // namespace suo
