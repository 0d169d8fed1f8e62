// The Winograd F(2x2,3x3) convolution of csrc/conv_wino.hip with its element-wise products on the BF16 matrix pipe at fp32 accuracy (3-way
// operand split, 6 of 9 cross terms, fp32 accumulate: see csrc/gemm_bf16x3.hip for the arithmetic) -- what the network launches for the
// Residual blocks' 3x3 convolutions and fused tails (csrc/net.hip; SUO_WINO_BF16X3=0 keeps the fp32-pipe kernels).
//
//   Y = A^T [ sum_c (G g_c G^T) (.) (B^T d_c B) ] A
// Per 16-channel chunk and Winograd component the product V_xi,nu (32 tiles x 16 channels) * U_xi,nu (16 channels x 32 outputs) is
// EIGHT v_mfma_f32_32x32x2_f32 (8 x 64 = 512 pipe cycles) in the fp32 kernel and SIX v_mfma_f32_32x32x16_bf16 (6 x 32 = 192 cycles)
// here: U is split on the host (fp64 transform, rounded once to fp32, then three round-to-nearest bf16 terms: csrc/bf16x3.h), V = B^T d B is computed in fp32
// exactly as before and split by the transforming thread on its way to LDS (three bf16 planes, 49 KB).  Same workgroup tile (8 x 16
// output pixels = 32 Winograd tiles x 128 output channels, 4 waves, wave w owns output channels [32 w, 32 w + 32)), same halo
// staging, same two-step output transform (rows xi = 0, 3 accumulate straight into Z, rows 1, 2 through a scratch accumulator and 16
// vector additions per chunk), same epilogues -- the accumulator layout of the bf16 MFMA is that of the fp32 one, so the fused
// Residual tail (conv3 1x1 + skip [+ up-sampled addend]) could be taken over unchanged (TX3 = false: conv3 on the fp32 pipe); the network uses
// TX3 = true, conv3 on the bf16 pipe as well (two passes of 64 pixels: see the tail's comment).
//
// The split product, the plane split (NP = 2), the accumulator's row and the workgroup order come from csrc/mma_ops.h.  The transposition patches keep their
// index expressions here (T[row * 36 + ...], the layout of mma_ops.h's patch_at / patch_row4): through the helpers the fused tails' register counts moved
// (254 -> 256, 246 -> 247) in kernels that sit at the limit of two workgroups per CU -- profiles/mma_ops_header.txt.
//
// This header holds the kernel templates and their constants; the kernels' body is csrc/conv_wino_x3_body.h (see ONEP, at the templates).  csrc/conv_wino_x3.hip
// instantiates the register-staged forms (and holds the weight packers), csrc/conv_wino_x3_dma.hip the LDS-DMA forms: two objects, so that the two staging paths
// build side by side.
#pragma once
#include <string.h>

#include "buffer_ops.h"
#include "mma_ops.h"
#include "suo_internal.h"
#include "tune.h"

namespace suo {

// (Tried and dropped, tools/bench_wino_x3.py: forcing the transform / fold additions into v_pk_add_f32 (-30 % VALU instructions) or into
// plain v_add_f32 changes nothing measurable; inline-asm VALU on MFMA results is unsafe -- hipcc's hazard recogniser does not see through it.)
__device__ __forceinline__ f32x4 x_sub4(f32x4 a, f32x4 b) { return a - b; }
__device__ __forceinline__ f32x4 x_add4(f32x4 a, f32x4 b) { return a + b; }
__device__ __forceinline__ void x_add16(f32x16& z, const f32x16& t) { z += t; }
__device__ __forceinline__ void x_sub16(f32x16& z, const f32x16& t) { z -= t; }

constexpr int X_CK = 16, X_PKH = 20, X_TH = 8, X_TW = 16, X_IH = 10, X_IW = 18, X_NPIX = X_IH * X_IW;

// NT = output channels / 32: 4 (128 channels: wave w owns n-tile w and all 16 components) or 2 (64 -> 64 channels: wave (wc, wn) owns n-tile wn and
// the 8 components of rows xi = 2 wc, 2 wc + 1 -- one accumulator each, no fold; the two halves meet through LDS before the epilogue, as in
// csrc/conv_wino.hip).
// NP = operand planes: 3 = three bf16 terms, six MFMAs per product block (csrc/bf16x3.h); 2 = two fp16 terms, three MFMAs (csrc/f16x2.h: the staged input times
// its site's 2^s (a.xscale), U's rows times 2^t_n, accumulators back to scale by a.oscale / a.oscale3 in the epilogues, a.range_flag raised beyond fp16's range)
// NEXT (fp16 form of the fused tail only): the block's output never comes back for the NEXT block's conv1 -- relu(bn_next(out2)) of the tile is split into LDS
// right where out2 is stored and multiplied by the next block's W1 (256 -> 128) here: the 256-channel tensor is written once and not re-read by a GEMM launch
// (csrc/net.hip: residual(..., next)).  Same products in the same order as gemm_bf16x3_kernel<NP = 2> forms them: bit-identical to the separate launch.
// W8 (round 6; 128 -> 128 channels, fp16 form): EIGHT waves on the tile for launches of at most one workgroup per CU (a one-frame call, the 2-7 crops of a SLAM
// pass).  There a workgroup's latency is the launch's duration -- 50 us for the fused tail whether 64 or 256 workgroups run, against 64 us per round of two co-resident
// ones in a 256-crop launch: stalls, not throughput -- so the tile's work is spread over twice the waves: wave (wn, wc) owns n-tile wn = w & 3 and the eight components
// of rows xi = 2 wc, 2 wc + 1 (wc = w >> 2) -- one accumulator each, half the products per wave, NO fold -- exactly the 64-channel form's scheme, the halves meeting
// through LDS after the K loop; a thread of the transform computes ONE row of B^T d B (four components); the tail's conv3 gives every wave one 32-channel n-tile of
// the 256.  Each output element is the same sum of the same products in the same order, except that Y = (R0 + R1) + R2 / (R3' - R2) + R1 pairs its rows as the
// 64-channel form does, where the four-wave form folds per chunk: results agree to fp32 rounding of that last addition, not bit for bit.
// DMA (the four-wave fp16 form; SUO_WINO_HALO_DMA=0 keeps the register-staged path, see conv3x3_wino_f16x2_dma below): the halo of chunk c + 1 goes from global memory
// STRAIGHT into the other halo buffer (buffer_load_dwordx4 ... lds: no VGPR destination, no ds_write_b128), 12 registers less across the transform.
//  - Layout: one wave-instruction writes 1 KiB lane-linear, so the pixel pitch is 16 floats (no padding) and float4 slot idx = tid + 256 i holds pixel P = idx >> 2
//    (P = 18 R + col) and channel quad (idx & 3) ^ ((R >> 1) & 3): the swizzle is on the SOURCE address (which quad a lane fetches; the four lanes of a pixel still
//    fetch its 64 contiguous bytes) and, the same one, in the transform's read addresses.  Bank arithmetic of the transform's ds_read_b128: a 16-lane group is 4 tile
//    rows t_ty x 4 consecutive tile columns t_tx of ONE quad tq; slot mod 16 = 4 (P mod 4) + (tq ^ ((R >> 1) & 3)), P = 36 t_ty + 2 t_tx + const: P mod 4 takes two
//    values (the parity of t_tx), (R >> 1) & 3 = (t_ty + const) & 3 four: 8 distinct 16-byte slots for 16 lanes, 2-way (unswizzled: 8-way; the padded pitch 20 of the
//    register path: conflict-free).  R >> 1 is t_ty or t_ty + 1 for a thread's four rows: two base addresses, every read a constant offset from one of them.
//  - Pixels outside the map (and slots 720-767): their lanes' offset is BUF_OOB in every chunk, and the slots are zeroed once with plain stores before the first DMA,
//    so it does not matter whether an out-of-range lane of the instruction writes zero or nothing.  Crop ends: the per-crop descriptor, as for the register path.
//  - The DMA is an asm statement (hipcc would wait vmcnt(0) for a DMA it knows of at the next ds_read): hipcc does not count it, so its own counted waits for the weight
//    loads only become stricter (vmcnt retires in order).  DMA(c + 1) is issued at the top of chunk c -- the last reads of that buffer ended before the first barrier
//    of chunk c - 1 -- and is retired before the barrier that closes chunk c: pairs 1 .. NPAIR - 1 have waited for weights requested after it; the explicit
//    vmcnt(4) there (the next chunk's first pair = 4 loads may stay in flight) states it.  The buffer is read one barrier later, at the top of chunk c + 1.
//  - The exact factor 2^s rides on the transform's first differences (32 products instead of 12; scaling by a power of two commutes with the additions: same bits), the
//    guard's running maximum on three ds_read_b128 of the lane's own slots of the landed buffer (the same elements the register path saw; max |x| 2^s = max |x 2^s|).
// SKD (the DMA form's tail with the up-sampled addend; SUO_WINO_SKIP_DMA=0 keeps the register loads, csrc/conv_wino_x3_skip_dma.hip): the epilogue's skip rows go from
// a.R into LDS by the same instruction, ONE EPILOGUE BLOCK AHEAD of their use.  Lane (lane >> 3, lane & 7) fetches the 16 bytes this same lane adds: one wave-
// instruction fills a 1 KiB lane-linear slot, the read back is the lane's own ds_read_b128, nothing crosses lanes and no workgroup barrier is involved.
//  - Four slots per wave (row groups k = 0..3 of one block at a time) behind everything else in S: 77 952 B per workgroup, two per CU as before.
//  - Order: block 0's four before pass 0's operand split; block b + 1's slot k right after block b's slot k has been read (lgkmcnt(0) inside the statement), before
//    block b's store k; pass 1's first block during pass 0's last.  Completion: explicit vmcnt(N), N derived where it is issued.
//  - A lane whose pixel is outside the map counts its slot as zero by a select: the rows a lane's slot sees differ from block to block (a tile's lower rows may be
//    outside where its upper rows are not), so zeroing the slots once, as the halo does, would not do.  o, and with it every stored bit, is the register path's.
//  - The per-column vectors (bias3, oscale3) come from LDS too: a load that hipcc counts, issued while a DMA is in flight, gets a wait that drains the DMA.  The addend's
//    own loads stay in registers: hipcc's waits for them retire a DMA or two of the block ahead early.
//  - Measured (profiles/wino_skip_dma.txt): this tail -7 % at 64x64.  The plain tail and the tail with the next block's conv1 were built the same way, also with a
//    six-slot ring: +-0 and +1 % -- what their skip rows cost is not the exposed round trip; they keep the register loads (profiles/REJECTED.md).
// A third weight slot for the freed registers (weights two pairs ahead) measured SLOWER than two (profiles/REJECTED.md): the ring stays two deep in both paths.
// ONEP (the LDS-DMA form's tail with NEXT; SUO_WINO_TAIL_ONE_PASS=0 keeps the two passes, csrc/conv_wino_x3_one_pass.hip): the tail's 1x1 stages in ONE pass over the
// 128-pixel tile, W3 and the next block's W1 streamed once per tile instead of once per 64-pixel pass -- see the tail's comment in the body.  Measured
// (profiles/wino_tail_one_pass.txt): the repeat alone is priced at -48 us of 1210 at 64x64; the one-pass form keeps -9 ... -17 us (-0.7 ... -1.4 %).  The plain
// tail was built the same way and did not gain (profiles/REJECTED.md): it keeps its two passes, as does the tail with the up-sampled addend, whose skip-row
// slots (SKD, 16 KB) do not fit beside a 66 KB operand.
//
// The body is csrc/conv_wino_x3_body.h, included INSIDE the two kernels below: wino3x3_x3_kernel keeps its nine parameters, so every existing instantiation keeps
// its name (tests and tools/kernel_digest.py know them) and, the body's text being what it was, its code; ONEP is the body's tenth, last parameter, fixed by the
// including kernel.  (As a device function inlined by both kernels the body compiled to different code in the existing kernels -- other register counts, the plain
// 128-channel 3x3 1 % slower -- though nothing in it had changed.)
template <bool FUSE, bool UP = false, bool TX3 = false, int NT = 4, int NP = 3, bool NEXT = false, bool SKD = false, bool W8 = false, bool DMA = false>
__global__ __launch_bounds__(W8 ? 512 : 256) __attribute__((amdgpu_waves_per_eu(2))) void wino3x3_x3_kernel(const ConvArgs a) {
    constexpr bool ONEP = false;
#include "conv_wino_x3_body.h"
}

template <bool FUSE, bool UP, bool TX3, int NT, int NP, bool NEXT, bool SKD, bool W8, bool DMA>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void wino3x3_x3_one_pass_kernel(const ConvArgs a) {
    constexpr bool ONEP = true;
#include "conv_wino_x3_body.h"
}

}  // namespace suo
