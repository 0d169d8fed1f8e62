// BOP scene_gt_info and ground-truth masks: what bop_toolkit's scripts/calc_gt_info.py:74-176 and scripts/calc_gt_masks.py:77-127
// compute per ground-truth instance from a render of the model and the test depth image -- px_count_all / valid / visib, bbox_obj, bbox_visib, and the
// mask / mask_visib images.  The definition is in include/suo_hip.h (suo_gt_info); tests/gt_info_ref.py restates it in numpy.
//
// Shape.  calc_gt_info.py renders on a canvas of 3W x 3H so that the truncated part of an object is counted; that canvas (14 MB an instance at 720 x 540) is
// never written to memory here.  gt_info_kernel is the tile pass of the rasteriser (csrc/raster_tile.h, the very code of raster_tile_kernel) under a second
// epilogue that runs while the 64 x 64 z-buffer of the tile is still in LDS:
//   every covered sample of the tile counts towards px_count_all and widens the integer box of the object (in image coordinates: canvas minus the offset);
//   a covered sample inside the W x H window -- membership is decided per sample, the window is not tile-aligned -- loads the test depth of its pixel, forms
//   the two fp64 distances in the order of misc.depth_im_to_dist_im and the 'bop19' visibility (csrc/visib.h, shared with csrc/eval_vsd.hip), counts
//   valid and visible pixels and widens the visible box; the mask form (canvas multiplier 1, offsets 0) also stores the two uint8 masks of the tile.
// A lane keeps its 16 samples' eleven integers in registers, a wave reduces them by shuffles, the four waves meet in LDS and the workgroup issues one integer
// atomic add / min / max per quantity into the instance's record, which gt_info_init_kernel has set.  Integer sums and extrema do not depend on order: an
// instance has the same values alone, in a batch and on any tiling.  A workgroup whose tile misses the render's pixel box leaves before it touches LDS or
// reads a triangle; an uncovered sample has distance 0, is neither valid nor visible, and needs no test depth.  The device writes integers (and mask bytes) only.
#include <limits.h>
#include <math.h>

#include "../../include/suo_hip.h"
#include "suo_internal.h"
#include "gt_info.h"
#include "visib.h"

namespace suo {

__global__ void gt_info_init_kernel(int* rec, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * GI_REC) return;
    const int q = i % GI_REC;
    rec[i] = q < GI_OBJ ? 0 : ((q - GI_OBJ) & 3) < 2 ? INT_MAX : INT_MIN;      // counts | x0 y0 (minima) x1 y1 (maxima), twice
}

__global__ __launch_bounds__(RS_BLOCK) void gt_info_kernel(GtInfoArgs g) {
    __shared__ unsigned zb[RS_TILE * RS_TILE];
    __shared__ int big[RS_BLOCK];
    __shared__ int nbig[2];
    __shared__ int red[RS_BLOCK / 64][GI_REC];
    const RasterArgs& a = g.ras;
    const int r = blockIdx.y, tid = threadIdx.x;
    const int X0 = ((int)blockIdx.x % a.tiles_x) * RS_TILE, Y0 = ((int)blockIdx.x / a.tiles_x) * RS_TILE;
    const int X1 = min(X0 + RS_TILE, a.w) - 1, Y1 = min(Y0 + RS_TILE, a.h) - 1;
    if (!tile_meets_render(a, r, X0, Y0, X1, Y1)) return;                      // uniform over the workgroup: nothing is covered here
    for (int i = tid; i < RS_TILE * RS_TILE; i += RS_BLOCK) zb[i] = 0xFFFFFFFFu;
    if (tid < 2) nbig[tid] = 0;
    __syncthreads();
    draw_tile(a, r, X0, Y0, X1, Y1, zb, big, nbig);

    const double fx = g.kim[(size_t)r * 4], fy = g.kim[(size_t)r * 4 + 1], cx = g.kim[(size_t)r * 4 + 2], cy = g.kim[(size_t)r * 4 + 3];
    const double ifx = 1.0 / fx, ify = 1.0 / fy;
    const size_t hw = (size_t)g.H * g.W;
    const float* test = g.test + (size_t)g.image_index[r] * hw;
    unsigned char* mask = g.mask ? g.mask + (size_t)r * hw : nullptr;
    unsigned char* mask_visib = g.mask_visib ? g.mask_visib + (size_t)r * hw : nullptr;
    int v[GI_REC];
#pragma unroll
    for (int q = 0; q < GI_REC; ++q) v[q] = q < GI_OBJ ? 0 : ((q - GI_OBJ) & 3) < 2 ? INT_MAX : INT_MIN;
    for (int k = 0; k < RS_TILE * RS_TILE / RS_BLOCK; ++k) {
        const int idx = k * RS_BLOCK + tid, lx = idx & (RS_TILE - 1), ly = idx / RS_TILE;
        if (X0 + lx > X1 || Y0 + ly > Y1) continue;                            // the partial last column / row of the canvas
        const unsigned z = zb[idx];
        const bool covered = z != 0xFFFFFFFFu;
        const int x = X0 + lx - g.off_x, y = Y0 + ly - g.off_y;                // image coordinates
        const bool inside = x >= 0 && x < g.W && y >= 0 && y < g.H;
        bool visib = false;
        if (covered) {
            ++v[GI_ALL];
            v[GI_OBJ] = min(v[GI_OBJ], x); v[GI_OBJ + 1] = min(v[GI_OBJ + 1], y); v[GI_OBJ + 2] = max(v[GI_OBJ + 2], x); v[GI_OBJ + 3] = max(v[GI_OBJ + 3], y);
            if (inside) {
                const double dg = (double)__uint_as_float(z), dt = (double)test[(size_t)y * g.W + x];
                const double mx = (double)x - cx, my = (double)y - cy;
                const double gx = (mx * dg) * ifx, gy = (my * dg) * ify, tx = (mx * dt) * ifx, ty = (my * dt) * ify;
                const double Dg = sqrt((gx * gx + gy * gy) + dg * dg);
                const double Dt = sqrt((tx * tx + ty * ty) + dt * dt);
                visib = visib_bop19(Dg, Dt, g.delta);
                if (Dg > 0.0 && Dt > 0.0) ++v[GI_VALID];
                if (visib) {
                    ++v[GI_VISIB];
                    v[GI_VIS] = min(v[GI_VIS], x); v[GI_VIS + 1] = min(v[GI_VIS + 1], y); v[GI_VIS + 2] = max(v[GI_VIS + 2], x); v[GI_VIS + 3] = max(v[GI_VIS + 3], y);
                }
            }
        }
        if (inside) {                                                          // the mask form: its buffers were cleared, so only tiles that draw store
            if (mask) mask[(size_t)y * g.W + x] = covered ? 255 : 0;
            if (mask_visib) mask_visib[(size_t)y * g.W + x] = visib ? 255 : 0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int q = 0; q < GI_REC; ++q) {
            const int other = __shfl_xor(v[q], o);
            v[q] = q < GI_OBJ ? v[q] + other : ((q - GI_OBJ) & 3) < 2 ? min(v[q], other) : max(v[q], other);
        }
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < GI_REC; ++q) red[tid >> 6][q] = v[q];
    }
    __syncthreads();
    if (tid < GI_REC) {
        const bool sum = tid < GI_OBJ, lo = ((tid - GI_OBJ) & 3) < 2;
        int x = red[0][tid];
        for (int wv = 1; wv < RS_BLOCK / 64; ++wv) x = sum ? x + red[wv][tid] : lo ? min(x, red[wv][tid]) : max(x, red[wv][tid]);
        int* dst = g.rec + (size_t)r * GI_REC + tid;
        if (sum) { if (x) atomicAdd(dst, x); }
        else if (lo) { if (x != INT_MAX) atomicMin(dst, x); }
        else if (x != INT_MIN) atomicMax(dst, x);
    }
}

void gt_info_enqueue(const GtInfoArgs& g, int n, int tiles, hipStream_t stream) {
    hipLaunchKernelGGL(gt_info_init_kernel, dim3((n * GI_REC + 255) / 256), dim3(256), 0, stream, g.rec, n);
    hipLaunchKernelGGL(gt_info_kernel, dim3(tiles, n), dim3(RS_BLOCK), 0, stream, g);
}

}  // namespace suo
