// Mask pose errors of bop_toolkit from two renders: what pose_error.cus (pose_error.py:256-286) and pose_error.cou_bb_proj (:300-329)
// take from the depth images of the model at the estimated and at the ground-truth pose -- the pixel counts of the union and the intersection of the two
// masks depth > 0, and the two masks' pixel boxes.  The definition is in include/suo_hip.h (suo_pose_errors_masks); the quotients are the caller's.
//
// Shape.  masks_kernel is the tile pass of the rasteriser (csrc/raster_tile.h, the very code of raster_tile_kernel and gt_info_kernel) under a third epilogue.
// The renders of a call are staged pair by pair: render 2 i is the estimate of pair i, render 2 i + 1 its ground truth.  A workgroup takes one tile of one
// pair and draws the two renders into TWO 64 x 64 z-buffers in LDS (32 KiB); neither depth image is written to memory.  Per sample it counts est | gt and
// est & gt and widens the two integer boxes.  A lane keeps its 16 samples' ten integers in registers, a wave reduces them by shuffles, the four waves meet in
// LDS and the workgroup issues one integer atomic add / min / max per quantity into the pair's record, as gt_info_kernel does.  Integer sums and extrema do
// not depend on order: a pair has the same values alone, in a batch and on any tiling.  A workgroup whose tile misses both renders' pixel boxes leaves before
// it touches LDS; a render whose box misses the tile is not drawn.  The device writes integers only.
#include <limits.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/suo_hip.h"
#include "suo_internal.h"
#include "mesh_db.h"
#include "raster_tile.h"

namespace suo {

// a pair's record on the device, ints: two counts, then two boxes as x0 y0 (minima) x1 y1 (maxima)
constexpr int MK_UNION = 0, MK_INTER = 1, MK_EST = 2, MK_GT = 6, MK_REC = 10;
constexpr int MK_MAX_PAIRS = 1024;                       // pairs of one launch
constexpr long long MK_MAX_RECORDS = 1LL << 22;          // triangle records of one launch (88 bytes each), unless a single pair has more

__device__ __host__ __forceinline__ int mk_identity(int q) { return q < MK_EST ? 0 : ((q - MK_EST) & 3) < 2 ? INT_MAX : INT_MIN; }

__global__ void masks_init_kernel(int* rec, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n * MK_REC) rec[i] = mk_identity(i % MK_REC);
}

__global__ __launch_bounds__(RS_BLOCK) void masks_kernel(RasterArgs a, int* rec) {
    __shared__ unsigned zb[2 * RS_TILE * RS_TILE];                         // the estimate's buffer, then the ground truth's
    __shared__ int big[RS_BLOCK];
    __shared__ int nbig[2];
    __shared__ int red[RS_BLOCK / 64][MK_REC];
    const int pair = blockIdx.y, tid = threadIdx.x;
    const int X0 = ((int)blockIdx.x % a.tiles_x) * RS_TILE, Y0 = ((int)blockIdx.x / a.tiles_x) * RS_TILE;
    const int X1 = min(X0 + RS_TILE, a.w) - 1, Y1 = min(Y0 + RS_TILE, a.h) - 1;
    const bool meets[2] = {tile_meets_render(a, 2 * pair, X0, Y0, X1, Y1), tile_meets_render(a, 2 * pair + 1, X0, Y0, X1, Y1)};
    if (!meets[0] && !meets[1]) return;                                        // uniform over the workgroup: nothing is covered here
    for (int i = tid; i < 2 * RS_TILE * RS_TILE; i += RS_BLOCK) zb[i] = 0xFFFFFFFFu;
    for (int s = 0; s < 2; ++s) {
        if (!meets[s]) continue;                                               // uniform
        __syncthreads();                                                       // the buffers are set; the draw before this one has left big / nbig
        if (tid < 2) nbig[tid] = 0;
        __syncthreads();
        draw_tile(a, 2 * pair + s, X0, Y0, X1, Y1, zb + s * RS_TILE * RS_TILE, big, nbig);
    }
    __syncthreads();
    int v[MK_REC];
#pragma unroll
    for (int q = 0; q < MK_REC; ++q) v[q] = mk_identity(q);
    for (int k = 0; k < RS_TILE * RS_TILE / RS_BLOCK; ++k) {
        const int idx = k * RS_BLOCK + tid, lx = idx & (RS_TILE - 1), ly = idx / RS_TILE;
        const int x = X0 + lx, y = Y0 + ly;
        if (x > X1 || y > Y1) continue;                                        // the partial last column / row of the image
        const bool e = zb[idx] != 0xFFFFFFFFu, g = zb[RS_TILE * RS_TILE + idx] != 0xFFFFFFFFu;
        v[MK_UNION] += (e || g) ? 1 : 0;
        v[MK_INTER] += (e && g) ? 1 : 0;
        if (e) { v[MK_EST] = min(v[MK_EST], x); v[MK_EST + 1] = min(v[MK_EST + 1], y); v[MK_EST + 2] = max(v[MK_EST + 2], x); v[MK_EST + 3] = max(v[MK_EST + 3], y); }
        if (g) { v[MK_GT] = min(v[MK_GT], x); v[MK_GT + 1] = min(v[MK_GT + 1], y); v[MK_GT + 2] = max(v[MK_GT + 2], x); v[MK_GT + 3] = max(v[MK_GT + 3], y); }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int q = 0; q < MK_REC; ++q) {
            const int other = __shfl_xor(v[q], o);
            v[q] = q < MK_EST ? v[q] + other : ((q - MK_EST) & 3) < 2 ? min(v[q], other) : max(v[q], other);
        }
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < MK_REC; ++q) red[tid >> 6][q] = v[q];
    }
    __syncthreads();
    if (tid < MK_REC) {
        const bool sum = tid < MK_EST, lo = ((tid - MK_EST) & 3) < 2;
        int x = red[0][tid];
        for (int wv = 1; wv < RS_BLOCK / 64; ++wv) x = sum ? x + red[wv][tid] : lo ? min(x, red[wv][tid]) : max(x, red[wv][tid]);
        int* dst = rec + (size_t)pair * MK_REC + tid;
        if (sum) { if (x) atomicAdd(dst, x); }
        else if (lo) { if (x != INT_MAX) atomicMin(dst, x); }
        else if (x != INT_MIN) atomicMax(dst, x);
    }
}

}  // namespace suo

using namespace suo;

extern "C" int suo_pose_errors_masks(void* h, int n, const int* model_index, const double* T_est, const double* T_gt, const double* K, int width, int height,
                                     long long* counts_out, int* box_est, int* box_gt) {
    const char* who = "suo_pose_errors_masks";
    MeshDb* db = (MeshDb*)h;
    if (!db) { suo_set_error("%s: null mesh database", who); return SUO_ERR_ARG; }
    if (n < 0 || width < 1 || height < 1) { suo_set_error("%s: bad argument (n >= 0, width and height >= 1)", who); return SUO_ERR_ARG; }
    if (n > 0 && (!model_index || !T_est || !T_gt || !K || !counts_out || !box_est || !box_gt)) { suo_set_error("%s: null pointer", who); return SUO_ERR_ARG; }
    if (n == 0) return SUO_OK;
    // the renders, pair by pair: 2 i the estimate, 2 i + 1 the ground truth
    std::vector<int> model2((size_t)n * 2);
    std::vector<double> T2((size_t)n * 24), K2((size_t)n * 18);
    for (int i = 0; i < n; ++i) {
        model2[2 * (size_t)i] = model2[2 * (size_t)i + 1] = model_index[i];
        memcpy(&T2[(size_t)i * 24], T_est + (size_t)i * 12, 96);
        memcpy(&T2[(size_t)i * 24 + 12], T_gt + (size_t)i * 12, 96);
        memcpy(&K2[(size_t)i * 18], K + (size_t)i * 9, 72);
        memcpy(&K2[(size_t)i * 18 + 9], K + (size_t)i * 9, 72);
    }
    std::lock_guard<std::mutex> lk(db->mu);
    int rc;
    // the launches, each checked whole before the first one runs
    std::vector<int> cut{0};
    for (int b = 0; b < n;) {
        int e = b;
        long long records = 0;
        while (e < n && e - b < MK_MAX_PAIRS) {
            const int m = model_index[e];
            const long long F = (m >= 0 && m < db->n_models && !db->face_off.empty()) ? 2LL * (db->face_off[m + 1] - db->face_off[m]) : 0;
            if (e > b && records + F > MK_MAX_RECORDS) break;
            records += F;
            ++e;
        }
        if ((rc = check_render_args(who, db, 2 * (e - b), model2.data() + 2 * (size_t)b, T2.data() + (size_t)b * 24, K2.data() + (size_t)b * 18, width, height))) return rc;
        cut.push_back(e);
        b = e;
    }
    const int tiles_y = (height + RS_TILE - 1) / RS_TILE;
    for (size_t c = 0; c + 1 < cut.size(); ++c) {
        const int b = cut[c], m = cut[c + 1] - cut[c];
        const size_t bytes = (size_t)m * MK_REC * 4;
        if ((rc = ensure_scratch(db, bytes))) return rc;
        int* rec_dev = (int*)db->scratch_dev;
        RasterArgs a;
        if ((rc = render_setup_locked(db, who, 2 * m, model2.data() + 2 * (size_t)b, T2.data() + (size_t)b * 24, K2.data() + (size_t)b * 18, width, height, &a))) return rc;
        hipLaunchKernelGGL(masks_init_kernel, dim3((m * MK_REC + 255) / 256), dim3(256), 0, db->stream, rec_dev, m);
        hipLaunchKernelGGL(masks_kernel, dim3(a.tiles_x * tiles_y, m), dim3(RS_BLOCK), 0, db->stream, a, rec_dev);
        SUO_HIP_CHECK(hipGetLastError());
        SUO_HIP_CHECK(hipMemcpyAsync(db->scratch_host, db->scratch_dev, bytes, hipMemcpyDeviceToHost, db->stream));
        SUO_HIP_CHECK(hipStreamSynchronize(db->stream));
        const int* rec = (const int*)db->scratch_host;
        for (int i = 0; i < m; ++i) {
            const int* q = rec + (size_t)i * MK_REC;
            counts_out[(size_t)(b + i) * 2] = q[MK_UNION];
            counts_out[(size_t)(b + i) * 2 + 1] = q[MK_INTER];
            for (int s = 0; s < 2; ++s) {
                const int* bx = q + (s ? MK_GT : MK_EST);
                int* dst = (s ? box_gt : box_est) + (size_t)(b + i) * 4;
                if (bx[0] > bx[2]) { dst[0] = dst[1] = dst[2] = dst[3] = -1; continue; }      // an empty mask
                dst[0] = bx[0]; dst[1] = bx[1]; dst[2] = bx[2] - bx[0]; dst[3] = bx[3] - bx[1];
            }
        }
    }
    return SUO_OK;
}
