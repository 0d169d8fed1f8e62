// Point-set pose errors of bop_toolkit: ADD, ADI and PROJ -- the error functions of eval_calc_errors.py that need the model's points but
// no symmetry set and no renderer.
//
// Replaces bop_toolkit_lib/pose_error.py:147-232 (add, adi, proj) with misc.py:93-107 (project_pts) and misc.py:266-276 (transform_pts_Rt):
//   ADD  = mean_i |E p_i - G p_i|                                (mm)     E = [R_est|t_est], G = [R_gt|t_gt]
//   ADI  = mean_i min_j |G p_i - E p_j|                          (mm)     the toolkit's direction: cKDTree(pts_est).query(pts_gt) -- for every GROUND-TRUTH point
//                                                                         the nearest ESTIMATED-pose point (csrc/eval.hip's float32 ADD-S is the reference meter's)
//   PROJ = mean_i |pi(K, E, p_i) - pi(K, G, p_i)|                (px)     pi = (P [p;1])_xy / (P [p;1])_z with P = K [R|t], divided as given
// in fp64 like the toolkit, on the float32 points of the mesh database widened exactly.
//
// Shape.  ADI is the work: P^2 pairs.  Lanes own ground-truth points (PE_G = 4 per thread, in registers), the estimated-pose points of a tile are transformed
// once into LDS (32 bytes a point: x, y, z and a pad, so that a point is one ds_read_b128 and one ds_read_b64) and read back wave-uniform -- every lane reads the
// same address, which the LDS serves as a broadcast whatever the bank.  The running minimum is kept of the SQUARED distance (sqrt is monotone and correctly
// rounded, so it commutes exactly with min) and the square root is taken once per point.  A pair's estimated-pose points are split over blockIdx.z to fill the
// device, and the point tiles of one pair meet in a 64-bit atomicMin on the bit pattern (non-negative doubles order like their patterns) -- eval_pairs_kernel's
// trick in the width of bop_errors_kernel's.  min is exact and the value of an (i, j) does not depend on which lane computes it, so the merged minima do not
// depend on the partition.
// The means are formed by a second kernel, one workgroup per pair, which also computes ADD and PROJ directly (P terms each): thread t sums the points t, t + 256,
// ... in that order, a wave adds its lanes by a shuffle tree, thread 0 adds the four waves in order.  That order depends on P alone: a pair has the same bits
// alone and in a batch.
// Non-finite values.  A transformed point with a non-finite coordinate (a NaN or overflowing pose) makes ADD and ADI of its pair +inf; a non-finite projected
// distance (z exactly 0) makes PROJ +inf.  Nothing is indexed by a computed value, so no input can make the kernels fault.
// fp64 VALU work per (i, j): 3 subtractions, 3 multiplications, 2 additions, 1 minimum = 9 instructions without contraction.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "../../include/suo_hip.h"
#include "suo_internal.h"
#include "mesh_db.h"

namespace suo {

constexpr int PE_BLOCK = 256;                    // threads per workgroup
constexpr int PE_G = 4;                          // ground-truth points per thread
constexpr int PE_GTILE = PE_BLOCK * PE_G;        // ground-truth points per workgroup
constexpr int PE_TILE = 512;                     // estimated-pose points staged in LDS per pass (16 KiB)
constexpr int PE_WG_TARGET = 2048;               // workgroups wanted where the problem allows: 256 CUs x 8

struct PointsArgs {
    const float* pts; const int* off;            // mesh database
    const int* model;                            // [n]
    const double* Te; const double* Tg;          // [n][12] row-major 3x4
    const double* K;                             // [n][9]
    unsigned long long* mind2;                   // [n][stride] bit patterns of min_j d^2
    double* out;                                 // [n][3] ADD, ADI, PROJ
    int stride, splits, which;
};

// ((r0 x + r1 y) + r2 z) + t, the order of eval_bop.hip and raster.hip
__device__ __forceinline__ double row3(const double* T, double x, double y, double z) { return ((T[0] * x + T[1] * y) + T[2] * z) + T[3]; }

struct __attribute__((aligned(16))) PePoint { double x, y, z, pad; };

__global__ __launch_bounds__(PE_BLOCK) void points_adi_kernel(PointsArgs a) {
    __shared__ PePoint tile[PE_TILE];
    const int z = blockIdx.x, m = a.model[z];
    const int p_begin = a.off[m], P = a.off[m + 1] - p_begin;
    const int g0 = blockIdx.y * PE_GTILE;
    if (g0 >= P) return;                                      // the grid is sized for the call's largest model
    int chunk = (P + a.splits - 1) / a.splits;
    chunk = (chunk + PE_TILE - 1) / PE_TILE * PE_TILE;
    const int j0 = blockIdx.z * chunk, j1 = min(P, j0 + chunk);
    if (j0 >= P) return;
    const float* pts = a.pts + (size_t)p_begin * 3;
    double Te[12], Tg[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) { Te[k] = a.Te[(size_t)z * 12 + k]; Tg[k] = a.Tg[(size_t)z * 12 + k]; }
    double gx[PE_G], gy[PE_G], gz[PE_G], best[PE_G];
#pragma unroll
    for (int k = 0; k < PE_G; ++k) {
        const int g = min(g0 + k * PE_BLOCK + (int)threadIdx.x, P - 1);
        const double x = (double)pts[(size_t)g * 3], y = (double)pts[(size_t)g * 3 + 1], w = (double)pts[(size_t)g * 3 + 2];
        gx[k] = row3(Tg, x, y, w); gy[k] = row3(Tg + 4, x, y, w); gz[k] = row3(Tg + 8, x, y, w);
        best[k] = INFINITY;
    }
    for (int j = j0; j < j1; j += PE_TILE) {
        const int cnt = min(PE_TILE, j1 - j);
        __syncthreads();
        for (int t = threadIdx.x; t < cnt; t += PE_BLOCK) {
            const double x = (double)pts[(size_t)(j + t) * 3], y = (double)pts[(size_t)(j + t) * 3 + 1], w = (double)pts[(size_t)(j + t) * 3 + 2];
            PePoint v;
            v.x = row3(Te, x, y, w); v.y = row3(Te + 4, x, y, w); v.z = row3(Te + 8, x, y, w); v.pad = 0.0;
            tile[t] = v;
        }
        __syncthreads();
#pragma unroll 4
        for (int t = 0; t < cnt; ++t) {
            const double ex = tile[t].x, ey = tile[t].y, ez = tile[t].z;
#pragma unroll
            for (int k = 0; k < PE_G; ++k) {
                const double dx = gx[k] - ex, dy = gy[k] - ey, dz = gz[k] - ez;
                best[k] = fmin(best[k], (dx * dx + dy * dy) + dz * dz);      // a NaN never becomes the minimum; the pair is caught by points_mean_kernel
            }
        }
    }
#pragma unroll
    for (int k = 0; k < PE_G; ++k) {
        const int g = g0 + k * PE_BLOCK + (int)threadIdx.x;
        if (g < P) atomicMin(&a.mind2[(size_t)z * a.stride + g], (unsigned long long)__double_as_longlong(best[k]));
    }
}

__device__ __forceinline__ bool finite3(double x, double y, double z) { return fabs(x) < INFINITY && fabs(y) < INFINITY && fabs(z) < INFINITY; }

// one workgroup per pair: ADD and PROJ directly, ADI from the merged minima; the order of the sums depends on P alone
__global__ __launch_bounds__(PE_BLOCK) void points_mean_kernel(PointsArgs a) {
    __shared__ double Pm[2][12];                              // K [R_est|t_est], K [R_gt|t_gt]
    __shared__ double red[PE_BLOCK / 64][3];
    const int z = blockIdx.x, m = a.model[z];
    const int p_begin = a.off[m], P = a.off[m + 1] - p_begin;
    const float* pts = a.pts + (size_t)p_begin * 3;
    const int tid = threadIdx.x;
    double Te[12], Tg[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) { Te[k] = a.Te[(size_t)z * 12 + k]; Tg[k] = a.Tg[(size_t)z * 12 + k]; }
    if (tid < 24) {
        const double* K = a.K + (size_t)z * 9;
        const double* T = (tid < 12 ? a.Te : a.Tg) + (size_t)z * 12;
        const int e = tid % 12, i = e >> 2, j = e & 3;
        Pm[tid / 12][e] = (K[i * 3] * T[j] + K[i * 3 + 1] * T[4 + j]) + K[i * 3 + 2] * T[8 + j];
    }
    __syncthreads();
    const bool want_adi = a.which & 2, want_proj = a.which & 4;
    double s_add = 0.0, s_adi = 0.0, s_proj = 0.0;
    for (int g = tid; g < P; g += PE_BLOCK) {
        const double x = (double)pts[(size_t)g * 3], y = (double)pts[(size_t)g * 3 + 1], w = (double)pts[(size_t)g * 3 + 2];
        const double ex = row3(Te, x, y, w), ey = row3(Te + 4, x, y, w), ez = row3(Te + 8, x, y, w);
        const double qx = row3(Tg, x, y, w), qy = row3(Tg + 4, x, y, w), qz = row3(Tg + 8, x, y, w);
        const double poison = finite3(ex, ey, ez) && finite3(qx, qy, qz) ? 0.0 : INFINITY;
        const double dx = ex - qx, dy = ey - qy, dz = ez - qz;
        s_add += sqrt((dx * dx + dy * dy) + dz * dz);
        if (want_adi) s_adi += sqrt(__longlong_as_double((long long)a.mind2[(size_t)z * a.stride + g])) + poison;
        if (want_proj) {
            const double eu = row3(Pm[0], x, y, w), ev = row3(Pm[0] + 4, x, y, w), ew = row3(Pm[0] + 8, x, y, w);
            const double qu = row3(Pm[1], x, y, w), qv = row3(Pm[1] + 4, x, y, w), qw = row3(Pm[1] + 8, x, y, w);
            const double du = eu / ew - qu / qw, dv = ev / ew - qv / qw;
            s_proj += sqrt(du * du + dv * dv);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s_add += __shfl_down(s_add, o); s_adi += __shfl_down(s_adi, o); s_proj += __shfl_down(s_proj, o); }
    if ((tid & 63) == 0) { red[tid >> 6][0] = s_add; red[tid >> 6][1] = s_adi; red[tid >> 6][2] = s_proj; }
    __syncthreads();
    if (tid < 3) {
        double s = red[0][tid];
        for (int w = 1; w < PE_BLOCK / 64; ++w) s += red[w][tid];
        const double mean = s / (double)P;
        a.out[(size_t)z * 3 + tid] = mean < INFINITY ? mean : INFINITY;      // a NaN or inf anywhere in the sum: +inf
    }
}

}  // namespace suo

using namespace suo;

extern "C" int suo_pose_errors_points(void* h, int n, const int* model_index, const double* T_est, const double* T_gt, const double* K, int which, double* add_out,
                                      double* adi_out, double* proj_out) {
    MeshDb* db = (MeshDb*)h;
    const bool w_add = which & SUO_POINTS_ADD, w_adi = which & SUO_POINTS_ADI, w_proj = which & SUO_POINTS_PROJ;
    if (!db || n < 0 || (which & ~(SUO_POINTS_ADD | SUO_POINTS_ADI | SUO_POINTS_PROJ)) ||
        (n > 0 && (!model_index || !T_est || !T_gt || (w_add && !add_out) || (w_adi && !adi_out) || (w_proj && (!proj_out || !K))))) {
        suo_set_error("suo_pose_errors_points: bad argument");
        return SUO_ERR_ARG;
    }
    if (n == 0 || !which) return SUO_OK;
    int pmax = 0, rc;
    if ((rc = check_model_index("suo_pose_errors_points", db, n, model_index, &pmax))) return rc;
    std::lock_guard<std::mutex> lk(db->mu);
    const int stride = w_adi ? (pmax + 63) & ~63 : 0;
    // the staged pair block (stage_pairs_locked; K == NULL: PROJ not asked for)   then device-only: out[n][3] | mind2[n][stride]
    const size_t o_out = pair_block_bytes(n), o_min = (o_out + (size_t)n * 24 + 255) & ~(size_t)255, total = o_min + (size_t)n * stride * 8;
    PairBlock B;
    if ((rc = stage_pairs_locked(db, n, model_index, T_est, T_gt, K, total, &B))) return rc;
    PointsArgs a;
    a.pts = db->pts_dev; a.off = db->off_dev;
    a.Te = B.Te; a.Tg = B.Tg; a.K = B.K; a.model = B.model;
    a.out = (double*)(db->scratch_dev + o_out); a.mind2 = (unsigned long long*)(db->scratch_dev + o_min);
    a.stride = stride; a.which = which; a.splits = 1;
    if (w_adi) {
        // all ones: above every bit pattern; points_adi_kernel's split 0 writes every point of every pair
        SUO_HIP_CHECK(hipMemsetAsync(db->scratch_dev + o_min, 0xff, (size_t)n * stride * 8, db->stream));
        const int gtiles = (pmax + PE_GTILE - 1) / PE_GTILE;
        const long long wgs = (long long)n * gtiles;
        const int splits = (int)std::max<long long>(1, std::min<long long>((PE_WG_TARGET + wgs - 1) / wgs, (pmax + PE_TILE - 1) / PE_TILE));
        if (gtiles > 65535 || splits > 65535) { suo_set_error("suo_pose_errors_points: %d points exceed the grid", pmax); return SUO_ERR_ARG; }
        a.splits = splits;
        hipLaunchKernelGGL(points_adi_kernel, dim3(n, gtiles, splits), dim3(PE_BLOCK), 0, db->stream, a);
        SUO_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(points_mean_kernel, dim3(n), dim3(PE_BLOCK), 0, db->stream, a);
    SUO_HIP_CHECK(hipGetLastError());
    SUO_HIP_CHECK(hipMemcpyAsync(db->scratch_host + o_out, db->scratch_dev + o_out, (size_t)n * 24, hipMemcpyDeviceToHost, db->stream));
    SUO_HIP_CHECK(hipStreamSynchronize(db->stream));
    const double* o = (const double*)(db->scratch_host + o_out);
    for (int i = 0; i < n; ++i) {
        if (w_add) add_out[i] = o[3 * i];
        if (w_adi) adi_out[i] = o[3 * i + 1];
        if (w_proj) proj_out[i] = o[3 * i + 2];
    }
    return SUO_OK;
}
