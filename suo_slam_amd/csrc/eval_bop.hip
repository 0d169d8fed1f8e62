// BOP-19 MSSD / MSPD pose errors -- the renderer-free two of the three terms of the BOP-19 average recall.
//
// Replaces bop_toolkit_lib/pose_error.py:96-144 (mssd, mspd) with misc.py:93-107 (project_pts) and misc.py:266-276 (transform_pts_Rt):
//   R_s = R_gt S_R,  t_s = R_gt S_t + t_gt                                  for every symmetry transformation s = [S_R|S_t] of the model
//   MSSD = min_s max_i |(R_est p_i + t_est) - (R_s p_i + t_s)|              (mm)
//   MSPD = min_s max_i |pi(K, R_est, t_est, p_i) - pi(K, R_s, t_s, p_i)|    (px),  pi = (K X)_xy / (K X)_z, divided as given
// in fp64 like the toolkit (the recall compares these errors with thresholds); the float32 points of the mesh database are widened exactly.
//
// Shape.  Lanes own points, symmetries are the loop: a workgroup takes one pair, one tile of BE_TILE = 1024 points (BE_NP = 4 per thread, in registers with
// their estimated-pose image and projection: 8 doubles a point) and one chunk of <= BE_SCH = 64 symmetries.  The composed [R_s|t_s] of the chunk are formed
// once per workgroup into LDS (thread = symmetry) and read back wave-uniform; K [R_est|t_est] likewise.  One pass over the points serves both errors: the
// transformed ground-truth point g = R_s p + t_s gives the 3-D distance and, through K g, the projection.  No P x S value leaves the registers: a wave reduces
// its per-symmetry maxima by shuffles, the workgroup's four waves meet in LDS, and one [n][S][2] block of per-symmetry maxima (squared) is merged across the
// point tiles with a 64-bit atomicMax on the bit pattern (non-negative doubles order like their patterns -- eval_pairs_kernel's trick with atomicMin).  A
// second, tiny kernel takes the minimum over the symmetries; the square root is taken once per pair on the host (sqrt is monotone and correctly rounded, so it
// commutes exactly with max and min).  max and min are exact, and the value of a (symmetry, point) does not depend on which lane computes it, so a result does
// not depend on the partition: a pair in a batch has the bits it has alone.  Lanes past the last point repeat point P - 1 (a maximum does not mind).
// A non-finite squared distance (z exactly 0, NaN or overflowing poses) is not a number fmax would keep: it sets a sticky per-pair flag instead and the pair
// reports +inf for that metric (the toolkit's min() over NaNs depends on their order).
// fp64 VALU work per (symmetry, point), no contraction: g 18, 3-D distance 8 + max 1 + flag 1, K g 15, two divisions ~2 x 17, 2-D distance 5 + max 1 + flag 1
// = ~84 instructions assumed; the per-symmetry wave reduction (6 shuffle steps x 2 values) adds ~10 % at 4 points per thread.  Compiled: 359 instructions per
// symmetry and thread (4 points), 306 of them fp64 VALU.  Measured: profiles/bop_errors.txt.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "../../include/suo_hip.h"
#include "suo_internal.h"
#include "mesh_db.h"

namespace suo {

constexpr int BE_BLOCK = 256;                    // threads per workgroup
constexpr int BE_NP = 4;                         // points per thread
constexpr int BE_TILE = BE_BLOCK * BE_NP;        // points per workgroup
constexpr int BE_SCH = 64;                       // most symmetries per workgroup
constexpr int BE_WG_TARGET = 1024;               // workgroups wanted where the problem allows: 256 CUs x 4

// (a0 b0 + a1 b1) + a2 b2, the order of a 3-term numpy dot
__device__ __forceinline__ double dot3(double a0, double b0, double a1, double b1, double a2, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

__global__ __launch_bounds__(BE_BLOCK) void bop_errors_kernel(BopArgs a) {
    __shared__ double Ts[BE_SCH][12];                         // [R_s|t_s] of the chunk
    __shared__ double Pe[12];                                 // K [R_est|t_est]
    __shared__ double red[BE_SCH][BE_BLOCK / 64][2];
    const int z = blockIdx.x, m = a.model[z];
    const int p_begin = a.off[m], P = a.off[m + 1] - p_begin;
    const int s_begin = a.soff[m], S = a.soff[m + 1] - s_begin;
    const int i0 = blockIdx.y * BE_TILE, s0 = blockIdx.z * a.chunk;
    if (i0 >= P || s0 >= S) return;                           // the grid is sized for the call's largest model
    const int ns = min(a.chunk, S - s0);
    const double* Te = a.Te + (size_t)z * 12;
    const double* Tg = a.Tg + (size_t)z * 12;
    const double* K = a.K + (size_t)z * 9;
    const int tid = threadIdx.x;
    if (tid < ns) {
        const double* Sy = a.sym + (size_t)(s_begin + s0 + tid) * 12;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) Ts[tid][i * 4 + j] = dot3(Tg[i * 4], Sy[j], Tg[i * 4 + 1], Sy[4 + j], Tg[i * 4 + 2], Sy[8 + j]);
            Ts[tid][i * 4 + 3] = dot3(Tg[i * 4], Sy[3], Tg[i * 4 + 1], Sy[7], Tg[i * 4 + 2], Sy[11]) + Tg[i * 4 + 3];
        }
    } else if (tid >= BE_BLOCK - 12) {                        // ns <= 64: these twelve threads are free
        const int e = tid - (BE_BLOCK - 12), i = e >> 2, j = e & 3;
        Pe[e] = dot3(K[i * 3], Te[j], K[i * 3 + 1], Te[4 + j], K[i * 3 + 2], Te[8 + j]);
    }
    __syncthreads();
    const float* pts = a.pts + (size_t)p_begin * 3;
    double px[BE_NP], py[BE_NP], pz[BE_NP], ex[BE_NP], ey[BE_NP], ez[BE_NP], eu[BE_NP], ev[BE_NP];
#pragma unroll
    for (int k = 0; k < BE_NP; ++k) {
        const int i = min(i0 + k * BE_BLOCK + tid, P - 1);
        const double x = (double)pts[(size_t)i * 3], y = (double)pts[(size_t)i * 3 + 1], w = (double)pts[(size_t)i * 3 + 2];
        px[k] = x; py[k] = y; pz[k] = w;
        ex[k] = dot3(Te[0], x, Te[1], y, Te[2], w) + Te[3];
        ey[k] = dot3(Te[4], x, Te[5], y, Te[6], w) + Te[7];
        ez[k] = dot3(Te[8], x, Te[9], y, Te[10], w) + Te[11];
        const double hu = dot3(Pe[0], x, Pe[1], y, Pe[2], w) + Pe[3];
        const double hv = dot3(Pe[4], x, Pe[5], y, Pe[6], w) + Pe[7];
        const double hw = dot3(Pe[8], x, Pe[9], y, Pe[10], w) + Pe[11];
        eu[k] = hu / hw; ev[k] = hv / hw;
    }
    const double K0 = K[0], K1 = K[1], K2 = K[2], K3 = K[3], K4 = K[4], K5 = K[5], K6 = K[6], K7 = K[7], K8 = K[8];
    bool bad3 = false, bad2 = false;
    const int lane = tid & 63, wave = tid >> 6;
    for (int s = 0; s < ns; ++s) {
        double T[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) T[e] = Ts[s][e];
        double m3 = 0.0, m2 = 0.0;
#pragma unroll
        for (int k = 0; k < BE_NP; ++k) {
            const double gx = dot3(T[0], px[k], T[1], py[k], T[2], pz[k]) + T[3];
            const double gy = dot3(T[4], px[k], T[5], py[k], T[6], pz[k]) + T[7];
            const double gz = dot3(T[8], px[k], T[9], py[k], T[10], pz[k]) + T[11];
            const double dx = ex[k] - gx, dy = ey[k] - gy, dz = ez[k] - gz;
            const double d3 = (dx * dx + dy * dy) + dz * dz;
            bad3 |= !(d3 < INFINITY);
            m3 = fmax(m3, d3);
            const double hu = dot3(K0, gx, K1, gy, K2, gz), hv = dot3(K3, gx, K4, gy, K5, gz), hw = dot3(K6, gx, K7, gy, K8, gz);
            const double du = eu[k] - hu / hw, dv = ev[k] - hv / hw;
            const double d2 = du * du + dv * dv;
            bad2 |= !(d2 < INFINITY);
            m2 = fmax(m2, d2);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { m3 = fmax(m3, __shfl_xor(m3, o)); m2 = fmax(m2, __shfl_xor(m2, o)); }
        if (lane == 0) { red[s][wave][0] = m3; red[s][wave][1] = m2; }
    }
    __syncthreads();
    if (tid < 2 * ns) {
        const int s = tid >> 1, c = tid & 1;
        double v = red[s][0][c];
#pragma unroll
        for (int w = 1; w < BE_BLOCK / 64; ++w) v = fmax(v, red[s][w][c]);
        atomicMax(&a.smax[((size_t)z * a.stride + s0 + s) * 2 + c], (unsigned long long)__double_as_longlong(v));
    }
    if (bad3 || bad2) atomicOr(&a.flags[z], (bad3 ? 1u : 0u) | (bad2 ? 2u : 0u));
}

// one workgroup per pair: the minimum over its symmetries of the merged maxima
__global__ __launch_bounds__(BE_BLOCK) void bop_errors_min_kernel(BopArgs a) {
    __shared__ double red[BE_BLOCK / 64][2];
    const int z = blockIdx.x, m = a.model[z];
    const int S = a.soff[m + 1] - a.soff[m];
    double v3 = INFINITY, v2 = INFINITY;
    for (int s = threadIdx.x; s < S; s += BE_BLOCK) {
        v3 = fmin(v3, __longlong_as_double((long long)a.smax[((size_t)z * a.stride + s) * 2]));
        v2 = fmin(v2, __longlong_as_double((long long)a.smax[((size_t)z * a.stride + s) * 2 + 1]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { v3 = fmin(v3, __shfl_xor(v3, o)); v2 = fmin(v2, __shfl_xor(v2, o)); }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = v3; red[threadIdx.x >> 6][1] = v2; }
    __syncthreads();
    if (threadIdx.x < 2) {
        double v = red[0][threadIdx.x];
        for (int w = 1; w < BE_BLOCK / 64; ++w) v = fmin(v, red[w][threadIdx.x]);
        a.out[(size_t)z * 2 + threadIdx.x] = v;
    }
}

// n_sym == nullptr: the identity alone for every model.  Caller holds db->mu.
static int set_symmetries_locked(MeshDb* db, const int* n_sym, const double* sym) {
    static const double ident[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    std::vector<int> off(db->n_models + 1, 0);
    for (int i = 0; i < db->n_models; ++i) off[i + 1] = off[i] + (n_sym ? n_sym[i] : 1);
    std::vector<double> host;
    if (!n_sym) {
        host.resize((size_t)db->n_models * 12);
        for (int i = 0; i < db->n_models; ++i) memcpy(&host[(size_t)i * 12], ident, sizeof(ident));
        sym = host.data();
    }
    double* s_dev = nullptr; int* o_dev = nullptr;
    const size_t sbytes = (size_t)off.back() * 12 * sizeof(double), obytes = off.size() * sizeof(int);
    hipError_t e = hipMalloc((void**)&s_dev, sbytes);
    if (e == hipSuccess) e = hipMalloc((void**)&o_dev, obytes);
    if (e == hipSuccess) e = hipMemcpy(s_dev, sym, sbytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(o_dev, off.data(), obytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (s_dev) (void)hipFree(s_dev);
        if (o_dev) (void)hipFree(o_dev);
        suo_set_error("suo_mesh_db_set_symmetries: %s", hipGetErrorString(e));
        return SUO_ERR_HIP;
    }
    if (db->sym_dev) (void)hipFree(db->sym_dev);
    if (db->sym_off_dev) (void)hipFree(db->sym_off_dev);
    db->sym_dev = s_dev; db->sym_off_dev = o_dev; db->sym_off = off;
    return SUO_OK;
}

}  // namespace suo

using namespace suo;

extern "C" int suo_mesh_db_set_symmetries(void* h, const int* n_sym, const double* sym) {
    MeshDb* db = (MeshDb*)h;
    if (!db || !n_sym || !sym) { suo_set_error("suo_mesh_db_set_symmetries: bad argument"); return SUO_ERR_ARG; }
    for (int i = 0; i < db->n_models; ++i)
        if (n_sym[i] < 1) { suo_set_error("suo_mesh_db_set_symmetries: model %d has %d symmetry transformations (the identity counts)", i, n_sym[i]); return SUO_ERR_ARG; }
    std::lock_guard<std::mutex> lk(db->mu);
    return set_symmetries_locked(db, n_sym, sym);
}

namespace suo {

// What suo_pose_errors_bop and suo_pose_nees (csrc/eval_nees_api.hip) share: the scratch layout, the staging of a call's pairs and the launch of
// bop_errors_kernel.  `extra` bytes behind the block of maxima (256-aligned, L->o_extra) are the caller's.  Caller holds db->mu and has checked the arguments.
int bop_maxima_enqueue_locked(MeshDb* db, const char* who, int n, const int* model_index, const double* T_est, const double* T_gt, const double* K, size_t extra,
                              BopLayout* L) {
    int rc;
    if (!db->sym_dev && (rc = set_symmetries_locked(db, nullptr, nullptr))) return rc;
    int pmax = 0, smax = 0;
    for (int i = 0; i < n; ++i) {
        const int mi = model_index[i];
        pmax = std::max(pmax, db->off[mi + 1] - db->off[mi]);
        smax = std::max(smax, db->sym_off[mi + 1] - db->sym_off[mi]);
    }
    // the staged pair block (stage_pairs_locked; K == NULL: MSPD not asked for)   then device-only: out[n][2] | flags[n] | smax[n][stride][2]
    const size_t o_out = pair_block_bytes(n), o_flags = o_out + (size_t)n * 16, o_smax = (o_flags + (size_t)n * 4 + 255) & ~(size_t)255;
    const size_t end = o_smax + (size_t)n * smax * 16;
    const size_t o_extra = extra ? (end + 255) & ~(size_t)255 : end;
    PairBlock B;
    if ((rc = stage_pairs_locked(db, n, model_index, T_est, T_gt, K, o_extra + extra, &B))) return rc;
    SUO_HIP_CHECK(hipMemsetAsync(db->scratch_dev + o_flags, 0, end - o_flags, db->stream));                             // +0.0: the identity of max over d^2 >= 0
    BopArgs a;
    a.pts = db->pts_dev; a.off = db->off_dev; a.sym = db->sym_dev; a.soff = db->sym_off_dev;
    a.Te = B.Te; a.Tg = B.Tg; a.K = B.K; a.model = B.model;
    a.out = (double*)(db->scratch_dev + o_out); a.flags = (unsigned*)(db->scratch_dev + o_flags); a.smax = (unsigned long long*)(db->scratch_dev + o_smax);
    a.stride = smax;
    // symmetry chunks: as many as bring the grid to BE_WG_TARGET workgroups, of 4..BE_SCH symmetries each (below 4 a workgroup's set-up of its points outweighs its loop)
    const int ptiles = (pmax + BE_TILE - 1) / BE_TILE;
    const long long wgs = (long long)n * ptiles;
    const int want = (int)std::max<long long>(1, (BE_WG_TARGET + wgs - 1) / wgs);
    a.chunk = std::min(smax, std::max(4, std::min(BE_SCH, (smax + want - 1) / want)));
    const int chunks = (smax + a.chunk - 1) / a.chunk;
    if (ptiles > 65535 || chunks > 65535) { suo_set_error("%s: %d points x %d symmetries exceed the grid", who, pmax, smax); return SUO_ERR_ARG; }
    hipLaunchKernelGGL(bop_errors_kernel, dim3(n, ptiles, chunks), dim3(BE_BLOCK), 0, db->stream, a);
    SUO_HIP_CHECK(hipGetLastError());
    L->args = a; L->o_out = o_out; L->o_flags = o_flags; L->o_extra = o_extra;
    return SUO_OK;
}

}  // namespace suo

extern "C" int suo_pose_errors_bop(void* h, int n, const int* model_index, const double* T_est, const double* T_gt, const double* K, double* mssd, double* mspd) {
    MeshDb* db = (MeshDb*)h;
    if (!db || n < 0 || (n > 0 && (!model_index || !T_est || !T_gt || (mspd && !K)))) { suo_set_error("suo_pose_errors_bop: bad argument"); return SUO_ERR_ARG; }
    if (n == 0) return SUO_OK;
    int rc;
    if ((rc = check_model_index("suo_pose_errors_bop", db, n, model_index, nullptr))) return rc;
    if (!mssd && !mspd) return SUO_OK;
    std::lock_guard<std::mutex> lk(db->mu);
    BopLayout L;
    if ((rc = bop_maxima_enqueue_locked(db, "suo_pose_errors_bop", n, model_index, T_est, T_gt, K, 0, &L))) return rc;
    const size_t o_out = L.o_out, o_flags = L.o_flags;
    hipLaunchKernelGGL(bop_errors_min_kernel, dim3(n), dim3(BE_BLOCK), 0, db->stream, L.args);
    SUO_HIP_CHECK(hipGetLastError());
    SUO_HIP_CHECK(hipMemcpyAsync(db->scratch_host + o_out, db->scratch_dev + o_out, o_flags + (size_t)n * 4 - o_out, hipMemcpyDeviceToHost, db->stream));
    SUO_HIP_CHECK(hipStreamSynchronize(db->stream));
    const double* o = (const double*)(db->scratch_host + o_out);
    const unsigned* fl = (const unsigned*)(db->scratch_host + o_flags);
    for (int i = 0; i < n; ++i) {
        if (mssd) mssd[i] = (fl[i] & 1u) ? INFINITY : sqrt(o[2 * i]);
        if (mspd) mspd[i] = (fl[i] & 2u) ? INFINITY : sqrt(o[2 * i + 1]);
    }
    return SUO_OK;
}
