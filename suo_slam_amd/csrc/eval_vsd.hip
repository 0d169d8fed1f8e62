// BOP-19 VSD pose error -- the third term of the BOP-19 average recall, on depth images rendered by csrc/raster.hip.
//
// Replaces bop_toolkit_lib/pose_error.py:40-93 (vsd, cost 'step') with misc.py:130-163 (depth_im_to_dist_im_fast) and visibility.py:9-75 (mode 'bop19'),
// operation for operation (this library is built with contraction off):
//   pre_X = (x - cx) / fx,  pre_Y = (y - cy) / fy                                       fp64, no half pixel (the toolkit has none)
//   dist(d) = sqrt(((pre_X d)^2 + (pre_Y d)^2) + d^2)                                    fp64 on the float32 depth widened exactly
//   visib_gt  = (float32(dist_gt) - float32(dist_test) <= float32(delta) or dist_test == 0) and dist_gt > 0
//   visib_est = (the same for est) or (visib_gt and dist_est > 0)
//   cost_t = #{intersection: |dist_gt - dist_est| [/ diameter] >= tau_t},   e_t = (cost_t + union - intersection) / union,  1.0 when union == 0
// Shape.  One workgroup per (pair, 64 x 64-pixel tile of the image); a tile outside the union of the two renders' pixel boxes leaves at once (both model
// depths are 0 there and no mask is set).  A lane counts union, intersection and the costs of its 16 pixels in registers; a wave adds them by shuffles, the
// four waves meet in LDS and the workgroup adds each counter with one integer atomic.  Integer sums do not depend on the launch shape.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <vector>

#include "../../include/suo_hip.h"
#include "suo_internal.h"
#include "mesh_db.h"
#include "visib.h"

namespace suo {

constexpr int VS_BLOCK = 256;
constexpr int VS_TILE = 64;
constexpr int VS_MAXT = 16;                      // most misalignment tolerances per call (the toolkit uses 10)

struct VsdArgs {
    const float* img;                            // rendered depth images [.][h][w]
    const int* r_est; const int* r_gt;           // [n] image of a pair's estimate / ground truth within img
    const int* rbox;                             // [.][4] pixel boxes of the renders, or nullptr: the whole image
    const float* test; const int* image_index;   // [n_images][h][w] mm, [n]
    const double* K; const double* taus; const double* diam;
    unsigned long long* counts;                  // [n][2 + n_taus] union, intersection, cost per tau
    float delta;
    int n_taus, normalized, w, h, tiles_x;
};

__global__ __launch_bounds__(VS_BLOCK) void vsd_kernel(VsdArgs a) {
    __shared__ unsigned red[VS_BLOCK / 64][2 + VS_MAXT];
    const int i = blockIdx.y, tid = threadIdx.x;
    const int X0 = ((int)blockIdx.x % a.tiles_x) * VS_TILE, Y0 = ((int)blockIdx.x / a.tiles_x) * VS_TILE;
    const int re = a.r_est[i], rg = a.r_gt[i];
    if (a.rbox) {
        const int x0 = min(a.rbox[re * 4], a.rbox[rg * 4]), y0 = min(a.rbox[re * 4 + 1], a.rbox[rg * 4 + 1]);
        const int x1 = max(a.rbox[re * 4 + 2], a.rbox[rg * 4 + 2]), y1 = max(a.rbox[re * 4 + 3], a.rbox[rg * 4 + 3]);
        if (x0 > X0 + VS_TILE - 1 || x1 < X0 || y0 > Y0 + VS_TILE - 1 || y1 < Y0) return;      // uniform over the workgroup
    }
    const size_t hw = (size_t)a.h * a.w;
    const float* de_im = a.img + (size_t)re * hw;
    const float* dg_im = a.img + (size_t)rg * hw;
    const float* dt_im = a.test + (size_t)a.image_index[i] * hw;
    const double fx = a.K[(size_t)i * 9], fy = a.K[(size_t)i * 9 + 4], cx = a.K[(size_t)i * 9 + 2], cy = a.K[(size_t)i * 9 + 5];
    const double diam = a.diam[i];
    double tau[VS_MAXT];
    unsigned cost[VS_MAXT];
#pragma unroll
    for (int t = 0; t < VS_MAXT; ++t) { tau[t] = t < a.n_taus ? a.taus[t] : INFINITY; cost[t] = 0; }
    unsigned n_union = 0, n_inter = 0;
    for (int k = 0; k < VS_TILE * VS_TILE / VS_BLOCK; ++k) {
        const int idx = k * VS_BLOCK + tid, x = X0 + (idx & (VS_TILE - 1)), y = Y0 + idx / VS_TILE;
        if (x >= a.w || y >= a.h) continue;
        const size_t p = (size_t)y * a.w + x;
        const float dg = dg_im[p], de = de_im[p];
        if (dg == 0.0f && de == 0.0f) continue;                                // neither mask can be set: both need a model distance > 0
        const double dt = (double)dt_im[p];
        const double pX = ((double)x - cx) / fx, pY = ((double)y - cy) / fy;
        const double tx = pX * dt, ty = pY * dt, gx = pX * (double)dg, gy = pY * (double)dg, ex = pX * (double)de, ey = pY * (double)de;
        const double Dt = sqrt((tx * tx + ty * ty) + dt * dt);
        const double Dg = sqrt((gx * gx + gy * gy) + (double)dg * (double)dg);
        const double De = sqrt((ex * ex + ey * ey) + (double)de * (double)de);
        const bool vg = visib_bop19(Dg, Dt, a.delta);
        const bool ve = visib_bop19(De, Dt, a.delta) || (vg && De > 0.0);
        if (vg || ve) ++n_union;
        if (vg && ve) {
            ++n_inter;
            double d = fabs(Dg - De);
            if (a.normalized) d /= diam;
#pragma unroll
            for (int t = 0; t < VS_MAXT; ++t) cost[t] += d >= tau[t] ? 1u : 0u;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n_union += __shfl_xor(n_union, o); n_inter += __shfl_xor(n_inter, o);
#pragma unroll
        for (int t = 0; t < VS_MAXT; ++t) cost[t] += __shfl_xor(cost[t], o);
    }
    if ((tid & 63) == 0) {
        red[tid >> 6][0] = n_union; red[tid >> 6][1] = n_inter;
#pragma unroll
        for (int t = 0; t < VS_MAXT; ++t) red[tid >> 6][2 + t] = cost[t];
    }
    __syncthreads();
    if (tid < 2 + a.n_taus) {
        unsigned v = 0;
        for (int wv = 0; wv < VS_BLOCK / 64; ++wv) v += red[wv][tid];
        if (v) atomicAdd(&a.counts[(size_t)i * (2 + a.n_taus) + tid], (unsigned long long)v);
    }
}

static int check_vsd_args(const char* who, int n, int width, int height, int n_images, const float* depth_test, const int* image_index, const double* K,
                          double delta, int n_taus, const double* taus, int normalized, const double* diameter, const double* errors) {
    if (n < 0 || width < 1 || height < 1 || n_taus < 1 || n_taus > VS_MAXT || !taus || !std::isfinite(delta) ||
        (n > 0 && (n_images < 1 || !depth_test || !image_index || !K || !errors || (normalized && !diameter)))) {
        suo_set_error("%s: bad argument (1 <= n_taus <= %d)", who, VS_MAXT);
        return SUO_ERR_ARG;
    }
    if (n > 65535 || (long long)width * height > (1LL << 28)) { suo_set_error("%s: %d pairs of %d x %d exceed one call", who, n, width, height); return SUO_ERR_ARG; }
    for (int i = 0; i < n; ++i) {
        if (image_index[i] < 0 || image_index[i] >= n_images) { suo_set_error("%s: image_index[%d]=%d out of range", who, i, image_index[i]); return SUO_ERR_ARG; }
        for (int e = 0; e < 9; ++e)
            if (!std::isfinite(K[(size_t)i * 9 + e])) { suo_set_error("%s: camera matrix %d is not finite", who, i); return SUO_ERR_ARG; }
    }
    return SUO_OK;
}

// The call's staged arguments and counters go into the scratch block (pinned host + device), the test images into a device-only buffer of their own;
// img / rbox are on the device already.  Caller holds db->mu.
static int vsd_run_locked(MeshDb* db, int n, int width, int height, const float* img_dev, const int* r_est, const int* r_gt, const int* rbox_dev, int n_images,
                          const float* depth_test, const int* image_index, const double* K, double delta, int n_taus, const double* taus, int normalized,
                          const double* diameter, double* errors, long long* counts) {
    const int nc = 2 + n_taus;
    const size_t hw = (size_t)height * width;
    // staged: K[n][9] | taus[n_taus] | diam[n] | image_index[n] | r_est[n] | r_gt[n]   then written by the device: counts[n][nc]
    const size_t o_k = 0, o_tau = (size_t)n * 72, o_diam = o_tau + (size_t)n_taus * 8, o_ii = o_diam + (size_t)n * 8, o_re = o_ii + (size_t)n * 4, o_rg = o_re + (size_t)n * 4;
    const size_t staged = (o_rg + (size_t)n * 4 + 15) & ~(size_t)15;
    const size_t o_cnt = staged, total = o_cnt + (size_t)n * nc * 8, test_bytes = (size_t)n_images * hw * 4;
    int rc;
    if ((rc = ensure_scratch(db, total))) return rc;
    if ((rc = grow_buffer(&db->test_dev, nullptr, &db->test_cap, test_bytes))) return rc;
    memcpy(db->scratch_host + o_k, K, (size_t)n * 72);
    memcpy(db->scratch_host + o_tau, taus, (size_t)n_taus * 8);
    double* dh = (double*)(db->scratch_host + o_diam);
    for (int i = 0; i < n; ++i) dh[i] = normalized ? diameter[i] : 1.0;
    memcpy(db->scratch_host + o_ii, image_index, (size_t)n * 4);
    memcpy(db->scratch_host + o_re, r_est, (size_t)n * 4);
    memcpy(db->scratch_host + o_rg, r_gt, (size_t)n * 4);
    SUO_HIP_CHECK(hipMemcpyAsync(db->scratch_dev, db->scratch_host, staged, hipMemcpyHostToDevice, db->stream));
    SUO_HIP_CHECK(hipMemsetAsync(db->scratch_dev + o_cnt, 0, (size_t)n * nc * 8, db->stream));
    SUO_HIP_CHECK(hipMemcpyAsync(db->test_dev, depth_test, test_bytes, hipMemcpyHostToDevice, db->stream));
    VsdArgs a;
    a.img = img_dev; a.rbox = rbox_dev;
    a.r_est = (const int*)(db->scratch_dev + o_re); a.r_gt = (const int*)(db->scratch_dev + o_rg);
    a.test = (const float*)db->test_dev; a.image_index = (const int*)(db->scratch_dev + o_ii);
    a.K = (const double*)(db->scratch_dev + o_k); a.taus = (const double*)(db->scratch_dev + o_tau); a.diam = (const double*)(db->scratch_dev + o_diam);
    a.counts = (unsigned long long*)(db->scratch_dev + o_cnt);
    a.delta = (float)delta; a.n_taus = n_taus; a.normalized = normalized; a.w = width; a.h = height;
    a.tiles_x = (width + VS_TILE - 1) / VS_TILE;
    const int tiles = a.tiles_x * ((height + VS_TILE - 1) / VS_TILE);
    hipLaunchKernelGGL(vsd_kernel, dim3(tiles, n), dim3(VS_BLOCK), 0, db->stream, a);
    SUO_HIP_CHECK(hipGetLastError());
    SUO_HIP_CHECK(hipMemcpyAsync(db->scratch_host + o_cnt, db->scratch_dev + o_cnt, (size_t)n * nc * 8, hipMemcpyDeviceToHost, db->stream));
    SUO_HIP_CHECK(hipStreamSynchronize(db->stream));
    const long long* c = (const long long*)(db->scratch_host + o_cnt);
    for (int i = 0; i < n; ++i) {
        const long long uni = c[(size_t)i * nc], inter = c[(size_t)i * nc + 1];
        for (int t = 0; t < n_taus; ++t)
            errors[(size_t)i * n_taus + t] = uni == 0 ? 1.0 : (double)(c[(size_t)i * nc + 2 + t] + (uni - inter)) / (double)uni;
        if (counts) memcpy(counts + (size_t)i * nc, c + (size_t)i * nc, (size_t)nc * 8);
    }
    return SUO_OK;
}

// suo_vsd_from_depth has no mesh database: one context of its own holds the stream and the scratch
static MeshDb* vsd_ctx() {
    static MeshDb* ctx = [] {
        MeshDb* d = new MeshDb();
        if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) { delete d; d = nullptr; }
        return d;
    }();
    return ctx;
}

}  // namespace suo

using namespace suo;

extern "C" int suo_vsd_from_depth(int n, int width, int height, const float* depth_est, const float* depth_gt, int n_images, const float* depth_test,
                                  const int* image_index, const double* K, double delta, int n_taus, const double* taus, int normalized_by_diameter,
                                  const double* diameter, double* errors, long long* counts) {
    int rc;
    if ((rc = check_vsd_args("suo_vsd_from_depth", n, width, height, n_images, depth_test, image_index, K, delta, n_taus, taus, normalized_by_diameter, diameter, errors)))
        return rc;
    if (n > 0 && (!depth_est || !depth_gt)) { suo_set_error("suo_vsd_from_depth: bad argument"); return SUO_ERR_ARG; }
    if (n == 0) return SUO_OK;
    MeshDb* db = vsd_ctx();
    if (!db) { suo_set_error("suo_vsd_from_depth: no stream"); return SUO_ERR_HIP; }
    std::lock_guard<std::mutex> lk(db->mu);
    const size_t bytes = (size_t)n * height * width * sizeof(float);
    if ((rc = grow_buffer(&db->img_dev, nullptr, &db->img_cap, 2 * bytes))) return rc;
    SUO_HIP_CHECK(hipMemcpyAsync(db->img_dev, depth_est, bytes, hipMemcpyHostToDevice, db->stream));
    SUO_HIP_CHECK(hipMemcpyAsync(db->img_dev + bytes, depth_gt, bytes, hipMemcpyHostToDevice, db->stream));
    std::vector<int> re(n), rg(n);
    for (int i = 0; i < n; ++i) { re[i] = i; rg[i] = n + i; }
    return vsd_run_locked(db, n, width, height, (const float*)db->img_dev, re.data(), rg.data(), nullptr, n_images, depth_test, image_index, K, delta, n_taus, taus,
                          normalized_by_diameter, diameter, errors, counts);
}

extern "C" int suo_pose_errors_vsd(void* h, int n, const int* model_index, const double* T_est, const double* T_gt, const double* K, int width, int height,
                                   int n_images, const float* depth_test, const int* image_index, double delta, int n_taus, const double* taus,
                                   int normalized_by_diameter, const double* diameter, double* errors, long long* counts) {
    MeshDb* db = (MeshDb*)h;
    if (!db) { suo_set_error("suo_pose_errors_vsd: bad argument"); return SUO_ERR_ARG; }
    int rc;
    if ((rc = check_vsd_args("suo_pose_errors_vsd", n, width, height, n_images, depth_test, image_index, K, delta, n_taus, taus, normalized_by_diameter, diameter, errors)))
        return rc;
    std::lock_guard<std::mutex> lk(db->mu);
    if ((rc = check_render_args("suo_pose_errors_vsd", db, n, model_index, T_est, K, width, height))) return rc;
    if ((rc = check_render_args("suo_pose_errors_vsd", db, n, model_index, T_gt, K, width, height))) return rc;
    if (n == 0) return SUO_OK;
    // the renders of the call, each (model, pose, fx, fy, cx, cy) once: the ground truths repeat
    struct Key {
        int m; double v[16];
        bool operator<(const Key& o) const { return m != o.m ? m < o.m : memcmp(v, o.v, sizeof(v)) < 0; }
    };
    std::map<Key, int> seen;
    std::vector<int> models, re(n), rg(n);
    std::vector<double> Ts, Ks;
    auto render_of = [&](int i, const double* T) {
        Key k;
        k.m = model_index[i];
        memcpy(k.v, T + (size_t)i * 12, 96);
        k.v[12] = K[(size_t)i * 9]; k.v[13] = K[(size_t)i * 9 + 4]; k.v[14] = K[(size_t)i * 9 + 2]; k.v[15] = K[(size_t)i * 9 + 5];
        auto it = seen.find(k);
        if (it != seen.end()) return it->second;
        const int r = (int)models.size();
        seen.emplace(k, r);
        models.push_back(k.m);
        Ts.insert(Ts.end(), T + (size_t)i * 12, T + (size_t)i * 12 + 12);
        Ks.insert(Ks.end(), K + (size_t)i * 9, K + (size_t)i * 9 + 9);
        return r;
    };
    for (int i = 0; i < n; ++i) { re[i] = render_of(i, T_est); rg[i] = render_of(i, T_gt); }
    if (models.size() > 65535) { suo_set_error("suo_pose_errors_vsd: %zu renders exceed one call", models.size()); return SUO_ERR_ARG; }
    float* img = nullptr; int* rbox = nullptr;
    if ((rc = render_depth_locked(db, (int)models.size(), models.data(), Ts.data(), Ks.data(), width, height, &img, &rbox))) return rc;
    return vsd_run_locked(db, n, width, height, img, re.data(), rg.data(), rbox, n_images, depth_test, image_index, K, delta, n_taus, taus, normalized_by_diameter,
                          diameter, errors, counts);
}
