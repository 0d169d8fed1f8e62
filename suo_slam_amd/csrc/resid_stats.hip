// Per-edge leverages, studentised residuals and the chi2 scale of a bundle-adjustment problem at the state it holds (include/suo_hip.h: suo_residual_statistics).
//
// Runs BEHIND the pose-covariance kernels of the problem's cov_form and the pair kernel (csrc/pose_cov.hip, csrc/pose_cov_graph.hip), on their stream: cam_cov / obj_cov
// hold Sigma_cc / Sigma_oo of every vertex, and for cov_form >= 2 cov_cross [36 p] holds Sigma_co of the problem's own pair p (rows the camera) -- the host entry
// asks for exactly those pairs (csrc/cov_stage.hip).  Forms 0 and 1 couple nothing: Sigma_co = 0 and no pair was asked for.
//
//   rs_edge_kernel     a thread per (sorted) edge, 64 consecutive edges per wave.  v and J = [Jc Jo] come from lm_device.h (edge_error_at, edge_jacobian: the functions the
//                      Hessian was built from), at Poses made from cam_T / obj_T the way pc_assemble_blocks makes them.  Edges are sorted by pair, so a wave's edges span a
//                      contiguous range of pairs: the wave stages the three 6x6 blocks of RS_CHUNK pairs at a time in LDS (108 doubles a pair, each read from memory once
//                      per wave) and the lanes of a pair read them from there.  Results go to the CALLER's edge index (RsProblem::order).
//   rs_reduce_kernel   per problem one workgroup for the summary and one wave per vertex (four to a workgroup).  A vertex's wave walks the vertex's edges in ascending
//                      caller index (RsProblem::vedge): lane l adds the counted ones among positions l, l + 64, ..., the 64 partials meet in wsum's fixed tree -- a
//                      shape that depends on the vertex's edge list alone (one thread walking the list alone cost 185 us on 60 x 8: a dependent load per edge).
//                      The problem's sums: leaf l = edges [16 l, 16 l + 16) added in ascending index, thread t adds leaves t, t + 256, ... in that order, the 256
//                      partials meet in block_sum's fixed tree: a shape that depends on n_edge alone.  The same bits alone or in a batch, at any grid size.
// fp64, vector stores only, no atomics.
#include <algorithm>

#include "lm_device.h"
#include "lm_launch.h"

namespace suo {

static_assert(LM_THREADS == 256, "rs_edge_kernel: four waves of 64 edges; rs_reduce_kernel: 256 partials");

constexpr int RS_CHUNK = 8;             // pairs a wave holds in LDS at a time: 8 x 108 doubles = 6.75 KB per wave, 27 KB per workgroup
constexpr int RS_LEAF = 16;             // edges per leaf of the problem's sums
constexpr double RS_MIN_DET = 1e-9;     // the no-redundancy rule of include/suo_hip.h: part of the definition, not a tolerance

__global__ __launch_bounds__(LM_THREADS) void rs_edge_kernel(const LmProblem* __restrict__ problems, const RsProblem* __restrict__ rs) {
    const LmProblem& P = problems[blockIdx.x];
    const RsProblem& R = rs[blockIdx.x];
    __shared__ double blk[LM_THREADS / 64][RS_CHUNK][108];      // per pair: Sigma_cc | Sigma_oo | Sigma_co
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int k0 = blockIdx.y * LM_THREADS + wv * 64;
    if (k0 >= P.n_edge) return;                                 // the whole wave: the grid's tail, or a smaller problem of the batch (no workgroup barrier below)
    const bool valid = k0 + lane < P.n_edge;
    const int k = valid ? k0 + lane : P.n_edge - 1;             // the lanes past the end repeat the last edge and store nothing
    const int p = P.edge_pair[k];
    const int c = P.pair_cam[p], o = P.pair_obj[p];
    const bool cfix = P.cam_fixed[c] != 0, ofix = P.obj_fixed[o] != 0;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);

    Pose cam, obj;
    pose_from_T(P.cam_T + 12 * (size_t)c, cam);
    pose_from_T(P.obj_T + 12 * (size_t)o, obj);
    double v[2], pw[3], pc[3], J[24];
    edge_error_at(P, k, cam, obj, v, pw, pc);
    edge_jacobian(P, k, cam, pw, pc, J);
#pragma unroll
    for (int i = 0; i < 6; ++i) {                               // zero columns for a fixed vertex
        if (cfix) { J[i] = 0; J[6 + i] = 0; }
        if (ofix) { J[12 + i] = 0; J[18 + i] = 0; }
    }
    const double* I = P.edge_info + 3 * (size_t)k;
    const double I0 = I[0], I1 = I[1], I2 = I[2];
    const double chi2 = edge_chi2(P, k, v);
    const bool counted = P.edge_inlier[k] != 0 && !(cfix && ofix);

    // ---- w0 / w1 = Sigma_e J^T (12 x 2), the pairs of this wave's edges RS_CHUNK at a time through LDS ----------------------------------------------
    const int p_first = P.edge_pair[k0], p_last = P.edge_pair[min(k0 + 63, P.n_edge - 1)];
    const bool coupled = P.cov_form >= 2 && P.n_cpair == P.n_pair;       // the request is the problem's own pair list (csrc/pose_cov_api.hip)
    double w0[12], w1[12];
    bool nanv = false;
#pragma unroll
    for (int i = 0; i < 12; ++i) { w0[i] = 0; w1[i] = 0; }
    for (int pb = p_first; pb <= p_last; pb += RS_CHUNK) {
        const int n = min(RS_CHUNK, p_last - pb + 1);
        for (int i = lane; i < n * 108; i += 64) {
            const int j = i / 108, r = i - j * 108, pp = pb + j;
            double val;
            if (r < 36) val = P.cam_cov[36 * (size_t)P.pair_cam[pp] + r];
            else if (r < 72) val = P.obj_cov[36 * (size_t)P.pair_obj[pp] + (r - 36)];
            else val = coupled ? P.cov_cross[36 * (size_t)pp + (r - 72)] : 0.0;
            blk[wv][j][r] = val;
        }
        __builtin_amdgcn_wave_barrier();
        if (p >= pb && p < pb + n) {
            const double* Scc = blk[wv][p - pb];
            const double* Soo = Scc + 36;
            const double* Sco = Scc + 72;
            nanv = isnan(Scc[0]) || isnan(Soo[0]);
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                double a0 = 0, a1 = 0, b0 = 0, b1 = 0;
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    a0 += Scc[6 * i + j] * J[j];       a1 += Scc[6 * i + j] * J[6 + j];
                    b0 += Sco[6 * j + i] * J[j];       b1 += Sco[6 * j + i] * J[6 + j];
                }
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    a0 += Sco[6 * i + j] * J[12 + j];  a1 += Sco[6 * i + j] * J[18 + j];
                    b0 += Soo[6 * i + j] * J[12 + j];  b1 += Soo[6 * i + j] * J[18 + j];
                }
                w0[i] = a0; w1[i] = a1; w0[6 + i] = b0; w1[6 + i] = b1;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    // ---- P = J Sigma_e J^T, lev = tr(P Omega), R = I + s P Omega, t = (Omega v)^T R^-1 v -----------------------------------------------------------
    double pxx = 0, pyy = 0, pxy_a = 0, pxy_b = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        pxx += J[i] * w0[i];        pyy += J[6 + i] * w1[i];
        pxy_a += J[i] * w1[i];      pxy_b += J[6 + i] * w0[i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        pxx += J[12 + i] * w0[6 + i];       pyy += J[18 + i] * w1[6 + i];
        pxy_a += J[12 + i] * w1[6 + i];     pxy_b += J[18 + i] * w0[6 + i];
    }
    const double pxy = 0.5 * (pxy_a + pxy_b);
    const double a00 = pxx * I0 + pxy * I1, a01 = pxx * I1 + pxy * I2, a10 = pxy * I0 + pyy * I1, a11 = pxy * I1 + pyy * I2;     // P Omega
    const double lev = a00 + a11;
    const double s = counted ? -1.0 : 1.0;
    const double r00 = 1.0 + s * a00, r01 = s * a01, r10 = s * a10, r11 = 1.0 + s * a11;
    const double det = r00 * r11 - r01 * r10;
    const bool nored = !nanv && (!(det > RS_MIN_DET) || !(r00 > 0) || !(r11 > 0));
    const double u0 = I0 * v[0] + I1 * v[1], u1 = I1 * v[0] + I2 * v[1];
    const double t = (u0 * (r11 * v[0] - r01 * v[1]) + u1 * (r00 * v[1] - r10 * v[0])) / det;
    if (valid) {
        const size_t e = (size_t)R.order[k];
        R.chi2[e] = chi2;
        R.pcov[3 * e] = nanv ? nan : pxx;
        R.pcov[3 * e + 1] = nanv ? nan : pxy;
        R.pcov[3 * e + 2] = nanv ? nan : pyy;
        R.lev[e] = nanv ? nan : lev;
        R.t[e] = (nanv || nored) ? nan : t;
        R.flag[e] = (uint8_t)((counted ? RS_COUNTED : 0) | (nanv ? RS_NAN : 0) | (nored ? RS_NORED : 0));
    }
}

__global__ __launch_bounds__(LM_THREADS) void rs_reduce_kernel(const LmProblem* __restrict__ problems, const RsProblem* __restrict__ rs) {
    const LmProblem& P = problems[blockIdx.x];
    const RsProblem& R = rs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, V = P.n_cam + P.n_obj, E = P.n_edge;
    if (blockIdx.y > 0) {
        // ---- a wave per vertex: (count, sum chi2, sum 2 - lev) over its counted edges.  Lane l adds positions l, l + 64, ... of the vertex's list (ascending caller
        //      index) in that order, the 64 partials meet in wsum's fixed tree: the shape depends on the vertex's edge list alone -----------------------------------
        const int vtx = (blockIdx.y - 1) * (LM_THREADS / 64) + wv;
        if (vtx >= V) return;                                   // the whole wave (no workgroup barrier in this branch)
        double cnt = 0, sc = 0, sr = 0;
        const int i1 = R.vptr[vtx + 1];
        for (int i = R.vptr[vtx] + lane; i < i1; i += 64) {
            const int e = R.vedge[i];
            const bool on = (R.flag[e] & RS_COUNTED) != 0;
            const double x = R.chi2[e], r = 2.0 - R.lev[e];
            if (on) { cnt += 1; sc += x; sr += r; }
        }
        cnt = wsum(cnt); sc = wsum(sc); sr = wsum(sr);
        if (lane < 3) R.vstat[3 * (size_t)vtx + lane] = lane == 0 ? cnt : (lane == 1 ? sc : sr);
        return;
    }
    __shared__ double red[LM_THREADS / 64];
    // ---- the rows of H: six per free vertex that a counted edge reaches (a thread per vertex looks no further than the first one; integers: no order to fix) --------
    double rows = 0;
    for (int vtx = tid; vtx < V; vtx += LM_THREADS) {
        if (vtx < P.n_cam ? P.cam_fixed[vtx] != 0 : P.obj_fixed[vtx - P.n_cam] != 0) continue;
        bool reached = false;
        for (int i = R.vptr[vtx]; i < R.vptr[vtx + 1] && !reached; ++i) reached = (R.flag[R.vedge[i]] & RS_COUNTED) != 0;
        if (reached) rows += 6;
    }
    // ---- the problem's sums: leaves of RS_LEAF edges, a thread's leaves in ascending order, then block_sum's tree (counts are exact in a double) ----------------
    double m = 0, n_nan = 0, n_nored = 0, m_nan = 0, s_chi2 = 0, s_lev = 0;
    for (int e0 = tid * RS_LEAF; e0 < E; e0 += LM_THREADS * RS_LEAF) {
        double lc = 0, ll = 0;
        const int e1 = min(E, e0 + RS_LEAF);
        for (int e = e0; e < e1; ++e) {
            const int f = R.flag[e];
            const double x = R.chi2[e], l = R.lev[e];
            if (f & RS_COUNTED) { m += 1; lc += x; ll += l; if (f & RS_NAN) m_nan += 1; }
            if (f & RS_NAN) n_nan += 1;
            if (f & RS_NORED) n_nored += 1;
        }
        s_chi2 += lc;
        s_lev += ll;
    }
    rows = block_sum(rows, red);
    m = block_sum(m, red);
    n_nan = block_sum(n_nan, red);
    n_nored = block_sum(n_nored, red);
    m_nan = block_sum(m_nan, red);
    s_chi2 = block_sum(s_chi2, red);
    s_lev = block_sum(s_lev, red);
    if (tid == 0) {
        const double dof = 2 * m - rows;
        R.summary[0] = m;
        R.summary[1] = rows;
        R.summary[2] = s_chi2;
        R.summary[3] = s_lev;
        R.summary[4] = dof;
        R.summary[5] = (dof > 0 && m_nan == 0) ? s_chi2 / dof : __longlong_as_double(0x7ff8000000000000ll);
        R.status[0] = (int)n_nan;
        R.status[1] = (int)n_nored;
    }
}

int launch_resid_stats(const void* problems_dev, const void* rs_dev, int n_problems, int max_edges, int max_vertices, hipStream_t s) {
    if (n_problems <= 0) return SUO_OK;
    const LmProblem* P = (const LmProblem*)problems_dev;
    const RsProblem* R = (const RsProblem*)rs_dev;
    const int ny = std::max(1, (max_edges + LM_THREADS - 1) / LM_THREADS), nv = (std::max(max_vertices, 0) + LM_THREADS / 64 - 1) / (LM_THREADS / 64);
    hipLaunchKernelGGL(rs_edge_kernel, dim3(n_problems, ny), dim3(LM_THREADS), 0, s, P, R);
    hipLaunchKernelGGL(rs_reduce_kernel, dim3(n_problems, 1 + nv), dim3(LM_THREADS), 0, s, P, R);      // y = 0: the problem's sums; y >= 1: four vertices each
    SUO_HIP_CHECK(hipGetLastError());
    return SUO_OK;
}

}  // namespace suo
