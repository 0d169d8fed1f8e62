// Covariance of a tracked camera with the map's uncertainty carried in (include/suo_hip.h: suo_tracking_covariances): the Schmidt consider covariance
//
//   P_c = Hcc^-1 + G Sigma_OO G^T,   G = Hcc^-1 [B_c1 ... B_cn],   B_co = sum over the counted edges of (c, o) of J_c^T Omega J_o
//
// of the camera-tracking graph, every object fixed at its map pose.  Hcc^-1 is NOT recomputed here: pose_cov_diag_kernel (csrc/pose_cov.hip, cov_form 1) runs in
// front on the same staged problem and leaves it in LmProblem::cam_cov -- zeros for a fixed camera, NaNs for a free camera without a counted edge or with a bad
// pivot -- so fixed_map_cov has suo_pose_covariances' bits.  The host (csrc/track_cov_api.hip) has taken the edges of the objects that are not in the map out of
// edge_inlier, mirrored Sigma_OO from its upper triangle and zeroed the rows and columns of those objects.
//
// One workgroup of 256 threads per (problem, camera), five phases with a barrier between them; ns = 6 n_obj <= 384:
//   B   a thread per object: J_c and J_o of lm_device.h (edge_jacobian: J_o is the derivative by the FIXED object's perturbation), the pair's edges in ascending
//       edge index, 36 sums in registers; zeros where the camera does not see the object
//   G   = Hcc^-1 B, a thread per entry                                                   6 x ns in LDS (18 KB at the cap)
//   Z   = G Sigma_OO, a thread per column, ascending k; lane j reads Sigma[k][j]: a row of Sigma is contiguous along the output column, and Sigma is read once
//       per camera, from device memory                                                   6 x ns in LDS, over B
//   P   = Hcc^-1 + Z G^T: four threads per entry take every fourth column, (p0 + p1) + (p2 + p3), then 0.5 (P + P^T)
//   cross [o] = -Z[:, o] and rel [o] = P + A Soo A^T + X A^T + A X^T, X = cross [o], A = Ad(T_c): a thread per (object, entry); rel is the mean of the (r, c) and
//       (c, r) evaluations, which the two threads form from the same two numbers
// LDS: 2 x 18 KB + 2 KB, static; at 37 KB four workgroups fit the CU's 160 KB, and a tracking call has one camera: the kernel is latency, not occupancy.
// Nothing here needs the matrix pipe: 6 x 384 x 384 multiply-adds per camera at the cap.  Vector stores only, no atomics, every sum in a fixed order.
#include "lm_device.h"
#include "lm_launch.h"
#include "pose_cov_device.h"
#include "track_cov.h"

namespace suo {

constexpr int TC_THREADS = 256;
constexpr int TC_NS = 6 * POSE_COV_GRAPH_MAX_OBJ;

__global__ __launch_bounds__(TC_THREADS) void track_cov_kernel(const LmProblem* __restrict__ problems, const TcProblem* __restrict__ tcs, int max_cam) {
    const int prob = blockIdx.x / max_cam, c = blockIdx.x - prob * max_cam;
    const LmProblem& P = problems[prob];
    const TcProblem& T = tcs[prob];
    if (c >= P.n_cam) return;
    __shared__ double G[6 * TC_NS], Z[6 * TC_NS], Hi[36], Praw[36], Pm[36], part[4 * 36];
    const int tid = threadIdx.x, n = P.n_obj, ns = 6 * n;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double* fm = P.cam_cov + 36 * (size_t)c;
    const bool fixed = P.cam_fixed[c] != 0;
    double* out_cov = T.cam_cov + 36 * (size_t)c;
    double* out_cross = T.cross + 36 * (size_t)c * n;
    double* out_rel = T.rel + 36 * (size_t)c * n;
    if (!fixed && isnan(fm[0])) {               // (the same in every thread) no counted edge or a bad pivot: every block of the camera
        if (tid < 36) out_cov[tid] = nan;
        for (int idx = tid; idx < 36 * n; idx += TC_THREADS) { out_cross[idx] = nan; out_rel[idx] = nan; }
        return;
    }
    if (tid < 36) Hi[tid] = fixed ? 0.0 : fm[tid];
    // ---- B into Z's LDS -----------------------------------------------------------------------------------------------------------
    for (int o = tid; o < n; o += TC_THREADS) {
        double b[36];
#pragma unroll
        for (int i = 0; i < 36; ++i) b[i] = 0;
        const int p = P.cam_obj_pair[(size_t)c * n + o];
        if (!fixed && p >= 0 && T.in_map[o]) {
            Pose cam, obj;
            pose_from_T(P.cam_T + 12 * (size_t)c, cam);
            pose_from_T(P.obj_T + 12 * (size_t)o, obj);
            for (int e = P.pair_start[p]; e < P.pair_start[p + 1]; ++e) {
                if (!P.edge_inlier[e]) continue;
                double er[2], pw[3], pc[3], J[24];
                edge_error_at(P, e, cam, obj, er, pw, pc);
                edge_jacobian(P, e, cam, pw, pc, J);
                const double* I = P.edge_info + 3 * (size_t)e;
                double w0[6], w1[6];
#pragma unroll
                for (int j = 0; j < 6; ++j) { w0[j] = I[0] * J[12 + j] + I[1] * J[18 + j]; w1[j] = I[1] * J[12 + j] + I[2] * J[18 + j]; }
#pragma unroll
                for (int r = 0; r < 6; ++r)
#pragma unroll
                    for (int j = 0; j < 6; ++j) b[6 * r + j] += J[r] * w0[j] + J[6 + r] * w1[j];
            }
        }
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int j = 0; j < 6; ++j) Z[r * ns + 6 * o + j] = b[6 * r + j];
    }
    __syncthreads();
    // ---- G = Hcc^-1 B ---------------------------------------------------------------------------------------------------------------
    for (int idx = tid; idx < 6 * ns; idx += TC_THREADS) {
        const int r = idx / ns, k = idx - r * ns;
        double acc = 0;
#pragma unroll
        for (int m = 0; m < 6; ++m) acc += Hi[6 * r + m] * Z[m * ns + k];
        G[idx] = acc;
    }
    __syncthreads();
    // ---- Z = G Sigma ------------------------------------------------------------------------------------------------------------------
    for (int j = tid; j < ns; j += TC_THREADS) {
        double acc[6] = {0, 0, 0, 0, 0, 0};
        for (int k = 0; k < ns; ++k) {
            const double s = T.sigma[(size_t)k * ns + j];
#pragma unroll
            for (int r = 0; r < 6; ++r) acc[r] += G[r * ns + k] * s;
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) Z[r * ns + j] = acc[r];
    }
    __syncthreads();
    // ---- P = Hcc^-1 + Z G^T -------------------------------------------------------------------------------------------------------------
    if (tid < 4 * 36) {
        const int ent = tid >> 2, q = tid & 3, r = ent / 6, c2 = ent - r * 6;
        double acc = 0;
        for (int j = q; j < ns; j += 4) acc += Z[r * ns + j] * G[c2 * ns + j];
        part[tid] = acc;
    }
    __syncthreads();
    if (tid < 36) Praw[tid] = Hi[tid] + ((part[4 * tid] + part[4 * tid + 1]) + (part[4 * tid + 2] + part[4 * tid + 3]));
    __syncthreads();
    if (tid < 36) {
        const int r = tid / 6, c2 = tid - r * 6;
        const double v = 0.5 * (Praw[tid] + Praw[6 * c2 + r]);
        Pm[tid] = v;
        out_cov[tid] = v;
    }
    __syncthreads();
    // ---- cross and rel of every object ---------------------------------------------------------------------------------------------------
    const double* Tc = P.cam_T + 12 * (size_t)c;
    for (int idx = tid; idx < 36 * n; idx += TC_THREADS) {
        const int o = idx / 36, rc = idx - o * 36, r = rc / 6, c2 = rc - r * 6;
        if (!T.in_map[o]) { out_cross[idx] = nan; out_rel[idx] = nan; continue; }
        auto x = [&](int i, int j) { return 0.0 - Z[i * ns + 6 * o + j]; };
        out_cross[idx] = x(r, c2);
        double Ar[6], Ac[6];
        pc_ad_row(Tc, false, r, Ar);
        pc_ad_row(Tc, false, c2, Ac);
        const double* Soo = T.sigma + (size_t)(6 * o) * ns + 6 * o;
        // entry (i, j) of P + A Soo A^T + X A^T + A X^T from rows Ai, Aj of A
        auto entry = [&](int i, int j, const double (&Ai)[6], const double (&Aj)[6]) {
            double acc = Pm[6 * i + j];
            for (int k = 0; k < 6; ++k) {
                double row = 0;
                for (int l = 0; l < 6; ++l) row += Soo[(size_t)k * ns + l] * Aj[l];
                acc += Ai[k] * row;
            }
            double w1 = 0, w2 = 0;
            for (int k = 0; k < 6; ++k) { w1 += x(i, k) * Aj[k]; w2 += Ai[k] * x(j, k); }
            acc += w1;
            acc += w2;
            return acc;
        };
        out_rel[idx] = 0.5 * (entry(r, c2, Ar, Ac) + entry(c2, r, Ac, Ar));
    }
}

int launch_track_cov(const void* problems_dev, const void* tc_dev, int n_problems, int max_cam, int max_obj, hipStream_t s) {
    if (n_problems <= 0 || max_cam <= 0) return SUO_OK;
    if (max_obj > POSE_COV_GRAPH_MAX_OBJ) {
        suo_set_error("tracking covariances: %d objects (G and Z are sized for %d)", max_obj, POSE_COV_GRAPH_MAX_OBJ);
        return SUO_ERR_ARG;
    }
    hipLaunchKernelGGL(track_cov_kernel, dim3((unsigned)n_problems * (unsigned)max_cam), dim3(TC_THREADS), 0, s, (const LmProblem*)problems_dev, (const TcProblem*)tc_dev,
                       max_cam);
    SUO_HIP_CHECK(hipGetLastError());
    return SUO_OK;
}

}  // namespace suo
