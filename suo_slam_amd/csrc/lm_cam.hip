// Camera tracking as ONE wave: the LM algorithm of csrc/lm.hip specialised to "one free camera, every object fixed".
//
// ObjectSLAM runs this problem once per view (optimize(curr_only=True), /root/reference/lib/object_slam.py:444,703-930:
// the current camera against the mapped objects, its = [10,10,10,10]).  The unknown is a single 6-vector, so there is
// nothing to eliminate and nothing to share between workgroup waves -- yet the general kernel spends 1.6 ms on it: ~45
// trials of ~35 us, each a sequence of workgroup-wide phases (pair blocks, gathers, block solves) with barriers and LDS
// reductions between them and most of its 256 threads idle.  Here a 64-lane wave owns the problem:
//   * every lane linearises its edges (same edge_pass_partial as the general kernel) and adds their J^T W J / J^T W r
//     contributions to 27 registers; a shuffle tree leaves the 6x6 system in every lane,
//   * every lane solves it (identical instruction stream -> identical result) -- no broadcast,
//   * lane 0 applies / restores the pose; the only synchronisation is the memory fence of a one-wave workgroup barrier.
// Same rounds / robust-kernel schedule / lambda schedule / re-classification as csrc/lm.hip; only the summation order of
// H, b and chi2 differs (rounding level).  Many problems run as independent one-wave workgroups.
#include "lm_device.h"
#include "lm_launch.h"

namespace suo {

__global__ __launch_bounds__(64) void lm_cam_kernel(const LmProblem* __restrict__ problems) {
    const LmProblem& P = problems[blockIdx.x];
    const int lane = threadIdx.x;
    int c0 = 0;                                                  // the free camera (the launcher checked there is exactly one)
    for (int c = 0; c < P.n_cam; ++c) if (!P.cam_fixed[c]) c0 = c;
    for (int c = lane; c < P.n_cam; c += 64) pose_from_T(P.cam_T + 12 * c, P.cam[c]);
    for (int o = lane; o < P.n_obj; o += 64) pose_from_T(P.obj_T + 12 * o, P.obj[o]);
    for (int e = lane; e < P.n_edge; e += 64) P.level[e] = 0;
    __syncthreads();                                             // one wave: no waiting, just the fence

    auto classify = [&]() -> int {                               // object_slam.py:848-866 / 877-896
        double good = 0;
        for (int e = lane; e < P.n_edge; e += 64) {
            double er[2];
            edge_error(P, e, er, nullptr, nullptr);
            const double c2 = edge_chi2(P, e, er);
            P.edge_chi2[e] = c2;
            if (c2 > P.chi2_thr) { P.level[e] = 1; P.edge_inlier[e] = 0; }
            else { P.level[e] = 0; P.edge_inlier[e] = 1; good += 1; }
        }
        return (int)wsum(good);
    };
    double h[27], x[6];                                          // H (21, packed upper) and b (6) of the camera; the trial's step
    Pose bak;
    const LmCounters n = lm_run_rounds<true>(
        P,
        [&]() -> int { return P.init_with_outliers ? P.n_edge : classify(); },
        [&]() -> bool {
            double nact = 0;
            for (int e = lane; e < P.n_edge; e += 64) nact += edge_active(P, e) ? 1.0 : 0.0;
            return wsum(nact) > 0;
        },
        [&](bool robust_on, int it, double& max_diag) -> double {      // errors, chi2, Jacobians; the camera's system
            const double currentChi = wsum(edge_pass_partial(P, 0, P.n_edge, robust_on, true, lane, 64));
#pragma unroll
            for (int k = 0; k < 27; ++k) h[k] = 0;
            for (int e = lane; e < P.n_edge; e += 64) {          // this lane's own Jacobians (written just above)
                if (!edge_active(P, e)) continue;
                const double* J = P.jac + 29 * (size_t)e;
                accumulate_jtwj<false>(J, J[24], J[25], J[26], J[27], J[28], h);
            }
#pragma unroll
            for (int k = 0; k < 27; ++k) h[k] = wsum(h[k]);
            if (it == 0) max_diag = sym21_max_abs_diag(h);
            return currentChi;
        },
        [&](double lambda, bool robust_on) -> LmTrial {
            bak = P.cam[c0];                                     // push()
            double A[36], b6[6];
#pragma unroll
            for (int d = 0; d < 6; ++d) x[d] = 0;
            sym21_to_system(h, lambda, A, b6);
            const bool ok2 = spd_solve6(A, b6, x);               // every lane, identically
            if (ok2 && lane == 0) pose_oplus(P.cam[c0], x);
            __syncthreads();
            const double tempChi = wsum(edge_pass_partial(P, 0, P.n_edge, robust_on, false, lane, 64));
            double sc = 0;                                        // computeScale: sum x (lambda x + b)
            if (ok2)
                for (int d = 0; d < 6; ++d) sc += x[d] * (lambda * x[d] + h[21 + d]);
            return {tempChi, sc, ok2};
        },
        [&]() {},                                                // update(x) is already in memory
        [&]() {
            __syncthreads();                                     // every lane has read the trial pose
            if (lane == 0) P.cam[c0] = bak;                      // pop()
            __syncthreads();
        },
        [&]() -> int {
            __syncthreads();
            const int good = classify();
            __syncthreads();
            return good;
        });
    for (int c = lane; c < P.n_cam; c += 64) pose_to_T(P.cam[c], P.cam_T + 12 * c);
    for (int o = lane; o < P.n_obj; o += 64) pose_to_T(P.obj[o], P.obj_T + 12 * o);
    if (lane == 0) n.store(P.stats);
}

// problems with exactly one free camera and no free object (the caller checks), one wave each
int launch_lm_cam(const void* problems_dev, int n_problems, hipStream_t s) {
    if (n_problems <= 0) return SUO_OK;
    hipLaunchKernelGGL(lm_cam_kernel, dim3(n_problems), dim3(64), 0, s, (const LmProblem*)problems_dev);
    SUO_HIP_CHECK(hipGetLastError());
    return SUO_OK;
}

}  // namespace suo
