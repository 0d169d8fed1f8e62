// Consistency of the reported uncertainties (include/suo_hip.h: suo_pose_nees, suo_keypoint_nees): the normalised estimation error squared of a pose under its
// 6x6 covariance and the chi2 of a keypoint under its 2x2 covariance.  fp64, no contraction, vector stores only, no atomics.
//
// Pose NEES of a pair (estimate T_est, ground truth T_gt, covariance Sigma) of model m:
//   s*     = the symmetry that attains the MSSD minimum min_s max_i |T_est p_i - T_gt S_s p_i|; on equal maxima the lowest index.  The P x S pass is
//            bop_errors_kernel's (csrc/eval_bop.hip), launched as it is; pose_nees_kernel reads its [n][S][2] block of merged squared maxima.  max, the merge and
//            the comparison are exact, so the pick does not depend on the launch shape.  A pair whose 3-D flag is set (a non-finite distance) gets -1.
//   T_ref  = T_gt S_s*:  R_ref = R_gt S_R,  t_ref = R_gt S_t + t_gt, in the operation order of eval_bop.hip (each entry (a0 b0 + a1 b1) + a2 b2).
//   xi     = log(T_est T_ref^-1) = [omega, upsilon], the inverse of the library's update T <- exp([omega, upsilon]) T (lm_device.h: pose_oplus):
//            D = T_est T_ref^-1:  R_D = R_est R_ref^T,  t_D = t_est - R_D t_ref;  unit quaternion (w >= 0, v) of R_D by R_to_q (lm_device.h);
//            omega = f v,  f = 2 atan2(|v|, w) / |v|  (|v|^2 < 1e-8: f = (2 / w)(1 - r / 3 + r^2 / 5), r = |v|^2 / w^2; the next term is < 1e-25),  theta = f |v| in [0, pi];
//            upsilon = V^-1 t_D = t_D - omega x t_D / 2 + k omega x (omega x t_D),  k = (1 - (theta / 2) cot(theta / 2)) / theta^2 with cot(theta / 2) = w / |v|;
//            theta^2 < 0.09: k = 1/12 + theta^2 / 720 + theta^4 / 30240 + ... (seven terms, the next is < 1e-17 relative).
//   NEES   = xi^T Sigma^-1 xi = |L^-1 xi|^2, Sigma = L L^T by Cholesky in registers (compile-time indices; the lower triangle of the row-major block is read),
//            one forward substitution, the six squares added in index order.  NaN for a block with a non-finite entry (all 36 are looked at) or a pivot that is
//            not positive (the 36 zeros of a fixed vertex), and for a pair with sym_index -1; nothing loops on a bad block.
// Shape.  One pair per 8-lane group, 32 pairs per 256-thread workgroup: the eight lanes share the scan over the symmetries (lane sub takes s = sub, sub + 8, ...;
// (value, index) pairs meet by three xor-shuffles inside the group, lexicographic order, so the result is the one of a serial scan), then every lane of the group
// carries the same ~100 doubles of the logarithm and the factorisation through the same operations and lane 0 stores.  A reporting path of thousands of pairs at
// most: the seven redundant lanes cost nothing that matters and no value crosses lanes after the pick.  Every sum has one order: two calls give the same bits and
// a pair in a batch has the bits it has alone.
//
// Keypoint chi2, one thread per keypoint of a ragged list of detections:
//   e = uv - pi(K, T_ref x),  pi = (K X)_xy / (K X)_z divided as given (a point behind the camera keeps its finite value),
//   chi2 = e^T C^-1 e = (c11 e0^2 - (c01 + c10) e0 e1 + c00 e1^2) / det C;  NaN when det C <= 0, a diagonal entry <= 0 or any input or the result is not finite.
#include <limits.h>
#include <math.h>

#include "eval_nees.h"
#include "lm_device.h"

namespace suo {

constexpr int NE_BLOCK = 256;                    // threads per workgroup
constexpr int NE_G = 8;                          // lanes per pair

__device__ __forceinline__ double ne_dot3(double a0, double b0, double a1, double b1, double a2, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

__global__ __launch_bounds__(NE_BLOCK) void pose_nees_kernel(PoseNeesArgs a) {
    const int gid = blockIdx.x * (NE_BLOCK / NE_G) + threadIdx.x / NE_G, sub = threadIdx.x % NE_G;
    const bool have = gid < a.n;
    const int z = have ? gid : a.n - 1;                       // (the groups past the last pair repeat it and store nothing: every lane takes the shuffles)
    const int m = a.model[z];
    const int s_begin = a.soff[m], S = a.soff[m + 1] - s_begin;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    // ---- the symmetry of the MSSD minimum, lowest index on ties
    double bv = INFINITY;
    int bi = INT_MAX;
    for (int s = sub; s < S; s += NE_G) {
        const double v = __longlong_as_double((long long)a.smax[((size_t)z * a.stride + s) * 2]);
        if (v < bv || bi == INT_MAX) { bv = v; bi = s; }
    }
#pragma unroll
    for (int o = 1; o < NE_G; o <<= 1) {
        const double ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    const bool bad = (a.flags[z] & 1u) != 0 || bi < 0 || bi >= S;
    const int sidx = bad ? 0 : bi;                            // S >= 1: a valid set to read whatever happens
    // ---- T_ref = T_gt S
    const double* Tg = a.Tg + (size_t)z * 12;
    const double* Te = a.Te + (size_t)z * 12;
    const double* Sy = a.sym + (size_t)(s_begin + sidx) * 12;
    double Tr[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) Tr[i * 4 + j] = ne_dot3(Tg[i * 4], Sy[j], Tg[i * 4 + 1], Sy[4 + j], Tg[i * 4 + 2], Sy[8 + j]);
        Tr[i * 4 + 3] = ne_dot3(Tg[i * 4], Sy[3], Tg[i * 4 + 1], Sy[7], Tg[i * 4 + 2], Sy[11]) + Tg[i * 4 + 3];
    }
    // ---- D = T_est T_ref^-1 and its logarithm
    double Rd[9], td[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Rd[i * 3 + j] = ne_dot3(Te[i * 4], Tr[j * 4], Te[i * 4 + 1], Tr[j * 4 + 1], Te[i * 4 + 2], Tr[j * 4 + 2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) td[i] = Te[i * 4 + 3] - ne_dot3(Rd[i * 3], Tr[3], Rd[i * 3 + 1], Tr[7], Rd[i * 3 + 2], Tr[11]);
    double q[4];
    R_to_q(Rd, q);
    const double w = q[0], n2 = (q[1] * q[1] + q[2] * q[2]) + q[3] * q[3];
    double f;
    if (n2 < 1e-8) {
        const double r = n2 / (w * w);
        f = (2.0 / w) * (1.0 - r / 3.0 + (r * r) / 5.0);
    } else {
        const double n = sqrt(n2);
        f = 2.0 * atan2(n, w) / n;
    }
    double xi[6];
    xi[0] = f * q[1]; xi[1] = f * q[2]; xi[2] = f * q[3];
    const double th2 = (f * f) * n2;
    double k;
    if (th2 < 0.09) {
        const double t = th2;
        k = 1.0 / 12.0 + t * (1.0 / 720.0 + t * (1.0 / 30240.0 + t * (1.0 / 1209600.0 + t * (1.0 / 47900160.0 + t * (691.0 / 1307674368000.0 + t * (1.0 / 74724249600.0))))));
    } else {
        k = (1.0 - 0.5 * f * w) / th2;                        // (theta / 2) cot(theta / 2) = (f |v| / 2) (w / |v|)
    }
    {
        const double wx = xi[0], wy = xi[1], wz = xi[2];
        const double cx = wy * td[2] - wz * td[1], cy = wz * td[0] - wx * td[2], cz = wx * td[1] - wy * td[0];       // omega x t
        const double ccx = wy * cz - wz * cy, ccy = wz * cx - wx * cz, ccz = wx * cy - wy * cx;                      // omega x (omega x t)
        xi[3] = (td[0] - 0.5 * cx) + k * ccx;
        xi[4] = (td[1] - 0.5 * cy) + k * ccy;
        xi[5] = (td[2] - 0.5 * cz) + k * ccz;
    }
    // ---- NEES through the Cholesky factor of the block
    const double* Cv = a.cov + (size_t)z * 36;
    double A[36];
    bool ok = true;
#pragma unroll
    for (int e = 0; e < 36; ++e) { A[e] = Cv[e]; ok &= isfinite(A[e]); }
    double L[6][6], y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double s = A[i * 6 + j];
#pragma unroll
            for (int c = 0; c < j; ++c) s -= L[i][c] * L[j][c];
            if (i == j) {
                if (!(s > 0) || !isfinite(s)) ok = false;
                L[i][i] = sqrt(ok ? s : 1.0);
            } else {
                L[i][j] = s / L[j][j];
            }
        }
        double s = xi[i];
#pragma unroll
        for (int c = 0; c < i; ++c) s -= L[i][c] * y[c];
        y[i] = s / L[i][i];
    }
    double nees = y[0] * y[0];
#pragma unroll
    for (int i = 1; i < 6; ++i) nees += y[i] * y[i];
    if (bad || !ok || !isfinite(nees)) nees = nan;
    if (have && sub == 0) {
        a.nees[z] = nees;
        a.sym_index[z] = bad ? -1 : bi;
#pragma unroll
        for (int i = 0; i < 6; ++i) a.xi[(size_t)z * 6 + i] = bad ? nan : xi[i];
#pragma unroll
        for (int i = 0; i < 12; ++i) a.Tref[(size_t)z * 12 + i] = bad ? nan : Tr[i];
    }
}

__global__ __launch_bounds__(NE_BLOCK) void keypoint_nees_kernel(KpNeesArgs a) {
    const int i = blockIdx.x * NE_BLOCK + threadIdx.x;
    if (i >= a.total) return;
    const int d = a.det[i];
    const double* T = a.T + (size_t)d * 12;
    const double* K = a.K + (size_t)d * 9;
    const double x = a.pts[(size_t)i * 3], yv = a.pts[(size_t)i * 3 + 1], zv = a.pts[(size_t)i * 3 + 2];
    const double X = ne_dot3(T[0], x, T[1], yv, T[2], zv) + T[3];
    const double Y = ne_dot3(T[4], x, T[5], yv, T[6], zv) + T[7];
    const double Z = ne_dot3(T[8], x, T[9], yv, T[10], zv) + T[11];
    const double hu = ne_dot3(K[0], X, K[1], Y, K[2], Z), hv = ne_dot3(K[3], X, K[4], Y, K[5], Z), hw = ne_dot3(K[6], X, K[7], Y, K[8], Z);
    const double e0 = a.uv[(size_t)i * 2] - hu / hw, e1 = a.uv[(size_t)i * 2 + 1] - hv / hw;
    const double c00 = a.cov[(size_t)i * 4], c01 = a.cov[(size_t)i * 4 + 1], c10 = a.cov[(size_t)i * 4 + 2], c11 = a.cov[(size_t)i * 4 + 3];
    const double det = c00 * c11 - c01 * c10;
    double chi2 = ((c11 * (e0 * e0) - (c01 + c10) * (e0 * e1)) + c00 * (e1 * e1)) / det;
    const bool ok = det > 0 && c00 > 0 && c11 > 0 && isfinite(c01) && isfinite(c10) && isfinite(det) && isfinite(e0) && isfinite(e1) && isfinite(chi2);
    if (!ok) chi2 = __longlong_as_double(0x7ff8000000000000ll);
    a.chi2[i] = chi2;
    a.err[(size_t)i * 2] = e0;
    a.err[(size_t)i * 2 + 1] = e1;
}

void pose_nees_enqueue(const PoseNeesArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(pose_nees_kernel, dim3((a.n + NE_BLOCK / NE_G - 1) / (NE_BLOCK / NE_G)), dim3(NE_BLOCK), 0, stream, a);
}

void keypoint_nees_enqueue(const KpNeesArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(keypoint_nees_kernel, dim3((a.total + NE_BLOCK - 1) / NE_BLOCK), dim3(NE_BLOCK), 0, stream, a);
}

}  // namespace suo
