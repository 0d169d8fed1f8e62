// The assembly of the coupled pose-covariance forms, shared by csrc/pose_cov.hip (form 2: the reduced system in LDS) and csrc/pose_cov_graph.hip (form 3: in
// device memory): the linearisation and the per-pair sums of lm_device.h, the vertices' diagonal blocks, the slots of the reduced system, Hcc^-1, Y and S.
// One workgroup of LM_THREADS threads per problem, every thread calling; the same operations in the same order whatever memory `sh` and `S` point to.
#pragma once
#include "lm_device.h"

namespace suo {

// row r of Ad(T) = [[R, 0], [[t]x R, R]] of the pose T (row-major 3x4), or of Ad(T^-1) (R^T, -R^T t); the pair kernel of csrc/pose_cov.hip and
// csrc/track_cov.hip propagate with it
DEV void pc_ad_row(const double* T, bool inverse, int r, double (&row)[6]) {
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) R[3 * i + j] = inverse ? T[4 * j + i] : T[4 * i + j];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = inverse ? -(T[i] * T[3] + T[4 + i] * T[7] + T[8 + i] * T[11]) : T[4 * i + 3];
    const int i = r % 3, i1 = (i + 1) % 3, i2 = (i + 2) % 3;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double tx = t[i1] * R[3 * i2 + j] - t[i2] * R[3 * i1 + j];     // ([t]x R)[i][j]
        row[j] = r < 3 ? R[3 * i + j] : tx;
        row[3 + j] = r < 3 ? 0.0 : R[3 * i + j];
    }
}

DEV bool pc_cam_in(const LmProblem& P, int c) { return !P.cam_fixed[c] && P.xc[6 * c] > 0; }

// Linearises at the state the problem holds, sums Hcc / Hoo per vertex, marks the vertices a counted edge reaches (xc / xo [6 v]), deals the slots of the reduced
// system to the free objects with a counted edge -- at most max_slots of them -- and inverts every Hcc.  sh: [0] ok (cleared on a camera block that is not positive
// definite)  [1] ns = 6 * slots  [2 + s] the object in slot s.  Returns ns, the same in every thread; ends on a barrier.
DEV int pc_assemble_blocks(const LmProblem& P, int* sh, int max_slots) {
    const int tid = threadIdx.x;
    // ---- the state as the LM kernels hold it; level 1 = not counted -------------------------------------------------------------
    for (int c = tid; c < P.n_cam; c += LM_THREADS) pose_from_T(P.cam_T + 12 * c, P.cam[c]);
    for (int o = tid; o < P.n_obj; o += LM_THREADS) pose_from_T(P.obj_T + 12 * o, P.obj[o]);
    for (int e = tid; e < P.n_edge; e += LM_THREADS) P.level[e] = P.edge_inlier[e] ? 0 : 1;
    if (tid == 0) sh[0] = 1;
    __syncthreads();
    (void)edge_pass_partial(P, 0, P.n_edge, false, true);      // Jacobians, weight 1
    __syncthreads();
    accumulate_pairs(P);                                        // per pair Hcc (21) Hoo (21) Hco (36), edge order
    __syncthreads();
    // ---- per vertex: its diagonal block (pairs in CSR order) and whether any counted edge reaches it (xc / xo [6 v]: scratch) ----
    for (int idx = tid; idx < P.n_cam * 21; idx += LM_THREADS) {
        const int c = idx / 21, k = idx - c * 21;
        double s = 0;
        if (!P.cam_fixed[c])
            for (int a = P.cam_pair_ptr[c]; a < P.cam_pair_ptr[c + 1]; ++a) s += P.pair_part[90 * (size_t)P.cam_pair_idx[a] + k];
        P.Hcc[36 * c + k] = s;
    }
    for (int idx = tid; idx < P.n_obj * 21; idx += LM_THREADS) {
        const int o = idx / 21, k = idx - o * 21;
        double s = 0;
        if (!P.obj_fixed[o])
            for (int a = P.obj_pair_ptr[o]; a < P.obj_pair_ptr[o + 1]; ++a) s += P.pair_part[90 * (size_t)P.obj_pair_idx[a] + 21 + k];
        P.Hoo[36 * o + k] = s;
    }
    for (int v = tid; v < P.n_cam + P.n_obj; v += LM_THREADS) {
        const bool is_cam = v < P.n_cam;
        const int i = is_cam ? v : v - P.n_cam;
        int n = 0;
        if (!(is_cam ? P.cam_fixed[i] : P.obj_fixed[i])) {
            const int* ptr = is_cam ? P.cam_pair_ptr : P.obj_pair_ptr;
            const int* pidx = is_cam ? P.cam_pair_idx : P.obj_pair_idx;
            for (int a = ptr[i]; a < ptr[i + 1]; ++a)
                for (int e = P.pair_start[pidx[a]]; e < P.pair_start[pidx[a] + 1]; ++e) n += P.level[e] == 0 ? 1 : 0;
        }
        (is_cam ? P.xc : P.xo)[6 * i] = n > 0 ? 1.0 : 0.0;
    }
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int o = 0; o < P.n_obj; ++o) {
            const bool in = !P.obj_fixed[o] && P.xo[6 * o] > 0 && n < max_slots;
            P.obj_slot[o] = in ? n : -1;
            if (in) { sh[2 + n] = o; ++n; }
        }
        sh[1] = 6 * n;
    }
    for (int c = tid; c < P.n_cam; c += LM_THREADS) {
        if (!pc_cam_in(P, c)) continue;
        double A[36], Ai[36];
        unpack_sym21(P.Hcc + 36 * c, A);
        if (!spd_inverse6(A, Ai)) { sh[0] = 0; for (int i = 0; i < 36; ++i) Ai[i] = 0; }
        for (int i = 0; i < 36; ++i) P.Hcc_inv[36 * c + i] = Ai[i];
    }
    __syncthreads();
    return __builtin_amdgcn_readfirstlane(sh[1]);
}

// Y[p] = Hcc^-1 Hco[p];  S = blockdiag(Hoo) - sum_c Hco(c, o1)^T Y(c, o2), cameras in CSR order (csrc/lm.hip), into S (ns rows of pitch sp, zeroed first: the
// element right of the diagonal is the factorisation's).  Ends on a barrier.
DEV void pc_assemble_schur(const LmProblem& P, const int* sh, int ns, double* S, int sp) {
    const int tid = threadIdx.x;
    for (int idx = tid; idx < P.n_pair * 36; idx += LM_THREADS) {
        const int p = idx / 36, rc = idx - p * 36, r = rc / 6, cc = rc - r * 6;
        const int c = P.pair_cam[p];
        double s = 0;
        if (pc_cam_in(P, c) && P.obj_slot[P.pair_obj[p]] >= 0) {
            const double* Hco = P.pair_part + 90 * (size_t)p + 42;
            for (int k = 0; k < 6; ++k) s += P.Hcc_inv[36 * c + r * 6 + k] * Hco[k * 6 + cc];
        }
        P.Y[idx] = s;
    }
    for (int idx = tid; idx < ns * sp; idx += LM_THREADS) S[idx] = 0;
    __syncthreads();
    for (int idx = tid; idx < ns * ns; idx += LM_THREADS) {
        const int row = idx / ns, col = idx - row * ns;
        const int s1 = row / 6, i = row - s1 * 6, s2 = col / 6, j = col - s2 * 6;
        const int o1 = sh[2 + s1], o2 = sh[2 + s2];
        double acc = 0;
        if (s1 == s2) {
            const int rr = i < j ? i : j, c2 = i < j ? j : i;
            acc = P.Hoo[36 * o1 + rr * 6 - rr * (rr - 1) / 2 + (c2 - rr)];
        }
        double sub = 0;
        for (int a = P.obj_pair_ptr[o1]; a < P.obj_pair_ptr[o1 + 1]; ++a) {
            const int p1 = P.obj_pair_idx[a], c = P.pair_cam[p1];
            const int p2 = P.cam_obj_pair[(size_t)c * P.n_obj + o2];      // the same camera's pair with object o2
            if (!pc_cam_in(P, c) || p2 < 0) continue;
            const double* H1 = P.pair_part + 90 * (size_t)p1 + 42;       // Hco(c, o1), row = camera dof
            const double* Y2 = P.Y + 36 * (size_t)p2;
            for (int k = 0; k < 6; ++k) sub += H1[k * 6 + i] * Y2[k * 6 + j];
        }
        S[row * sp + col] = acc - sub;
    }
    __syncthreads();
}

}  // namespace suo
