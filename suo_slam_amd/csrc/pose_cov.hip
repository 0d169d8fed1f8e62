// 6x6 marginal covariances of the camera and object poses of a bundle-adjustment problem at the state it holds (include/suo_hip.h: suo_pose_covariances).
//
//   H      = sum of J^T Omega J over the edges whose edge_inlier is 1 and whose camera and object are not both fixed -- no Huber weight, no lambda; the columns of J are
//            [omega, upsilon] of the left-multiplicative update exp(delta) T, restricted to the free vertices (the convention of suo_debug_ba_jacobians / lm_device.h)
//   Sigma  = H^-1; the result is its 6x6 diagonal block per vertex, 36 row-major doubles: zeros for a fixed vertex, NaNs for a free vertex without a counted edge
//            and for every block of a system whose factorisation meets a non-positive pivot.  The chi2 scale is not applied.
//
// Three forms, chosen per problem on the host (csrc/cov_stage.hip: plan_cov_batch -> LmProblem::cov_form):
//   0  no free camera: H is block-diagonal over the objects.  One wave per problem in the lane layout of csrc/lm_frame2.hip -- G = 8 lanes own an object (G = 4 from
//      9 objects on), lane (object, sub) walks the object's edges sub, sub + G, ...; the 21 packed entries of the block meet inside the group by log2(G) DPP steps;
//      every group inverts its own block by Cholesky in registers.  Problems of more than 64 / G objects are walked in passes: nothing couples the objects.
//   1  no free object (camera tracking): the same kernel over the cameras, with the camera's half of the Jacobian.
//   2  free cameras next to at most 16 free objects: one 256-thread workgroup per problem.  The linearisation and the per-pair sums are lm_device.h's (edge_pass_partial,
//      accumulate_pairs); S = Hoo - sum_c Hco^T Hcc^-1 Hco is factorised ONCE by the block-6 Cholesky of the LM kernels (wg_cholesky_factor), the ns columns of
//      S^-1 = Sigma_OO are the substitutions against the identity, dealt to the four waves (wave_cholesky_substitute: no workgroup barrier between columns), and stay
//      in LDS: a camera's block Hcc^-1 + Y Sigma_OO Y^T, Y = Hcc^-1 Hco over the objects it sees, needs the off-diagonal blocks between them.  A wave per camera
//      forms Z = Y Sigma_OO (6 x ns) and Z Y^T in the LDS the factor no longer needs.  A free vertex without a counted edge gets no row in the system.
//   3  the same system in device memory, spread over the grid (suo_pose_covariances_graph: more than 16 free objects, (camera, camera) pairs): csrc/pose_cov_graph.hip.
// Pairs (suo_pose_covariances_pairs): the cross block Sigma_ab and the covariance of the relative pose of requested vertex pairs (camera, object) / (object, object).
//   Forms 0 and 1 couple nothing, so every cross block between two different vertices is zero.  In form 2 the PAIRS instantiation of the coupled kernel writes, for
//   the requested pairs whose two vertices are in the system, Sigma_co = -Z[:, slot(o)] from the camera wave that holds Z (dense over the objects: also where the
//   camera does not see the object) and Sigma_ab from Sinv; the marginal entries keep the <false> instantiation, which compiles the pair work out.
//   pose_cov_pairs_kernel runs behind both kernels, a workgroup per 64 pairs of a problem and a thread per (pair, entry): it fills the blocks that are zeros (a fixed vertex,
//   forms 0 / 1), NaNs (a vertex whose marginal block is NaN) or the marginal block itself (a == b), and propagates  Sigma_cc + A Sigma_oo A^T + Sigma_co A^T +
//   A Sigma_oc, A = Ad(T_c),  or  B (Sigma_aa + Sigma_bb - Sigma_ab - Sigma_ba) B^T, B = Ad(T_b^-1)  (include/suo_hip.h); for the graph entry also (camera a, camera b):
//   Sigma_bb + A Sigma_aa A^T - A Sigma_ab - Sigma_ba A^T, A = Ad(T_b T_a^-1), with a zero cross block in forms 0 / 1 and form 3's Z_a Y_b^T otherwise.
// Vector stores only, no atomics; every sum runs in a fixed order, so two runs give the same bits, and a problem's result does not depend on the rest of the batch.
#include <algorithm>

#include "lm_device.h"
#include "lm_launch.h"
#include "pose_cov_device.h"

namespace suo {

static_assert(LM_THREADS == 256, "pose_cov_coupled_kernel: four waves");

template <int G>
DEV double pc_gsum(double v) {                  // sum over the G lanes of a group, the same value in each of them (csrc/lm_frame2.hip: gsum)
    v += dpp_get<0xB1>(v);                      // lane ^ 1
    v += dpp_get<0x4E>(v);                      // lane ^ 2
    if (G >= 8) v += dpp_get<0x141>(v);         // row_half_mirror: the other quad of the 8
    return v;
}

// inverse of the symmetric positive definite 6x6 given by its packed upper triangle, packed the same way: Cholesky A = L L^T, M = L^-1, A^-1 = M^T M (exactly
// symmetric).  Compile-time indices only: everything stays in registers.  false: a pivot was not positive (the result is then meaningless).
DEV bool spd_inverse6_packed(const double (&h)[21], double (&inv)[21]) {
    double A[6][6], L[6][6], M[6][6], dinv[6];
    bool ok = true;
    {
        int u = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) { A[c][r] = h[u]; ++u; }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double s = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
            if (i == j) {
                if (!(s > 0) || !isfinite(s)) ok = false;
                const double sp = ok ? s : 1.0;
                dinv[i] = rsqrt_nr(sp);
                L[i][i] = sp * dinv[i];
            } else {
                L[i][j] = s * dinv[j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        M[j][j] = dinv[j];
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double s = 0;
#pragma unroll
            for (int k = j; k < i; ++k) s += L[i][k] * M[k][j];
            M[i][j] = -(s * dinv[i]);
        }
    }
    {
        int u = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) {
                double s = 0;
#pragma unroll
                for (int k = c; k < 6; ++k) s += M[k][r] * M[k][c];
                inv[u] = s;
                ++u;
            }
    }
    return ok;
}

// forms 0 / 1: the blocks of the vertices of one side (CAM: cameras, else objects), every vertex of the other side being fixed
template <int G, bool CAM>
DEV void pose_cov_diag_body(const LmProblem& P) {
    constexpr int PER = 64 / G;
    const int lane = threadIdx.x, slot = lane / G, sub = lane % G;
    const int nv = CAM ? P.n_cam : P.n_obj;
    const int* vptr = CAM ? P.cam_pair_ptr : P.obj_pair_ptr;
    const int* vidx = CAM ? P.cam_pair_idx : P.obj_pair_idx;
    const uint8_t* vfixed = CAM ? P.cam_fixed : P.obj_fixed;
    double* out = CAM ? P.cam_cov : P.obj_cov;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    int n_nan = 0;
    for (int v0 = 0; v0 < nv; v0 += PER) {
        const int v = v0 + slot;
        const bool have = v < nv, fr = have && !vfixed[v];
        double h[21], cnt = 0;
#pragma unroll
        for (int k = 0; k < 21; ++k) h[k] = 0;
        if (fr) {
            for (int a = vptr[v]; a < vptr[v + 1]; ++a) {
                const int p = vidx[a];
                double Tc[12], To[12];
#pragma unroll
                for (int i = 0; i < 12; ++i) { Tc[i] = P.cam_T[12 * (size_t)P.pair_cam[p] + i]; To[i] = P.obj_T[12 * (size_t)P.pair_obj[p] + i]; }
                const int e1 = pair_hi(P, p);
                for (int e = P.pair_start[p] + sub; e < e1; e += G) {
                    if (!P.edge_inlier[e]) continue;
                    const double* x = P.edge_p + 3 * (size_t)e;
                    const double* k = P.edge_k + 4 * (size_t)e;
                    const double* I = P.edge_info + 3 * (size_t)e;
                    double pw[3], pc[3];
#pragma unroll
                    for (int r = 0; r < 3; ++r) pw[r] = To[4 * r] * x[0] + To[4 * r + 1] * x[1] + To[4 * r + 2] * x[2] + To[4 * r + 3];
#pragma unroll
                    for (int r = 0; r < 3; ++r) pc[r] = Tc[4 * r] * pw[0] + Tc[4 * r + 1] * pw[1] + Tc[4 * r + 2] * pw[2] + Tc[4 * r + 3];
                    // d err / d p_c (2x3, two structural zeros), then the vertex's half of EdgeSE3ProjectFromObject::linearizeOplus: [-[q]x | I] behind it,
                    // q = p_c for the camera, and behind R_c with q = p_w for the object
                    const double iz = 1.0 / pc[2];
                    const double pj00 = -(k[0] * iz), pj02 = k[0] * pc[0] * iz * iz, pj11 = -(k[1] * iz), pj12 = k[1] * pc[1] * iz * iz;
                    double a0[3], a1[3];
                    const double* q = CAM ? pc : pw;
                    if (CAM) {
                        a0[0] = pj00; a0[1] = 0; a0[2] = pj02;
                        a1[0] = 0; a1[1] = pj11; a1[2] = pj12;
                    } else {
#pragma unroll
                        for (int cc = 0; cc < 3; ++cc) { a0[cc] = pj00 * Tc[cc] + pj02 * Tc[8 + cc]; a1[cc] = pj11 * Tc[4 + cc] + pj12 * Tc[8 + cc]; }
                    }
                    const double J0[6] = {a0[2] * q[1] - a0[1] * q[2], a0[0] * q[2] - a0[2] * q[0], a0[1] * q[0] - a0[0] * q[1], a0[0], a0[1], a0[2]};
                    const double J1[6] = {a1[2] * q[1] - a1[1] * q[2], a1[0] * q[2] - a1[2] * q[0], a1[1] * q[0] - a1[0] * q[1], a1[0], a1[1], a1[2]};
                    double wj0[6], wj1[6];
#pragma unroll
                    for (int cc = 0; cc < 6; ++cc) { wj0[cc] = I[0] * J0[cc] + I[1] * J1[cc]; wj1[cc] = I[1] * J0[cc] + I[2] * J1[cc]; }
                    int u = 0;
#pragma unroll
                    for (int r = 0; r < 6; ++r)
#pragma unroll
                        for (int cc = r; cc < 6; ++cc) { h[u] += J0[r] * wj0[cc] + J1[r] * wj1[cc]; ++u; }
                    cnt += 1;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 21; ++k) h[k] = pc_gsum<G>(h[k]);
        cnt = pc_gsum<G>(cnt);
        double inv[21];
        const bool ok = spd_inverse6_packed(h, inv);          // every group its own block, in lock-step
        const bool bad = fr && !(ok && cnt > 0);
        if (have && sub == 0 && out) {
            double* o = out + 36 * (size_t)v;
            int u = 0;
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int cc = r; cc < 6; ++cc) {
                    const double val = !fr ? 0.0 : (bad ? nan : inv[u]);
                    o[r * 6 + cc] = val; o[cc * 6 + r] = val;
                    ++u;
                }
        }
        n_nan += __popcll(__ballot(bad && sub == 0));
    }
    // the other side: fixed vertices only
    double* other = CAM ? P.obj_cov : P.cam_cov;
    const int n_other = CAM ? P.n_obj : P.n_cam;
    if (other)
        for (int i = lane; i < 36 * n_other; i += 64) other[i] = 0.0;
    if (lane == 0 && P.cov_status) { P.cov_status[CAM ? 0 : 1] = n_nan; P.cov_status[CAM ? 1 : 0] = 0; }
}

// 8 lanes per vertex up to 8 vertices, 4 from 9 on (passes of 16): chosen per PROBLEM, so that its result does not depend on what else is in the launch
__global__ __launch_bounds__(64) void pose_cov_diag_kernel(const LmProblem* __restrict__ problems) {
    const LmProblem& P = problems[blockIdx.x];
    if (P.cov_form == 0) {
        if (P.n_obj <= 8) pose_cov_diag_body<8, false>(P);
        else pose_cov_diag_body<4, false>(P);
    } else if (P.cov_form == 1) {
        if (P.n_cam <= 8) pose_cov_diag_body<8, true>(P);
        else pose_cov_diag_body<4, true>(P);
    }
}

// form 2.  Dynamic LDS (doubles): [16: ok, ns, the object of every slot | Sinv ns x ns | S ns x (ns + 1), later the waves' camera buffers 4 x (12 ns + 36)]
constexpr int PC_HEAD = 16;
static size_t pose_cov_lds_bytes(int max_free_obj) {
    const size_t ns = 6 * (size_t)max_free_obj;
    return sizeof(double) * (PC_HEAD + ns * ns + std::max(ns * (ns + 1), (size_t)(LM_THREADS / 64) * (12 * ns + 36)));
}

template <bool PAIRS>
__global__ __launch_bounds__(LM_THREADS) void pose_cov_coupled_kernel(const LmProblem* __restrict__ problems) {
    const LmProblem& P = problems[blockIdx.x];
    if (P.cov_form != 2) return;
    extern __shared__ __attribute__((aligned(16))) double pc_lds[];
    int* sh = (int*)pc_lds;                     // [0] ok  [1] ns  [2 + s] the object in slot s
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    // ---- linearisation, per-vertex blocks, slots, Hcc^-1, Y and S: csrc/pose_cov_device.h, shared with form 3 (csrc/pose_cov_graph.hip) -----------------------
    const int ns = pc_assemble_blocks(P, sh, LM_MAX_SCHUR_OBJ), sp = ns + 1;
    auto cam_in = [&](int c) { return pc_cam_in(P, c); };
    double* Sinv = pc_lds + PC_HEAD;
    double* S = Sinv + ns * ns;
    pc_assemble_schur(P, sh, ns, S, sp);
    // ---- S = L L^T once; column c of Sigma_OO = S^-1 is the solve against e_c, one wave per column ----------------------------------
    wg_cholesky_factor(S, sp, ns, tid, LM_THREADS, &sh[0]);
    for (int col = wv; col < ns; col += LM_THREADS / 64) {
        double* rhs = Sinv + col * ns;
        for (int i = lane; i < ns; i += 64) rhs[i] = i == col ? 1.0 : 0.0;
        __builtin_amdgcn_wave_barrier();
        wave_cholesky_substitute(S, sp, rhs, ns, lane);
    }
    __syncthreads();
    const bool ok = sh[0] != 0;
    if (P.obj_cov)
        for (int idx = tid; idx < P.n_obj * 36; idx += LM_THREADS) {
            const int o = idx / 36, rc = idx - o * 36, r = rc / 6, cc = rc - r * 6;
            const int s = P.obj_slot[o];
            double val = 0.0;
            if (!P.obj_fixed[o]) val = (s < 0 || !ok) ? nan : 0.5 * (Sinv[(6 * s + r) * ns + 6 * s + cc] + Sinv[(6 * s + cc) * ns + 6 * s + r]);
            P.obj_cov[idx] = val;
        }
    if constexpr (PAIRS) {
        // Sigma_ab of the requested (object, object) pairs whose two objects are in the system, symmetrised like the marginal blocks: (a, b) is the transpose
        // of (b, a) to the bit, and (a, a) is the marginal block
        if (ok)
            for (int idx = tid; idx < P.n_cpair * 36; idx += LM_THREADS) {
                const int q = idx / 36, rc = idx - q * 36, r = rc / 6, cc = rc - r * 6;
                const int a = P.cpair_a[q] - P.n_cam, b = P.cpair_b[q] - P.n_cam;
                if (a < 0 || b < 0) continue;
                const int sa = P.obj_slot[a], sb = P.obj_slot[b];
                if (sa < 0 || sb < 0) continue;
                P.cov_cross[idx] = 0.5 * (Sinv[(6 * sa + r) * ns + 6 * sb + cc] + Sinv[(6 * sb + cc) * ns + 6 * sa + r]);
            }
    }
    // ---- cameras, a wave each: Hcc^-1 + Y Sigma_OO Y^T with Y (6 x ns, zero where the camera does not see the object), Z = Y Sigma_OO in the factor's LDS -----
    if (P.cam_cov) {
        double* Yd = S + wv * (12 * ns + 36);
        double* Z = Yd + 6 * ns;
        double* tmp = Z + 6 * ns;
        for (int c = wv; c < P.n_cam; c += LM_THREADS / 64) {
            double* oc = P.cam_cov + 36 * (size_t)c;
            if (P.cam_fixed[c] || !cam_in(c) || !ok) {
                if (lane < 36) oc[lane] = P.cam_fixed[c] ? 0.0 : nan;
                continue;
            }
            for (int i = lane; i < 6 * ns; i += 64) Yd[i] = 0;
            __builtin_amdgcn_wave_barrier();
            for (int a = P.cam_pair_ptr[c]; a < P.cam_pair_ptr[c + 1]; ++a) {
                const int p = P.cam_pair_idx[a], s = P.obj_slot[P.pair_obj[p]];
                if (s >= 0 && lane < 36) Yd[(lane / 6) * ns + 6 * s + lane % 6] = P.Y[36 * (size_t)p + lane];
            }
            __builtin_amdgcn_wave_barrier();
            for (int i = lane; i < 6 * ns; i += 64) {
                const int r = i / ns, j = i - r * ns;
                double acc = 0;
                for (int k = 0; k < ns; ++k) acc += Yd[r * ns + k] * Sinv[k * ns + j];
                Z[i] = acc;
            }
            __builtin_amdgcn_wave_barrier();
            const int r = (lane % 36) / 6, c2 = lane % 6;
            if constexpr (PAIRS) {
                // Sigma_co = -Z[:, slot(o)] of the requested pairs of this camera, while Z is in LDS; rows are the pair's first vertex.  The list is searched 64
                // pairs at a time, a lane each; the wave then writes the blocks of the hits one after the other
                for (int q0 = 0; q0 < P.n_cpair; q0 += 64) {
                    int s = -1;
                    bool cam_first = false;
                    if (q0 + lane < P.n_cpair) {
                        const int a = P.cpair_a[q0 + lane], b = P.cpair_b[q0 + lane];
                        cam_first = a == c && b >= P.n_cam;
                        if (cam_first || (b == c && a >= P.n_cam)) s = P.obj_slot[(cam_first ? b : a) - P.n_cam];
                    }
                    for (unsigned long long hits = __ballot(s >= 0); hits; hits &= hits - 1) {
                        const int l = __ffsll(hits) - 1;
                        const int sl = __shfl(s, l, 64);
                        const bool first = __shfl((int)cam_first, l, 64) != 0;
                        if (lane < 36) P.cov_cross[36 * (size_t)(q0 + l) + (first ? r * 6 + c2 : c2 * 6 + r)] = -Z[r * ns + 6 * sl + c2];
                    }
                }
            }
            if (lane < 36) {
                double acc = P.Hcc_inv[36 * c + lane];
                for (int j = 0; j < ns; ++j) acc += Z[r * ns + j] * Yd[c2 * ns + j];
                tmp[lane] = acc;
            }
            __builtin_amdgcn_wave_barrier();
            if (lane < 36) oc[lane] = 0.5 * (tmp[lane] + tmp[c2 * 6 + r]);
            __builtin_amdgcn_wave_barrier();
        }
    }
    __syncthreads();
    if (tid == 0 && P.cov_status) {
        int nc = 0, no = 0;
        if (P.cam_cov) for (int c = 0; c < P.n_cam; ++c) nc += isnan(P.cam_cov[36 * (size_t)c]) ? 1 : 0;
        if (P.obj_cov) for (int o = 0; o < P.n_obj; ++o) no += isnan(P.obj_cov[36 * (size_t)o]) ? 1 : 0;
        P.cov_status[0] = nc; P.cov_status[1] = no;
    }
}

// entry (r, c) of  Scc + A Soo A^T + Sco A^T + A Sco^T  (S1 = Scc, S2 = Soo, X = Sigma_co or, x_transposed, Sigma_oc)  or, obj_obj, of
// A (Saa + Sbb - Sab - Sab^T) A^T  (S1 = Saa, S2 = Sbb, X = Sigma_ab); Ar / Ac: rows r and c of A; X == nullptr: a cross block of zeros.  x_negated: the
// first form with -X, which is the (camera a, camera b) pair's  Sbb + A Saa A^T - Sba A^T - A Sab  (S1 = Sbb, S2 = Saa, X = Sigma_ab, x_transposed)
DEV double pc_rel_entry(bool obj_obj, const double* S1, const double* S2, const double* X, bool x_transposed, const double (&Ar)[6], const double (&Ac)[6], int r, int c,
                        bool x_negated = false) {
    auto x = [&](int i, int j) {
        const double v = !X ? 0.0 : (x_transposed ? X[6 * j + i] : X[6 * i + j]);
        return x_negated ? -v : v;
    };
    double acc = obj_obj ? 0.0 : S1[6 * r + c];
    for (int k = 0; k < 6; ++k) {
        double row = 0;
        for (int l = 0; l < 6; ++l) {
            const double d = obj_obj ? ((S1[6 * k + l] + S2[6 * k + l]) - x(k, l)) - x(l, k) : S2[6 * k + l];
            row += d * Ac[l];
        }
        acc += Ar[k] * row;
    }
    if (!obj_obj) {
        double w1 = 0, w2 = 0;
        for (int k = 0; k < 6; ++k) { w1 += x(r, k) * Ac[k]; w2 += Ar[k] * x(c, k); }
        acc += w1;
        acc += w2;
    }
    return acc;
}

// Behind the two kernels above, every form: cross and rel of the problem's requested pairs (the block comment on top), PC_PAIRS_PER_WG pairs per workgroup
// (blockIdx.y); the first workgroup of a problem also counts status[2] = pairs with NaN blocks (integer sums: no order to fix)
constexpr int PC_PAIRS_PER_WG = 64;
__global__ __launch_bounds__(LM_THREADS) void pose_cov_pairs_kernel(const LmProblem* __restrict__ problems) {
    const LmProblem& P = problems[blockIdx.x];
    const int tid = threadIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    auto block_of = [&](int v) { return v < P.n_cam ? P.cam_cov + 36 * (size_t)v : P.obj_cov + 36 * (size_t)(v - P.n_cam); };
    if (blockIdx.y == 0) {
        __shared__ int wave_nan[LM_THREADS / 64];
        int n = 0;
        for (int q = tid; q < P.n_cpair; q += LM_THREADS) n += (isnan(block_of(P.cpair_a[q])[0]) || isnan(block_of(P.cpair_b[q])[0])) ? 1 : 0;
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) n += __shfl_xor(n, m, 64);
        if ((tid & 63) == 0) wave_nan[tid >> 6] = n;
        __syncthreads();
        if (tid == 0 && P.cov_status) {
            int total = 0;
            for (int w = 0; w < LM_THREADS / 64; ++w) total += wave_nan[w];
            P.cov_status[2] = total;
        }
    }
    const int q_lo = blockIdx.y * PC_PAIRS_PER_WG, q_hi = min(P.n_cpair, q_lo + PC_PAIRS_PER_WG);
    for (int idx = 36 * q_lo + tid; idx < 36 * q_hi; idx += LM_THREADS) {
        const int q = idx / 36, rc = idx - q * 36, r = rc / 6, c = rc - r * 6;
        const int a = P.cpair_a[q], b = P.cpair_b[q];
        const bool a_cam = a < P.n_cam, b_cam = b < P.n_cam;
        const double* Sa = block_of(a);
        const double* Sb = block_of(b);
        const bool a_fixed = a_cam ? P.cam_fixed[a] : P.obj_fixed[a - P.n_cam], b_fixed = b_cam ? P.cam_fixed[b] : P.obj_fixed[b - P.n_cam];
        double* cross = P.cov_cross + 36 * (size_t)q;
        if (isnan(Sa[0]) || isnan(Sb[0])) { cross[rc] = nan; P.cov_rel[idx] = nan; continue; }
        // Sigma_ab: the marginal block (a == b), zeros (a fixed vertex; forms 0 / 1 couple nothing), or what the coupled kernel (form 3: pcg_cross_kernel of
        // csrc/pose_cov_graph.hip) wrote -- that block is only read here: the other threads of the pair read it too
        const bool same = a == b, zero = !same && (a_fixed || b_fixed || P.cov_form < 2);
        const double* X = same ? Sa : (zero ? nullptr : cross);
        if (same) cross[rc] = Sa[rc];
        if (zero) cross[rc] = 0.0;
        double Ar[6], Ac[6], m_rc, m_cr;
        if (a_cam && b_cam) {
            // (camera a, camera b) of suo_pose_covariances_graph: T_b T_a^-1, delta_rel = delta_b - A delta_a, A = Ad(T_b T_a^-1); (c, c) is the identity, exactly
            if (same) { P.cov_rel[idx] = 0.0; continue; }
            const double* Ta = P.cam_T + 12 * (size_t)a;
            const double* Tb = P.cam_T + 12 * (size_t)b;
            double Trel[12];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 3; ++j) Trel[4 * i + j] = (Tb[4 * i] * Ta[4 * j] + Tb[4 * i + 1] * Ta[4 * j + 1]) + Tb[4 * i + 2] * Ta[4 * j + 2];       // R_b R_a^T
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) Trel[4 * i + 3] = Tb[4 * i + 3] - ((Trel[4 * i] * Ta[3] + Trel[4 * i + 1] * Ta[7]) + Trel[4 * i + 2] * Ta[11]);
            pc_ad_row(Trel, false, r, Ar);
            pc_ad_row(Trel, false, c, Ac);
            m_rc = pc_rel_entry(false, Sb, Sa, X, true, Ar, Ac, r, c, true);
            m_cr = pc_rel_entry(false, Sb, Sa, X, true, Ac, Ar, c, r, true);
        } else if (!a_cam && !b_cam) {
            const double* Tb = P.obj_T + 12 * (size_t)(b - P.n_cam);
            pc_ad_row(Tb, true, r, Ar);
            pc_ad_row(Tb, true, c, Ac);
            m_rc = pc_rel_entry(true, Sa, Sb, X, false, Ar, Ac, r, c);
            m_cr = pc_rel_entry(true, Sa, Sb, X, false, Ac, Ar, c, r);
        } else {
            const double* Tc = P.cam_T + 12 * (size_t)(a_cam ? a : b);
            pc_ad_row(Tc, false, r, Ar);
            pc_ad_row(Tc, false, c, Ac);
            m_rc = pc_rel_entry(false, a_cam ? Sa : Sb, a_cam ? Sb : Sa, X, !a_cam, Ar, Ac, r, c);
            m_cr = pc_rel_entry(false, a_cam ? Sa : Sb, a_cam ? Sb : Sa, X, !a_cam, Ac, Ar, c, r);
        }
        P.cov_rel[idx] = 0.5 * (m_rc + m_cr);
    }
}

int launch_pose_cov_diag(const void* problems_dev, int n_problems, hipStream_t s) {
    if (n_problems <= 0) return SUO_OK;
    hipLaunchKernelGGL(pose_cov_diag_kernel, dim3(n_problems), dim3(64), 0, s, (const LmProblem*)problems_dev);
    SUO_HIP_CHECK(hipGetLastError());
    return SUO_OK;
}

template <bool PAIRS>
static int launch_pose_cov_coupled_as(const void* problems_dev, int n_problems, int max_free_obj, hipStream_t s) {
    if (n_problems <= 0) return SUO_OK;
    if (max_free_obj < 0 || max_free_obj > LM_MAX_SCHUR_OBJ) {
        suo_set_error("pose covariances: %d free objects next to free cameras (the reduced system holds %d)", max_free_obj, LM_MAX_SCHUR_OBJ);
        return SUO_ERR_ARG;
    }
    static bool attr_set = false;
    if (!attr_set) {
        SUO_HIP_CHECK(hipFuncSetAttribute((const void*)pose_cov_coupled_kernel<PAIRS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pose_cov_lds_bytes(LM_MAX_SCHUR_OBJ)));
        attr_set = true;
    }
    hipLaunchKernelGGL(pose_cov_coupled_kernel<PAIRS>, dim3(n_problems), dim3(LM_THREADS), pose_cov_lds_bytes(max_free_obj), s, (const LmProblem*)problems_dev);
    SUO_HIP_CHECK(hipGetLastError());
    return SUO_OK;
}

int launch_pose_cov_coupled(const void* problems_dev, int n_problems, int max_free_obj, hipStream_t s, bool pairs) {
    return pairs ? launch_pose_cov_coupled_as<true>(problems_dev, n_problems, max_free_obj, s) : launch_pose_cov_coupled_as<false>(problems_dev, n_problems, max_free_obj, s);
}

int launch_pose_cov_pairs(const void* problems_dev, int n_problems, int max_pairs, hipStream_t s) {
    if (n_problems <= 0) return SUO_OK;
    const int ny = std::max(1, (max_pairs + PC_PAIRS_PER_WG - 1) / PC_PAIRS_PER_WG);
    hipLaunchKernelGGL(pose_cov_pairs_kernel, dim3(n_problems, ny), dim3(LM_THREADS), 0, s, (const LmProblem*)problems_dev);
    SUO_HIP_CHECK(hipGetLastError());
    return SUO_OK;
}

}  // namespace suo
