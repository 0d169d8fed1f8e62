// cov_form 3 of the pose covariances (include/suo_hip.h: suo_pose_covariances_graph): free cameras next to free objects with the reduced system in DEVICE MEMORY
// and the work spread over the grid -- maps of more than 16 free objects (up to POSE_COV_GRAPH_MAX_OBJ) and every coupled problem that asks for a
// (camera, camera) pair.  Definitions, NaN rules and outputs are those of csrc/pose_cov.hip; the assembly is shared with its form 2 (csrc/pose_cov_device.h).
//
// Per problem the arena holds S (ns x (ns + 1), later its factor), Sigma_OO (ns x ns), Z = Y Sigma_OO of every camera (6 x ns each) and a header [ok, ns, the object
// of every slot] (csrc/cov_stage.hip), ns = 6 * free objects with a counted edge.  A phase hands data to other workgroups only across a launch boundary: a CU's vector
// L1 is not refreshed by another CU's stores and the per-XCD L2s are not coherent inside a kernel, so there is no grid barrier and no flag.  Four launches:
//   1  pcg_factor_kernel    one workgroup per problem: assembly, then S = L L^T in place, blocked by 6 -- the diagonal 6 x 6 redundantly in registers, the panel
//                           (a row per thread, kept in LDS for the update: 6 doubles per row), the trailing update in 16 x 16 tiles over the workgroup.
//                           1 / L_rr sits right of the diagonal.  A non-positive or non-finite pivot clears `ok` and the factorisation runs on with 1.0.
//   2  pcg_columns_kernel   grid (problem, 4 columns), one wave per column c of Sigma_OO = S^-1: L y = e_c from row c on (the rows above are zeros), each row of L read
//                           coalesced, multiplied lane-wise and reduced across the wave; L^T x = y as ns updates x[k] -= L[i][k] x[i] (k < i), the same rows again.
//                           The next row's loads are issued before the current row's arithmetic.  y: ns doubles of LDS per wave.  No column waits for another.
//   3  pcg_cameras_kernel   grid (problem, 4 cameras), one wave per camera: Z_c = Y_c Sigma_OO over the objects the camera sees (lane j owns column j, j + 64, ...),
//                           written to the scratch; Sigma_cc = Hcc^-1 + Z_c Y_c^T from the lanes' partial products, reduced across the wave, symmetrised.  The first
//                           workgroup of a problem also writes the objects' blocks from Sigma_OO.
//   4  pcg_cross_kernel     grid (problem, 64 pairs): Sigma_ab of the requested pairs whose two vertices are in the system -- (object, object) from Sigma_OO,
//                           (camera, object) = -Z_c[:, slot(o)], (camera a, camera b) = Z_a Y_b^T, symmetrised with (b, a) so that (a, b) is the transpose of (b, a) to the
//                           bit -- and status[0..1].  pose_cov_pairs_kernel (csrc/pose_cov.hip) runs behind it as behind the other forms.
// fp64, vector stores only, no atomics; every sum runs in a fixed order that depends on the problem alone, so two runs give the same bits and a problem's result does
// not depend on the rest of the batch.  No LDS array grows with ns^2; the two that grow with ns (the panel, a wave's y) are sized for the cap.
#include <algorithm>

#include "lm_device.h"
#include "lm_launch.h"
#include "pose_cov_device.h"

namespace suo {

static_assert(LM_THREADS == 256, "csrc/pose_cov_graph.hip: four waves, 16 x 16 tiles");
constexpr int PCG_NS_MAX = 6 * POSE_COV_GRAPH_MAX_OBJ;
constexpr int PCG_KPL = PCG_NS_MAX / 64;          // elements of a row of L per lane
static_assert(PCG_NS_MAX % 64 == 0, "a lane owns PCG_KPL columns");
constexpr int PCG_PANEL_PITCH = 7;                // odd: lanes of consecutive rows on different LDS banks
constexpr int PCG_WAVES = LM_THREADS / 64;

__global__ __launch_bounds__(LM_THREADS) void pcg_factor_kernel(const LmProblem* __restrict__ problems) {
    const LmProblem& P = problems[blockIdx.x];
    if (P.cov_form != 3) return;
    __shared__ double panel[PCG_NS_MAX * PCG_PANEL_PITCH];
    const int tid = threadIdx.x;
    int* hdr = P.cov_hdr;
    const int ns = pc_assemble_blocks(P, hdr, POSE_COV_GRAPH_MAX_OBJ), sp = ns + 1;
    double* S = P.cov_S;
    pc_assemble_schur(P, hdr, ns, S, sp);
    for (int k0 = 0; k0 < ns; k0 += 6) {
        double L[6][6], rd[6];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c) L[r][c] = S[(k0 + r) * sp + k0 + c];
        bool good = true;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            double piv = L[c][c];
#pragma unroll
            for (int q = 0; q < c; ++q) piv -= L[c][q] * L[c][q];
            const bool pos = piv > 0 && isfinite(piv);
            if (!pos) good = false;
            const double pp = pos ? piv : 1.0;
            rd[c] = rsqrt_nr(pp);
            L[c][c] = pp * rd[c];
#pragma unroll
            for (int r = c + 1; r < 6; ++r) {
                double v = L[r][c];
#pragma unroll
                for (int q = 0; q < c; ++q) v -= L[r][q] * L[c][q];
                L[r][c] = v * rd[c];
            }
        }
        if (!good && tid == 0) hdr[0] = 0;
        const int base = k0 + 6, m = ns - base;
        // panel row base + t:  L21[t][.] = A21[t][.] L11^-T
        for (int t = tid; t < m; t += LM_THREADS) {
            double* row = S + (size_t)(base + t) * sp + k0;
            double x[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                double v = row[c];
#pragma unroll
                for (int q = 0; q < c; ++q) v -= x[q] * L[c][q];
                x[c] = v * rd[c];
            }
#pragma unroll
            for (int c = 0; c < 6; ++c) { row[c] = x[c]; panel[t * PCG_PANEL_PITCH + c] = x[c]; }
        }
        __syncthreads();                                   // panel complete; every thread has read the diagonal block
        if (tid == 0) {
#pragma unroll
            for (int r = 0; r < 6; ++r) {
#pragma unroll
                for (int c = 0; c <= r; ++c) S[(k0 + r) * sp + k0 + c] = L[r][c];
                S[(k0 + r) * sp + k0 + r + 1] = rd[r];     // never referenced otherwise (sp > ns: the last row's is the pad column)
            }
        }
        // trailing update of the lower triangle, 16 x 16 tiles of (row a, column b <= a): a thread's element takes its six products in column order
        const int ty = tid >> 4, tx = tid & 15;
        for (int a = ty; a < m; a += 16) {
            double la[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) la[c] = panel[a * PCG_PANEL_PITCH + c];
            double* row = S + (size_t)(base + a) * sp + base;
            for (int b = tx; b <= a; b += 16) {
                double acc = row[b];
#pragma unroll
                for (int c = 0; c < 6; ++c) acc -= la[c] * panel[b * PCG_PANEL_PITCH + c];
                row[b] = acc;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(LM_THREADS) void pcg_columns_kernel(const LmProblem* __restrict__ problems) {
    const LmProblem& P = problems[blockIdx.x];
    if (P.cov_form != 3) return;
    __shared__ double ybuf[PCG_WAVES][PCG_NS_MAX];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int ns = __builtin_amdgcn_readfirstlane(P.cov_hdr[1]), sp = ns + 1;
    const int col = blockIdx.y * PCG_WAVES + wv;
    if (col >= ns) return;                                 // (no workgroup barrier below)
    const int nj = (ns + 63) >> 6;
    const double* S = P.cov_S;
    double* y = ybuf[wv];
#pragma unroll
    for (int j = 0; j < PCG_KPL; ++j) y[lane + 64 * j] = 0.0;
    __builtin_amdgcn_wave_barrier();
    // elements [lo, hi) of row i of L, lane-strided (zeros outside), and 1 / L_ii
    auto load_row = [&](int i, int lo, int hi, double (&v)[PCG_KPL], double& rdi) {
        const double* row = S + (size_t)i * sp;
#pragma unroll
        for (int j = 0; j < PCG_KPL; ++j) {
            const int k = lane + 64 * j;
            v[j] = (j < nj && k >= lo && k < hi) ? row[k] : 0.0;
        }
        rdi = row[i + 1];
    };
    double cur[PCG_KPL], nxt[PCG_KPL], rd_cur, rd_nxt = 0;
    // ---- L y = e_col: rows col .. ns - 1 ----
    load_row(col, col, col, cur, rd_cur);
    for (int i = col; i < ns; ++i) {
        if (i + 1 < ns) load_row(i + 1, col, i + 1, nxt, rd_nxt);
        double part = 0;
#pragma unroll
        for (int j = 0; j < PCG_KPL; ++j) part += cur[j] * y[lane + 64 * j];
        const double yi = ((i == col ? 1.0 : 0.0) - wsum(part)) * rd_cur;
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) y[i] = yi;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < PCG_KPL; ++j) cur[j] = nxt[j];
        rd_cur = rd_nxt;
    }
    // ---- L^T x = y: from the last row up, x[k] -= L[i][k] x[i] for k < i ----
    load_row(ns - 1, 0, ns - 1, cur, rd_cur);
    for (int i = ns - 1; i >= 0; --i) {
        if (i > 0) load_row(i - 1, 0, i - 1, nxt, rd_nxt);
        const double xi = y[i] * rd_cur;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < PCG_KPL; ++j) {
            const int k = lane + 64 * j;
            if (k < i) y[k] -= cur[j] * xi;
        }
        if (lane == 0) y[i] = xi;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < PCG_KPL; ++j) cur[j] = nxt[j];
        rd_cur = rd_nxt;
    }
    double* out = P.cov_Sinv + (size_t)col * ns;
    for (int k = lane; k < ns; k += 64) out[k] = y[k];
}

__global__ __launch_bounds__(LM_THREADS) void pcg_cameras_kernel(const LmProblem* __restrict__ problems) {
    const LmProblem& P = problems[blockIdx.x];
    if (P.cov_form != 3) return;
    __shared__ double tmp[PCG_WAVES][36];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const int* hdr = P.cov_hdr;
    const bool ok = hdr[0] != 0;
    const int ns = __builtin_amdgcn_readfirstlane(hdr[1]);
    const double* Sinv = P.cov_Sinv;
    if (blockIdx.y == 0)
        for (int idx = tid; idx < P.n_obj * 36; idx += LM_THREADS) {
            const int o = idx / 36, rc = idx - o * 36, r = rc / 6, cc = rc - r * 6;
            const int s = P.obj_slot[o];
            double val = 0.0;
            if (!P.obj_fixed[o]) val = (s < 0 || !ok) ? nan : 0.5 * (Sinv[(size_t)(6 * s + r) * ns + 6 * s + cc] + Sinv[(size_t)(6 * s + cc) * ns + 6 * s + r]);
            P.obj_cov[idx] = val;
        }
    const int c = blockIdx.y * PCG_WAVES + wv;
    if (c >= P.n_cam) return;                              // (no workgroup barrier below)
    double* oc = P.cam_cov + 36 * (size_t)c;
    if (!pc_cam_in(P, c) || !ok) {
        if (lane < 36) oc[lane] = P.cam_fixed[c] ? 0.0 : nan;
        return;
    }
    double* Z = P.cov_Z + (size_t)c * 6 * ns;
    const int a0 = P.cam_pair_ptr[c], a1 = P.cam_pair_ptr[c + 1];
    double part[36];
#pragma unroll
    for (int u = 0; u < 36; ++u) part[u] = 0;
    for (int j = lane; j < ns; j += 64) {
        // column j of Z = Y Sigma_OO: the objects the camera sees in CSR order, their six rows of Sigma_OO read coalesced
        double acc[6] = {0, 0, 0, 0, 0, 0};
        for (int a = a0; a < a1; ++a) {
            const int p = P.cam_pair_idx[a], s = P.obj_slot[P.pair_obj[p]];
            if (s < 0) continue;
            const double* Yp = P.Y + 36 * (size_t)p;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const double v = Sinv[(size_t)(6 * s + k) * ns + j];
#pragma unroll
                for (int r = 0; r < 6; ++r) acc[r] += Yp[r * 6 + k] * v;
            }
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) Z[(size_t)r * ns + j] = acc[r];
        // this column's share of Z Y^T: column j of Y is (slot j / 6, dof j % 6) of the camera's pair with that object, zero where it does not see it
        const int sj = j / 6, kj = j - 6 * sj;
        const int pj = P.cam_obj_pair[(size_t)c * P.n_obj + hdr[2 + sj]];
        if (pj >= 0) {
            const double* Yp = P.Y + 36 * (size_t)pj;
#pragma unroll
            for (int c2 = 0; c2 < 6; ++c2) {
                const double yv = Yp[c2 * 6 + kj];
#pragma unroll
                for (int r = 0; r < 6; ++r) part[r * 6 + c2] += acc[r] * yv;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < 36; ++u) {
        const double total = wsum(part[u]);
        if (lane == 0) tmp[wv][u] = total;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < 36) {
        const int r = lane / 6, c2 = lane - 6 * r, tr = c2 * 6 + r;
        const double v = P.Hcc_inv[36 * c + lane] + tmp[wv][lane], vt = P.Hcc_inv[36 * c + tr] + tmp[wv][tr];
        oc[lane] = 0.5 * (v + vt);
    }
}

// (Z_a Y_b^T)[r][c]: the objects camera b sees, in CSR order
DEV double pcg_zy(const LmProblem& P, int ns, int a, int b, int r, int c) {
    const double* Za = P.cov_Z + ((size_t)a * 6 + r) * ns;
    double acc = 0;
    for (int i = P.cam_pair_ptr[b]; i < P.cam_pair_ptr[b + 1]; ++i) {
        const int p = P.cam_pair_idx[i], s = P.obj_slot[P.pair_obj[p]];
        if (s < 0) continue;
        const double* Yp = P.Y + 36 * (size_t)p + 6 * c;
        for (int k = 0; k < 6; ++k) acc += Za[6 * s + k] * Yp[k];
    }
    return acc;
}

constexpr int PCG_PAIRS_PER_WG = 64;
__global__ __launch_bounds__(LM_THREADS) void pcg_cross_kernel(const LmProblem* __restrict__ problems) {
    const LmProblem& P = problems[blockIdx.x];
    if (P.cov_form != 3) return;
    const int tid = threadIdx.x;
    if (blockIdx.y == 0) {
        // status[0..1]: the NaN blocks of the cameras and of the objects (integer sums: no order to fix)
        __shared__ int wave_nan[PCG_WAVES][2];
        int nc = 0, no = 0;
        for (int c = tid; c < P.n_cam; c += LM_THREADS) nc += isnan(P.cam_cov[36 * (size_t)c]) ? 1 : 0;
        for (int o = tid; o < P.n_obj; o += LM_THREADS) no += isnan(P.obj_cov[36 * (size_t)o]) ? 1 : 0;
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) { nc += __shfl_xor(nc, m, 64); no += __shfl_xor(no, m, 64); }
        if ((tid & 63) == 0) { wave_nan[tid >> 6][0] = nc; wave_nan[tid >> 6][1] = no; }
        __syncthreads();
        if (tid == 0 && P.cov_status) {
            int tc = 0, to = 0;
            for (int w = 0; w < PCG_WAVES; ++w) { tc += wave_nan[w][0]; to += wave_nan[w][1]; }
            P.cov_status[0] = tc; P.cov_status[1] = to;
        }
    }
    const int* hdr = P.cov_hdr;
    if (hdr[0] == 0) return;                               // a bad pivot: every free vertex is NaN, the pair kernel fills the blocks
    const int ns = hdr[1];
    const double* Sinv = P.cov_Sinv;
    const int q_lo = blockIdx.y * PCG_PAIRS_PER_WG, q_hi = min(P.n_cpair, q_lo + PCG_PAIRS_PER_WG);
    for (int idx = 36 * q_lo + tid; idx < 36 * q_hi; idx += LM_THREADS) {
        const int q = idx / 36, rc = idx - q * 36, r = rc / 6, c = rc - r * 6;
        const int a = P.cpair_a[q], b = P.cpair_b[q];
        if (a == b) continue;                              // the marginal block: the pair kernel's
        const bool a_cam = a < P.n_cam, b_cam = b < P.n_cam;
        if (a_cam && b_cam) {
            if (!pc_cam_in(P, a) || !pc_cam_in(P, b)) continue;
            P.cov_cross[idx] = 0.5 * (pcg_zy(P, ns, a, b, r, c) + pcg_zy(P, ns, b, a, c, r));
        } else if (!a_cam && !b_cam) {
            const int sa = P.obj_slot[a - P.n_cam], sb = P.obj_slot[b - P.n_cam];
            if (sa < 0 || sb < 0) continue;
            P.cov_cross[idx] = 0.5 * (Sinv[(size_t)(6 * sa + r) * ns + 6 * sb + c] + Sinv[(size_t)(6 * sb + c) * ns + 6 * sa + r]);
        } else {
            // Sigma_co = -Z_c[:, slot(o)], rows the pair's first vertex
            const int cam = a_cam ? a : b, s = P.obj_slot[(a_cam ? b : a) - P.n_cam];
            if (!pc_cam_in(P, cam) || s < 0) continue;
            const double* Zc = P.cov_Z + (size_t)cam * 6 * ns;
            P.cov_cross[idx] = -(a_cam ? Zc[(size_t)r * ns + 6 * s + c] : Zc[(size_t)c * ns + 6 * s + r]);
        }
    }
}

int launch_pose_cov_graph(const void* problems_dev, int n_problems, int max_free_obj, int max_cam, int max_pairs, hipStream_t s) {
    if (n_problems <= 0) return SUO_OK;
    if (max_free_obj < 0 || max_free_obj > POSE_COV_GRAPH_MAX_OBJ) {
        suo_set_error("pose covariances: %d free objects next to free cameras (the device-memory form takes %d)", max_free_obj, POSE_COV_GRAPH_MAX_OBJ);
        return SUO_ERR_ARG;
    }
    const LmProblem* P = (const LmProblem*)problems_dev;
    const int n_col = std::max(1, (6 * max_free_obj + PCG_WAVES - 1) / PCG_WAVES), n_camg = std::max(1, (max_cam + PCG_WAVES - 1) / PCG_WAVES);
    const int n_pairg = std::max(1, (max_pairs + PCG_PAIRS_PER_WG - 1) / PCG_PAIRS_PER_WG);
    hipLaunchKernelGGL(pcg_factor_kernel, dim3(n_problems), dim3(LM_THREADS), 0, s, P);
    hipLaunchKernelGGL(pcg_columns_kernel, dim3(n_problems, n_col), dim3(LM_THREADS), 0, s, P);
    hipLaunchKernelGGL(pcg_cameras_kernel, dim3(n_problems, n_camg), dim3(LM_THREADS), 0, s, P);
    hipLaunchKernelGGL(pcg_cross_kernel, dim3(n_problems, n_pairg), dim3(LM_THREADS), 0, s, P);
    SUO_HIP_CHECK(hipGetLastError());
    return SUO_OK;
}

}  // namespace suo
