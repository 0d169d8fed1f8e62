// Host-buffer entry points of the PnP kernels (what the reference's FFI would bind):
//   suo_pnp / suo_pnp_batch / suo_pnp_replay  <- lambdatwist.pnp      (thirdparty/lambdatwist/pnp_python_binding.cpp:57-62)
// They stage the caller's host arrays into the process arena (one H2D), launch, and copy results back (one D2H).
#include <math.h>
#include <string.h>

#include <algorithm>

#include "ba_stage.h"

namespace suo {

// PnpParams::get_iterations (thirdparty/lambdatwist/parameters.h:76-102), evaluated on the host so the
// kernel's adaptive iteration count uses the same libm as the reference would.
int pnp_get_iterations(double estimated_inliers) {
    const double p_meets = 0.9, min_probability = 0.99999;
    const unsigned max_iterations = 1000, min_iterations = 100;
    double p_inlier = std::min(0.9, estimated_inliers * p_meets);
    p_inlier = std::min(std::max(p_inlier, 1e-2), 1 - 1e-8);
    if (p_inlier < 0.01) return (int)max_iterations;
    const double p_failure = std::min(std::max(1.0 - min_probability, 1e-8), 0.01);
    const double p_good = pow(p_inlier, 4);
    const double iterations = ceil(log(p_failure) / log(1.0 - p_good)) + 50;
    if (iterations < min_iterations) return (int)min_iterations;
    if (iterations > max_iterations) return (int)max_iterations;
    return (int)iterations;
}

}  // namespace suo

using namespace suo;

extern "C" {

static int pnp_batch_impl(int n_obj, const int* n_pts, const double* xs, const double* ys, double threshold, uint64_t seed, const int* draws, int n_draws,
                          int do_refine, double* T_out, int* status, int* best_inliers, int* iterations, int* winner) {
    if (n_obj <= 0) return SUO_OK;
    if (!n_pts || !xs || !ys || !T_out) { suo_set_error("suo_pnp_batch: null argument"); return SUO_ERR_ARG; }
    if (draws && n_draws < pnp_get_iterations(0.0)) {
        suo_set_error("suo_pnp_replay: %d draws per object, the RANSAC loop may run %d iterations", n_draws, pnp_get_iterations(0.0));
        return SUO_ERR_ARG;
    }
    // limits and table indices are checked on the host before anything is staged: the whole call is refused, nothing is launched
    for (int o = 0; o < n_obj; ++o) {
        if (n_pts[o] < 0) { suo_set_error("suo_pnp_batch: negative point count"); return SUO_ERR_ARG; }
        if (n_pts[o] > PNP_MAX_POINTS) {
            suo_set_error("%s: object %d has %d points, the limit is %d per object", draws ? "suo_pnp_replay" : "suo_pnp_batch", o, n_pts[o], PNP_MAX_POINTS);
            return SUO_ERR_ARG;
        }
    }
    if (draws)
        for (int o = 0; o < n_obj; ++o) {
            const int* d = draws + 4 * (size_t)n_draws * o;
            if (n_pts[o] < 4) continue;                               // not solvable: the kernel never reads this object's rows
            for (size_t k = 0; k < 4 * (size_t)n_draws; ++k)        // (a repeated index within a row is a degenerate sample, not an error)
                if (d[k] < 0 || d[k] >= n_pts[o]) {
                    suo_set_error("suo_pnp_replay: object %d, row %d of the draw table holds index %d, the object has %d points", o, (int)(k / 4), d[k], n_pts[o]);
                    return SUO_ERR_ARG;
                }
        }
    std::lock_guard<std::mutex> lock(g_arena.mu);
    std::vector<int> offsets(n_obj + 1, 0), tab_off(n_obj, 0);
    std::vector<int> tab;
    for (int o = 0; o < n_obj; ++o) {
        if (n_pts[o] < 0) { suo_set_error("suo_pnp_batch: negative point count"); return SUO_ERR_ARG; }
        offsets[o + 1] = offsets[o] + n_pts[o];
        tab_off[o] = (int)tab.size();
        for (int b = 0; b <= n_pts[o]; ++b) tab.push_back(pnp_get_iterations(n_pts[o] > 0 ? b / (double)n_pts[o] : 0.0));
    }
    const int total = offsets[n_obj];
    Layout L;
    const size_t o_off = L.take(sizeof(int) * (n_obj + 1)), o_toff = L.take(sizeof(int) * n_obj), o_tab = L.take(sizeof(int) * tab.size());
    const size_t o_xs = L.take(sizeof(double) * 3 * (size_t)total), o_ys = L.take(sizeof(double) * 2 * (size_t)total);
    const size_t o_dr = L.take(draws ? sizeof(int) * 4 * (size_t)n_draws * n_obj : 0);
    const size_t in_bytes = L.off;
    const size_t o_T = L.take(sizeof(double) * 16 * (size_t)n_obj), o_st = L.take(sizeof(int) * n_obj), o_best = L.take(sizeof(int) * n_obj),
                 o_it = L.take(sizeof(int) * n_obj), o_win = L.take(sizeof(int) * n_obj);
    int rc = g_arena.ensure(L.off);
    if (rc != SUO_OK) return rc;
    char* h = g_arena.host;
    char* d = g_arena.dev;
    memcpy(h + o_off, offsets.data(), sizeof(int) * (n_obj + 1));
    memcpy(h + o_toff, tab_off.data(), sizeof(int) * n_obj);
    memcpy(h + o_tab, tab.data(), sizeof(int) * tab.size());
    memcpy(h + o_xs, xs, sizeof(double) * 3 * (size_t)total);
    memcpy(h + o_ys, ys, sizeof(double) * 2 * (size_t)total);
    if (draws) memcpy(h + o_dr, draws, sizeof(int) * 4 * (size_t)n_draws * n_obj);
    hipStream_t s = g_arena.stream;
    SUO_HIP_CHECK(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, s));
    if (draws)
        rc = launch_pnp_replay(n_obj, (const int*)(d + o_off), (const double*)(d + o_xs), (const double*)(d + o_ys), threshold, (const int*)(d + o_tab),
                               (const int*)(d + o_toff), do_refine, (const int*)(d + o_dr), n_draws, (double*)(d + o_T), (int*)(d + o_st), (int*)(d + o_best),
                               (int*)(d + o_it), (int*)(d + o_win), s);
    else
    rc = launch_pnp_batch(n_obj, (const int*)(d + o_off), (const double*)(d + o_xs), (const double*)(d + o_ys), threshold, seed,
                          (const int*)(d + o_tab), (const int*)(d + o_toff), do_refine, (double*)(d + o_T), (int*)(d + o_st),
                          (int*)(d + o_best), (int*)(d + o_it), s);
    if (rc != SUO_OK) return rc;
    SUO_HIP_CHECK(hipMemcpyAsync(h + o_T, d + o_T, L.off - o_T, hipMemcpyDeviceToHost, s));
    SUO_HIP_CHECK(hipStreamSynchronize(s));
    memcpy(T_out, h + o_T, sizeof(double) * 16 * (size_t)n_obj);
    if (status) memcpy(status, h + o_st, sizeof(int) * n_obj);
    if (best_inliers) memcpy(best_inliers, h + o_best, sizeof(int) * n_obj);
    if (iterations) memcpy(iterations, h + o_it, sizeof(int) * n_obj);
    if (winner && draws) memcpy(winner, h + o_win, sizeof(int) * n_obj);
    return SUO_OK;
}

int suo_pnp_batch(int n_obj, const int* n_pts, const double* xs, const double* ys, double threshold, uint64_t seed,
                  int do_refine, double* T_out, int* status, int* best_inliers, int* iterations) {
    return pnp_batch_impl(n_obj, n_pts, xs, ys, threshold, seed, nullptr, 0, do_refine, T_out, status, best_inliers, iterations, nullptr);
}

int suo_pnp_replay(int n_obj, const int* n_pts, const double* xs, const double* ys, double threshold, const int* draws, int n_draws, int do_refine,
                   double* T_out, int* status, int* best_inliers, int* iterations, int* winner) {
    if (!draws) { suo_set_error("suo_pnp_replay: draws is NULL"); return SUO_ERR_ARG; }
    return pnp_batch_impl(n_obj, n_pts, xs, ys, threshold, 0, draws, n_draws, do_refine, T_out, status, best_inliers, iterations, winner);
}

// Test entry: the refinement half of pnp_batch_kernel on its own (include/suo_hip.h).  Everything is checked before anything is allocated or launched.
int suo_debug_pnp_refine(int n_obj, const int* n_pts, const double* xs, const double* ys, double threshold, const int* mode, const double* start_qt,
                         const int* start_idx, const int* sel_in, const int* max_iter, const double* tol, double* out_d, int* out_i, int* sel0_out,
                         int* sel1_out) {
    if (n_obj <= 0) { suo_set_error("suo_debug_pnp_refine: n_obj = %d", n_obj); return SUO_ERR_ARG; }
    if (!n_pts || !xs || !ys || !mode || !start_qt || !start_idx || !sel_in || !max_iter || !tol || !out_d || !out_i || !sel0_out || !sel1_out) {
        suo_set_error("suo_debug_pnp_refine: null argument");
        return SUO_ERR_ARG;
    }
    std::vector<int> offsets((size_t)n_obj + 1, 0);
    for (int o = 0; o < n_obj; ++o) {
        const int n = n_pts[o];
        if (n < 0 || n > PNP_MAX_POINTS) {
            suo_set_error("suo_debug_pnp_refine: object %d has %d points, the limit is %d per object", o, n, PNP_MAX_POINTS);
            return SUO_ERR_ARG;
        }
        if (mode[o] != 0 && mode[o] != 1) { suo_set_error("suo_debug_pnp_refine: object %d, mode %d", o, mode[o]); return SUO_ERR_ARG; }
        if (mode[o] == 1 && (max_iter[o] < 0 || max_iter[o] > 50)) {
            suo_set_error("suo_debug_pnp_refine: object %d, max_iter %d (0 .. 50)", o, max_iter[o]);
            return SUO_ERR_ARG;
        }
        if (start_idx[4 * o] >= 0)
            for (int k = 0; k < 4; ++k)
                if (start_idx[4 * o + k] < 0 || start_idx[4 * o + k] >= n) {
                    suo_set_error("suo_debug_pnp_refine: object %d starts from point %d, it has %d points", o, start_idx[4 * o + k], n);
                    return SUO_ERR_ARG;
                }
        offsets[o + 1] = offsets[o] + n;
    }
    const size_t N = (size_t)n_obj, total = (size_t)offsets[n_obj], tp = total ? total : 1;
    Layout L;
    const size_t o_xs = L.take(sizeof(double) * 3 * tp), o_ys = L.take(sizeof(double) * 2 * tp), o_qt = L.take(sizeof(double) * 7 * N),
                 o_tol = L.take(sizeof(double) * N), o_off = L.take(sizeof(int) * (N + 1)), o_mode = L.take(sizeof(int) * N), o_idx = L.take(sizeof(int) * 4 * N),
                 o_sel = L.take(sizeof(int) * tp), o_mi = L.take(sizeof(int) * N);
    const size_t o_d = L.take(sizeof(double) * 88 * N), o_i = L.take(sizeof(int) * 8 * N), o_s0 = L.take(sizeof(int) * tp), o_s1 = L.take(sizeof(int) * tp);
    char* d = nullptr;
    SUO_HIP_CHECK(hipMalloc((void**)&d, L.off));
    struct Free { char* d; ~Free() { (void)hipFree(d); } } guard{d};
    SUO_HIP_CHECK(hipMemcpy(d + o_xs, xs, sizeof(double) * 3 * total, hipMemcpyHostToDevice));
    SUO_HIP_CHECK(hipMemcpy(d + o_ys, ys, sizeof(double) * 2 * total, hipMemcpyHostToDevice));
    SUO_HIP_CHECK(hipMemcpy(d + o_qt, start_qt, sizeof(double) * 7 * N, hipMemcpyHostToDevice));
    SUO_HIP_CHECK(hipMemcpy(d + o_tol, tol, sizeof(double) * N, hipMemcpyHostToDevice));
    SUO_HIP_CHECK(hipMemcpy(d + o_off, offsets.data(), sizeof(int) * (N + 1), hipMemcpyHostToDevice));
    SUO_HIP_CHECK(hipMemcpy(d + o_mode, mode, sizeof(int) * N, hipMemcpyHostToDevice));
    SUO_HIP_CHECK(hipMemcpy(d + o_idx, start_idx, sizeof(int) * 4 * N, hipMemcpyHostToDevice));
    SUO_HIP_CHECK(hipMemcpy(d + o_sel, sel_in, sizeof(int) * total, hipMemcpyHostToDevice));
    SUO_HIP_CHECK(hipMemcpy(d + o_mi, max_iter, sizeof(int) * N, hipMemcpyHostToDevice));
    int rc = launch_debug_pnp_refine(n_obj, (const int*)(d + o_off), (const double*)(d + o_xs), (const double*)(d + o_ys), threshold, (const int*)(d + o_mode),
                                     (const double*)(d + o_qt), (const int*)(d + o_idx), (const int*)(d + o_sel), (const int*)(d + o_mi),
                                     (const double*)(d + o_tol), (double*)(d + o_d), (int*)(d + o_i), (int*)(d + o_s0), (int*)(d + o_s1), nullptr);
    if (rc != SUO_OK) return rc;
    SUO_HIP_CHECK(hipDeviceSynchronize());
    SUO_HIP_CHECK(hipMemcpy(out_d, d + o_d, sizeof(double) * 88 * N, hipMemcpyDeviceToHost));
    SUO_HIP_CHECK(hipMemcpy(out_i, d + o_i, sizeof(int) * 8 * N, hipMemcpyDeviceToHost));
    SUO_HIP_CHECK(hipMemcpy(sel0_out, d + o_s0, sizeof(int) * total, hipMemcpyDeviceToHost));
    SUO_HIP_CHECK(hipMemcpy(sel1_out, d + o_s1, sizeof(int) * total, hipMemcpyDeviceToHost));
    return SUO_OK;
}

// Test entry: the minimal solver of pnp_batch_kernel on its own (include/suo_hip.h).  Everything is checked before anything is allocated or launched.
int suo_debug_p3p(int n, const double* xs, const double* ys, int* valid, double* R, double* t, double* qt, int* status) {
    if (n <= 0) { suo_set_error("suo_debug_p3p: n = %d", n); return SUO_ERR_ARG; }
    if (!xs || !ys || !valid || !R || !t || !qt || !status) { suo_set_error("suo_debug_p3p: null argument"); return SUO_ERR_ARG; }
    const size_t N = (size_t)n;
    Layout L;
    const size_t o_xs = L.take(sizeof(double) * 12 * N), o_ys = L.take(sizeof(double) * 8 * N);
    const size_t o_R = L.take(sizeof(double) * 36 * N), o_t = L.take(sizeof(double) * 12 * N), o_qt = L.take(sizeof(double) * 7 * N),
                 o_v = L.take(sizeof(int) * N), o_st = L.take(sizeof(int) * N);
    char* d = nullptr;
    SUO_HIP_CHECK(hipMalloc((void**)&d, L.off));
    struct Free { char* d; ~Free() { (void)hipFree(d); } } guard{d};
    SUO_HIP_CHECK(hipMemcpy(d + o_xs, xs, sizeof(double) * 12 * N, hipMemcpyHostToDevice));
    SUO_HIP_CHECK(hipMemcpy(d + o_ys, ys, sizeof(double) * 8 * N, hipMemcpyHostToDevice));
    int rc = launch_debug_p3p(n, (const double*)(d + o_xs), (const double*)(d + o_ys), (int*)(d + o_v), (double*)(d + o_R), (double*)(d + o_t),
                              (double*)(d + o_qt), (int*)(d + o_st), nullptr);
    if (rc != SUO_OK) return rc;
    SUO_HIP_CHECK(hipDeviceSynchronize());
    SUO_HIP_CHECK(hipMemcpy(R, d + o_R, sizeof(double) * 36 * N, hipMemcpyDeviceToHost));
    SUO_HIP_CHECK(hipMemcpy(t, d + o_t, sizeof(double) * 12 * N, hipMemcpyDeviceToHost));
    SUO_HIP_CHECK(hipMemcpy(qt, d + o_qt, sizeof(double) * 7 * N, hipMemcpyDeviceToHost));
    SUO_HIP_CHECK(hipMemcpy(valid, d + o_v, sizeof(int) * N, hipMemcpyDeviceToHost));
    SUO_HIP_CHECK(hipMemcpy(status, d + o_st, sizeof(int) * N, hipMemcpyDeviceToHost));
    return SUO_OK;
}

int suo_pnp(const double* xs, const double* ys, int n, double threshold, double* T_out) {
    int st = 0;
    return suo_pnp_batch(1, &n, xs, ys, threshold, 0, 1, T_out, &st, nullptr, nullptr);
}

}  // extern "C"
