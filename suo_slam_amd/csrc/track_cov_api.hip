// Host-buffer entry points of the tracking covariances (include/suo_hip.h: suo_tracking_covariances and its batch form): staged through the arena of
// suo_optimize_batch (csrc/ba_stage.hip) as problems of cov_form 1, the map's covariance and the outputs in the `extra` room behind the scratch; one H2D of the
// problems, one of the maps, pose_cov_diag_kernel (csrc/pose_cov.hip) for Hcc^-1, track_cov_kernel (csrc/track_cov.hip) behind it, two D2H.  The caller's
// problem is read only: the staged copy carries its own edge_inlier, with the edges of the objects that are not in the map taken out.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "ba_stage.h"
#include "track_cov.h"

using namespace suo;

struct TrackOut { double* const* cam_cov; double* const* fixed_map_cov; double* const* cross; double* const* rel; int* status; };

static int track_batch(const suo_ba_problem* probs, int n_prob, const double* const* map_cov, const TrackOut& out) {
    const char* who = "suo_tracking_covariances";
    std::vector<suo_ba_problem> staged(probs, probs + n_prob);
    std::vector<std::vector<uint8_t>> inlier(n_prob), in_map(n_prob);
    std::vector<int> form(n_prob, 1), n_out_of_map(n_prob, 0);
    int max_cam = 0, max_obj = 0;
    for (int i = 0; i < n_prob; ++i) {
        const suo_ba_problem& q = probs[i];
        if (q.n_cam < 0 || q.n_obj < 0 || q.n_edge < 0 || (q.n_cam > 0 && (!q.cam_fixed || !q.cam_T)) || (q.n_obj > 0 && (!q.obj_fixed || !q.obj_T)) ||
            (q.n_edge > 0 && (!q.edge_cam || !q.edge_obj || !q.edge_inlier))) {
            suo_set_error("%s: bad sizes or null arrays in problem %d", who, i);
            return SUO_ERR_ARG;
        }
        for (int o = 0; o < q.n_obj; ++o)
            if (!q.obj_fixed[o]) {
                suo_set_error("%s: object %d of problem %d is free; the tracking graph holds every object fixed at its map pose", who, o, i);
                return SUO_ERR_ARG;
            }
        if (q.n_obj > POSE_COV_GRAPH_MAX_OBJ) {
            suo_set_error("%s: problem %d has %d objects; the entry takes at most %d", who, i, q.n_obj, POSE_COV_GRAPH_MAX_OBJ);
            return SUO_ERR_ARG;
        }
        if (q.n_obj > 0 && (!map_cov || !map_cov[i])) { suo_set_error("%s: null map_cov for problem %d", who, i); return SUO_ERR_ARG; }
        const size_t ns = 6 * (size_t)q.n_obj;
        in_map[i].resize(q.n_obj);
        for (int o = 0; o < q.n_obj; ++o) {
            in_map[i][o] = isnan(map_cov[i][(6 * (size_t)o) * ns + 6 * (size_t)o]) ? 0 : 1;
            n_out_of_map[i] += in_map[i][o] ? 0 : 1;
        }
        inlier[i].resize(q.n_edge);
        for (int e = 0; e < q.n_edge; ++e) {
            if (q.edge_cam[e] < 0 || q.edge_cam[e] >= q.n_cam || q.edge_obj[e] < 0 || q.edge_obj[e] >= q.n_obj) {
                suo_set_error("%s: edge %d of problem %d references a missing vertex", who, e, i);
                return SUO_ERR_ARG;
            }
            inlier[i][e] = (q.edge_inlier[e] != 0 && in_map[i][q.edge_obj[e]]) ? 1 : 0;
        }
        staged[i].edge_inlier = inlier[i].data();
        max_cam = std::max(max_cam, q.n_cam);
        max_obj = std::max(max_obj, q.n_obj);
    }
    // the extra room: [TcProblem structs | every problem's sigma, in_map | in_end: every problem's cam_cov, cross, rel | out_end], offsets from Staged::o_extra
    std::vector<TcProblem> tc(n_prob);
    size_t x_in_end = 0, x_out_end = 0;
    auto lay_out = [&](char* base) {
        Layout L;
        auto put = [&](auto*& p, size_t n) { p = (std::remove_reference_t<decltype(p)>)((uintptr_t)base + L.take(sizeof(*p) * n)); };
        (void)L.take(sizeof(TcProblem) * (size_t)n_prob);
        for (int i = 0; i < n_prob; ++i) { const size_t ns = 6 * (size_t)probs[i].n_obj; put(tc[i].sigma, ns * ns); put(tc[i].in_map, (size_t)probs[i].n_obj); }
        x_in_end = L.off;
        for (int i = 0; i < n_prob; ++i) {
            const size_t C = probs[i].n_cam, O = probs[i].n_obj;
            put(tc[i].cam_cov, 36 * C); put(tc[i].cross, 36 * C * O); put(tc[i].rel, 36 * C * O);
        }
        x_out_end = L.off;
    };
    lay_out(nullptr);
    std::lock_guard<std::mutex> lock(g_arena.mu);
    Staged st;
    int rc = stage_problems(staged.data(), n_prob, g_arena, st, who, form.data(), nullptr, false, x_out_end);
    if (rc != SUO_OK) return rc;
    char* xdev = g_arena.dev + st.o_extra;       // (16-byte aligned: Layout::take)
    lay_out(xdev);
    for (int i = 0; i < n_prob; ++i) {
        const int O = probs[i].n_obj;
        const size_t ns = 6 * (size_t)O;
        double* S = g_arena.mirror(tc[i].sigma);
        const double* M = map_cov ? map_cov[i] : nullptr;
        const uint8_t* in = in_map[i].data();
        for (size_t r = 0; r < ns; ++r)
            for (size_t c = r; c < ns; ++c) {
                const double v = (in[r / 6] && in[c / 6]) ? M[r * ns + c] : 0.0;
                S[r * ns + c] = v; S[c * ns + r] = v;
            }
        memcpy(g_arena.mirror(tc[i].in_map), in, (size_t)O);
        memcpy(g_arena.host + st.o_extra + sizeof(TcProblem) * (size_t)i, &tc[i], sizeof(TcProblem));
    }
    hipStream_t s = g_arena.stream;
    SUO_HIP_CHECK(hipMemcpyAsync(xdev, g_arena.host + st.o_extra, x_in_end, hipMemcpyHostToDevice, s));
    const void* P = g_arena.dev + st.o_structs;
    rc = launch_pose_cov_diag(P, n_prob, s);
    if (rc != SUO_OK) return rc;
    rc = launch_track_cov(P, xdev, n_prob, max_cam, max_obj, s);
    if (rc != SUO_OK) return rc;
    SUO_HIP_CHECK(hipMemcpyAsync(g_arena.host + st.cov_begin, g_arena.dev + st.cov_begin, st.cov_end - st.cov_begin, hipMemcpyDeviceToHost, s));
    if (x_out_end > x_in_end)
        SUO_HIP_CHECK(hipMemcpyAsync(g_arena.host + st.o_extra + x_in_end, xdev + x_in_end, x_out_end - x_in_end, hipMemcpyDeviceToHost, s));
    SUO_HIP_CHECK(hipStreamSynchronize(s));
    auto member = [&](double* const* list, int i) { return list ? list[i] : nullptr; };
    for (int i = 0; i < n_prob; ++i) {
        const LmProblem& S = st.prep[i].S;
        const size_t C = S.n_cam, O = S.n_obj;
        if (double* d = member(out.fixed_map_cov, i)) memcpy(d, g_arena.mirror(S.cam_cov), sizeof(double) * 36 * C);
        if (double* d = member(out.cam_cov, i)) memcpy(d, g_arena.mirror(tc[i].cam_cov), sizeof(double) * 36 * C);
        if (double* d = member(out.cross, i)) memcpy(d, g_arena.mirror(tc[i].cross), sizeof(double) * 36 * C * O);
        if (double* d = member(out.rel, i)) memcpy(d, g_arena.mirror(tc[i].rel), sizeof(double) * 36 * C * O);
        if (out.status) { out.status[2 * i] = g_arena.mirror(S.cov_status)[0]; out.status[2 * i + 1] = n_out_of_map[i]; }
    }
    return SUO_OK;
}

extern "C" {

int suo_tracking_covariances_batch(const suo_ba_problem* probs, int n_prob, const double* const* map_cov, double* const* cam_cov, double* const* fixed_map_cov,
                                   double* const* cross, double* const* rel, int* status) {
    if (n_prob <= 0) return SUO_OK;
    if (!probs) { suo_set_error("suo_tracking_covariances_batch: null argument"); return SUO_ERR_ARG; }
    return track_batch(probs, n_prob, map_cov, TrackOut{cam_cov, fixed_map_cov, cross, rel, status});
}

int suo_tracking_covariances(const suo_ba_problem* problem, const double* map_cov, double* cam_cov, double* fixed_map_cov, double* cross, double* rel, int* status) {
    if (!problem) { suo_set_error("suo_tracking_covariances: null argument"); return SUO_ERR_ARG; }
    return suo_tracking_covariances_batch(problem, 1, &map_cov, &cam_cov, &fixed_map_cov, &cross, &rel, status);
}

}  // extern "C"
