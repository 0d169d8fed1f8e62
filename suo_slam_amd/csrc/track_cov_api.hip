// Host-buffer entry points of the tracking covariances (include/suo_hip.h: suo_tracking_covariances and its batch form): through csrc/cov_stage.hip as problems
// of cov_form 1, the map's covariance and the TcProblem outputs in the covariance rooms beside them; the problems and the map in an H2D each, pose_cov_diag_kernel
// (csrc/pose_cov.hip) for Hcc^-1, track_cov_kernel (csrc/track_cov.hip) behind it, one D2H.  What is this entry's own: its size check and refusals, and the staged
// copy's edge_inlier, with the edges of the objects that are not in the map taken out.  The caller's problem is read only.
#include <math.h>
#include <string.h>

#include "cov_stage.h"

using namespace suo;

extern "C" int suo_tracking_covariances_batch(const suo_ba_problem* probs, int n_prob, const double* const* map_cov, double* const* cam_cov,
                                              double* const* fixed_map_cov, double* const* cross, double* const* rel, int* status) {
    if (n_prob <= 0) return SUO_OK;
    if (!probs) { suo_set_error("suo_tracking_covariances_batch: null argument"); return SUO_ERR_ARG; }
    std::vector<suo_ba_problem> staged(probs, probs + n_prob);
    std::vector<std::vector<uint8_t>> inlier(n_prob), in_map(n_prob);
    std::vector<int> n_out_of_map(n_prob, 0);
    const CovRequest rq{"suo_tracking_covariances", false, nullptr, false, map_cov, in_map.data()};
    const char* who = rq.who;
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
    }
    CovStaged cs;
    int rc = plan_cov_batch(probs, n_prob, rq, cs);          // form 1 throughout; prepared: the edges' vertices exist from here on
    if (rc != SUO_OK) return rc;
    for (int i = 0; i < n_prob; ++i) {
        const suo_ba_problem& q = probs[i];
        inlier[i].resize(q.n_edge);
        for (int e = 0; e < q.n_edge; ++e) inlier[i][e] = (q.edge_inlier[e] != 0 && in_map[i][q.edge_obj[e]]) ? 1 : 0;
        staged[i].edge_inlier = inlier[i].data();
    }
    std::lock_guard<std::mutex> lock(g_arena.mu);
    rc = stage_cov(staged.data(), n_prob, rq, cs);
    if (rc == SUO_OK) rc = launch_cov_chain(rq, cs, n_prob);
    if (rc == SUO_OK) rc = launch_track_cov(cs.problems(), cs.tc_dev, n_prob, cs.plan.max_cam, cs.plan.max_obj, g_arena.stream);
    if (rc == SUO_OK) rc = fetch_cov(cs);
    if (rc != SUO_OK) return rc;
    for (int i = 0; i < n_prob; ++i) {
        const LmProblem& S = cs.st.prep[i].S;
        const TcProblem& T = g_arena.mirror(cs.tc_dev)[i];
        const size_t C = S.n_cam, O = S.n_obj;
        if (double* d = cov_buffer(fixed_map_cov, i)) memcpy(d, g_arena.mirror(S.cam_cov), sizeof(double) * 36 * C);
        if (double* d = cov_buffer(cam_cov, i)) memcpy(d, g_arena.mirror(T.cam_cov), sizeof(double) * 36 * C);
        if (double* d = cov_buffer(cross, i)) memcpy(d, g_arena.mirror(T.cross), sizeof(double) * 36 * C * O);
        if (double* d = cov_buffer(rel, i)) memcpy(d, g_arena.mirror(T.rel), sizeof(double) * 36 * C * O);
        if (status) { status[2 * i] = g_arena.mirror(S.cov_status)[0]; status[2 * i + 1] = n_out_of_map[i]; }
    }
    return SUO_OK;
}

extern "C" int suo_tracking_covariances(const suo_ba_problem* problem, const double* map_cov, double* cam_cov, double* fixed_map_cov, double* cross, double* rel, int* status) {
    if (!problem) { suo_set_error("suo_tracking_covariances: null argument"); return SUO_ERR_ARG; }
    return suo_tracking_covariances_batch(problem, 1, &map_cov, &cam_cov, &fixed_map_cov, &cross, &rel, status);
}
