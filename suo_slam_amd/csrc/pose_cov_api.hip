// Host-buffer entry points of the pose covariances (include/suo_hip.h: suo_pose_covariances / suo_pose_covariances_pairs / suo_pose_covariances_graph and their batch
// forms) and of suo_residual_statistics.  Each describes its request and goes through csrc/cov_stage.hip: plan, the problems staged through the arena of
// suo_optimize_batch with the covariance arrays riding beside them (one H2D), the chain of csrc/pose_cov.hip and csrc/pose_cov_graph.hip -- csrc/resid_stats.hip
// behind it for the residual entry --, one D2H of the output room, the scatter into the caller's buffers.  The caller's problem is read only.
#include <string.h>

#include "cov_stage.h"

using namespace suo;

// The shared body of the entries.  rq.pairs == nullptr: the marginal entry -- the coupled kernel without the pair work, no pair kernel, status [n][2].
// With pairs: the PAIRS instantiation, the pair kernel behind both, status [n][3]; cross / rel (one pointer per problem) and their members may be null.
static int cov_batch(const suo_ba_problem* probs, int n_prob, const CovRequest& rq, double* const* cam_cov, double* const* obj_cov, double* const* cross,
                     double* const* rel, int* status) {
    CovStaged cs;
    int rc = plan_cov_batch(probs, n_prob, rq, cs);
    if (rc != SUO_OK) return rc;
    std::lock_guard<std::mutex> lock(g_arena.mu);
    rc = stage_cov(probs, n_prob, rq, cs);
    if (rc == SUO_OK) rc = launch_cov_chain(rq, cs, n_prob);
    if (rc == SUO_OK) rc = fetch_cov(cs);
    if (rc != SUO_OK) return rc;
    const int ns = rq.pairs ? 3 : 2;
    for (int i = 0; i < n_prob; ++i) {
        const LmProblem& S = cs.st.prep[i].S;
        if (double* d = cov_buffer(cam_cov, i)) memcpy(d, g_arena.mirror(S.cam_cov), sizeof(double) * 36 * (size_t)S.n_cam);
        if (double* d = cov_buffer(obj_cov, i)) memcpy(d, g_arena.mirror(S.obj_cov), sizeof(double) * 36 * (size_t)S.n_obj);
        if (double* d = cov_buffer(cross, i)) memcpy(d, g_arena.mirror(S.cov_cross), sizeof(double) * 36 * (size_t)S.n_cpair);
        if (double* d = cov_buffer(rel, i)) memcpy(d, g_arena.mirror(S.cov_rel), sizeof(double) * 36 * (size_t)S.n_cpair);
        if (status) memcpy(status + ns * i, g_arena.mirror(S.cov_status), sizeof(int) * ns);
    }
    return SUO_OK;
}

// suo_residual_statistics: the graph entry's plan and chain, asked for Sigma_co of every problem's own (camera, object) pairs; csrc/resid_stats.hip behind them
extern "C" int suo_residual_statistics_batch(const suo_ba_problem* probs, int n_prob, double* const* cam_cov, double* const* obj_cov, double* const* edge_chi2,
                                             double* const* edge_pcov, double* const* edge_lev, double* const* edge_t, double* const* cam_stat,
                                             double* const* obj_stat, double* summary, int* status) {
    if (n_prob <= 0) return SUO_OK;
    if (!probs) { suo_set_error("suo_residual_statistics_batch: null argument"); return SUO_ERR_ARG; }
    const CovRequest rq{"suo_residual_statistics", true, nullptr, true};          // the graph entry's plan, and resid
    CovStaged cs;
    int rc = plan_cov_batch(probs, n_prob, rq, cs);
    if (rc != SUO_OK) return rc;
    std::lock_guard<std::mutex> lock(g_arena.mu);
    rc = stage_cov(probs, n_prob, rq, cs);
    if (rc == SUO_OK) rc = launch_cov_chain(rq, cs, n_prob);
    if (rc == SUO_OK) rc = launch_resid_stats(cs.problems(), cs.rs_dev, n_prob, cs.plan.max_edges, cs.plan.max_vertices, g_arena.stream);
    if (rc == SUO_OK) rc = fetch_cov(cs);
    if (rc != SUO_OK) return rc;
    for (int i = 0; i < n_prob; ++i) {
        const LmProblem& S = cs.st.prep[i].S;
        const RsProblem& R = g_arena.mirror(cs.rs_dev)[i];
        const size_t E = S.n_edge, C = S.n_cam, O = S.n_obj;
        if (double* d = cov_buffer(cam_cov, i)) memcpy(d, g_arena.mirror(S.cam_cov), sizeof(double) * 36 * C);
        if (double* d = cov_buffer(obj_cov, i)) memcpy(d, g_arena.mirror(S.obj_cov), sizeof(double) * 36 * O);
        if (double* d = cov_buffer(edge_chi2, i)) memcpy(d, g_arena.mirror(R.chi2), sizeof(double) * E);
        if (double* d = cov_buffer(edge_pcov, i)) memcpy(d, g_arena.mirror(R.pcov), sizeof(double) * 3 * E);
        if (double* d = cov_buffer(edge_lev, i)) memcpy(d, g_arena.mirror(R.lev), sizeof(double) * E);
        if (double* d = cov_buffer(edge_t, i)) memcpy(d, g_arena.mirror(R.t), sizeof(double) * E);
        if (double* d = cov_buffer(cam_stat, i)) memcpy(d, g_arena.mirror(R.vstat), sizeof(double) * 3 * C);
        if (double* d = cov_buffer(obj_stat, i)) memcpy(d, g_arena.mirror(R.vstat) + 3 * C, sizeof(double) * 3 * O);
        if (summary) memcpy(summary + 6 * (size_t)i, g_arena.mirror(R.summary), sizeof(double) * 6);
        if (status) {
            memcpy(status + 4 * (size_t)i, g_arena.mirror(S.cov_status), sizeof(int) * 2);
            memcpy(status + 4 * (size_t)i + 2, g_arena.mirror(R.status), sizeof(int) * 2);
        }
    }
    return SUO_OK;
}

extern "C" {

int suo_residual_statistics(const suo_ba_problem* problem, double* cam_cov, double* obj_cov, double* edge_chi2, double* edge_pcov, double* edge_lev, double* edge_t,
                            double* cam_stat, double* obj_stat, double* summary, int* status) {
    if (!problem) { suo_set_error("suo_residual_statistics: null argument"); return SUO_ERR_ARG; }
    return suo_residual_statistics_batch(problem, 1, &cam_cov, &obj_cov, &edge_chi2, &edge_pcov, &edge_lev, &edge_t, &cam_stat, &obj_stat, summary, status);
}

int suo_pose_covariances_batch(const suo_ba_problem* probs, int n_prob, double* const* cam_cov, double* const* obj_cov, int* status) {
    if (n_prob <= 0) return SUO_OK;
    if (!probs || !cam_cov || !obj_cov) { suo_set_error("suo_pose_covariances_batch: null argument"); return SUO_ERR_ARG; }
    return cov_batch(probs, n_prob, CovRequest{"suo_pose_covariances"}, cam_cov, obj_cov, nullptr, nullptr, status);
}

int suo_pose_covariances(const suo_ba_problem* problem, double* cam_cov, double* obj_cov, int* status) {
    if (!problem) { suo_set_error("suo_pose_covariances: null argument"); return SUO_ERR_ARG; }
    return suo_pose_covariances_batch(problem, 1, &cam_cov, &obj_cov, status);
}

int suo_pose_covariances_pairs_batch(const suo_ba_problem* probs, int n_prob, const int* n_pair, const int32_t* const* pair_a, const int32_t* const* pair_b,
                                     double* const* cam_cov, double* const* obj_cov, double* const* cross, double* const* rel, int* status) {
    if (n_prob <= 0) return SUO_OK;
    if (!probs || !n_pair || !pair_a || !pair_b) { suo_set_error("suo_pose_covariances_pairs_batch: null argument"); return SUO_ERR_ARG; }
    const CovPairs pairs{n_pair, pair_a, pair_b};
    return cov_batch(probs, n_prob, CovRequest{"suo_pose_covariances_pairs", false, &pairs}, cam_cov, obj_cov, cross, rel, status);
}

int suo_pose_covariances_pairs(const suo_ba_problem* problem, int n_pair, const int32_t* pair_a, const int32_t* pair_b, double* cam_cov, double* obj_cov, double* cross,
                               double* rel, int* status) {
    if (!problem) { suo_set_error("suo_pose_covariances_pairs: null argument"); return SUO_ERR_ARG; }
    return suo_pose_covariances_pairs_batch(problem, 1, &n_pair, &pair_a, &pair_b, &cam_cov, &obj_cov, &cross, &rel, status);
}

int suo_pose_covariances_graph_batch(const suo_ba_problem* probs, int n_prob, const int* n_pair, const int32_t* const* pair_a, const int32_t* const* pair_b,
                                     double* const* cam_cov, double* const* obj_cov, double* const* cross, double* const* rel, int* status) {
    if (n_prob <= 0) return SUO_OK;
    if (!probs || !n_pair || !pair_a || !pair_b) { suo_set_error("suo_pose_covariances_graph_batch: null argument"); return SUO_ERR_ARG; }
    const CovPairs pairs{n_pair, pair_a, pair_b};
    return cov_batch(probs, n_prob, CovRequest{"suo_pose_covariances_graph", true, &pairs}, cam_cov, obj_cov, cross, rel, status);
}

int suo_pose_covariances_graph(const suo_ba_problem* problem, int n_pair, const int32_t* pair_a, const int32_t* pair_b, double* cam_cov, double* obj_cov, double* cross,
                               double* rel, int* status) {
    if (!problem) { suo_set_error("suo_pose_covariances_graph: null argument"); return SUO_ERR_ARG; }
    return suo_pose_covariances_graph_batch(problem, 1, &n_pair, &pair_a, &pair_b, &cam_cov, &obj_cov, &cross, &rel, status);
}

}  // extern "C"
