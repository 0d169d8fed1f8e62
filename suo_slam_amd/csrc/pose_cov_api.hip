// Host-buffer entry points of the pose covariances (include/suo_hip.h: suo_pose_covariances / suo_pose_covariances_pairs / suo_pose_covariances_graph and their batch
// forms): staged through the arena of suo_optimize_batch (csrc/ba_stage.hip), one H2D, the kernels of csrc/pose_cov.hip and csrc/pose_cov_graph.hip, one D2H of the
// blocks.  The caller's problem is read only.  suo_residual_statistics goes the same way with csrc/resid_stats.hip behind the covariance kernels.
#include <string.h>

#include <algorithm>

#include "ba_stage.h"

using namespace suo;

static_assert(POSE_COV_GRAPH_MAX_OBJ == SUO_POSE_COV_GRAPH_MAX_OBJ, "the cap the header documents");

// Which kernel of csrc/pose_cov.hip takes every problem of the batch, decided ONCE, on the host (the counterpart of csrc/ba_api.hip: plan_ba_batch).
// A problem's form depends on that problem alone, so a batch gives every member the bits it gets alone.
struct CovPlan {
    std::vector<int> form;           // LmProblem::cov_form: 0 no free camera, 1 no free object (and a free camera), 2 coupled in LDS, 3 coupled in device memory
    bool diag = false, coupled = false, graph = false;
    int max_free_obj = 0;            // over the form-2 problems: sizes the reduced system's LDS
    int graph_free_obj = 0, graph_cam = 0;      // over the form-3 problems: size the grids of csrc/pose_cov_graph.hip
};
// graph (the suo_pose_covariances_graph entries): a coupled problem the old entries answer -- at most 16 free objects, no (camera, camera) pair -- keeps form 2 and
// with it their bits; every other coupled problem takes form 3, up to POSE_COV_GRAPH_MAX_OBJ free objects.  The old entries refuse what form 2 does not hold.
static int plan_cov_batch(const suo_ba_problem* probs, int n_prob, CovPlan& plan, bool graph = false, const CovPairs* pairs = nullptr) {
    plan.form.assign(n_prob, 0);
    for (int i = 0; i < n_prob; ++i) {
        const suo_ba_problem& q = probs[i];
        if (q.n_cam < 0 || q.n_obj < 0 || q.n_edge < 0 || (q.n_cam > 0 && !q.cam_fixed) || (q.n_obj > 0 && !q.obj_fixed)) {
            suo_set_error("suo_pose_covariances: bad sizes or null flags in problem %d", i);
            return SUO_ERR_ARG;
        }
        int nfo = 0, nfc = 0;
        for (int o = 0; o < q.n_obj; ++o) nfo += q.obj_fixed[o] ? 0 : 1;
        for (int c = 0; c < q.n_cam; ++c) nfc += q.cam_fixed[c] ? 0 : 1;
        if (nfc == 0) { plan.form[i] = 0; plan.diag = true; continue; }
        if (nfo == 0) { plan.form[i] = 1; plan.diag = true; continue; }
        if (graph) {
            bool cam_cam = false;
            // (the lists are validated behind the plan, as for the old entries: only compare here)
            for (int k = 0; pairs && pairs->a[i] && pairs->b[i] && !cam_cam && k < pairs->n[i]; ++k) cam_cam = pairs->a[i][k] < q.n_cam && pairs->b[i][k] < q.n_cam;
            if (nfo > POSE_COV_GRAPH_MAX_OBJ) {
                suo_set_error("suo_pose_covariances_graph: problem %d has %d free objects next to %d free cameras; the device-memory form takes at most %d", i, nfo, nfc,
                              POSE_COV_GRAPH_MAX_OBJ);
                return SUO_ERR_ARG;
            }
            if (cam_cam || nfo > LM_MAX_SCHUR_OBJ) {
                plan.form[i] = 3; plan.graph = true;
                plan.graph_free_obj = std::max(plan.graph_free_obj, nfo);
                plan.graph_cam = std::max(plan.graph_cam, q.n_cam);
                continue;
            }
        }
        if (nfo > LM_MAX_SCHUR_OBJ) {
            suo_set_error("suo_pose_covariances: problem %d has %d free objects next to %d free cameras; the coupled form keeps the reduced system and its inverse "
                          "in LDS and takes at most %d", i, nfo, nfc, LM_MAX_SCHUR_OBJ);
            return SUO_ERR_ARG;
        }
        plan.form[i] = 2; plan.coupled = true;
        plan.max_free_obj = std::max(plan.max_free_obj, nfo);
    }
    return SUO_OK;
}

// The shared body of the entries.  pairs == nullptr: the marginal entry -- the coupled kernel without the pair work, no pair kernel, status [n][2].
// With pairs: the PAIRS instantiation, the pair kernel behind both, status [n][3]; cross / rel (one pointer per problem) and their members may be null.
// graph: the suo_pose_covariances_graph entries -- (camera, camera) pairs are served and coupled problems may take form 3.
static int cov_batch(const suo_ba_problem* probs, int n_prob, double* const* cam_cov, double* const* obj_cov, int* status, const CovPairs* pairs, double* const* cross,
                     double* const* rel, const char* who, bool graph = false) {
    CovPlan plan;
    int rc = plan_cov_batch(probs, n_prob, plan, graph, pairs);
    if (rc != SUO_OK) return rc;
    for (int i = 0; pairs && i < n_prob; ++i) {
        const int n = pairs->n[i], nc = probs[i].n_cam, nv = probs[i].n_cam + probs[i].n_obj;
        if (n < 0 || (n > 0 && (!pairs->a[i] || !pairs->b[i]))) { suo_set_error("%s: problem %d: n_pair = %d or null pair lists", who, i, n); return SUO_ERR_ARG; }
        for (int q = 0; q < n; ++q) {
            const int a = pairs->a[i][q], b = pairs->b[i][q];
            if (a < 0 || a >= nv || b < 0 || b >= nv) { suo_set_error("%s: problem %d: pair %d = (%d, %d) names a vertex outside [0, %d)", who, i, q, a, b, nv); return SUO_ERR_ARG; }
            if (!graph && a < nc && b < nc) { suo_set_error("%s: problem %d: pair %d = (%d, %d) is (camera, camera); pairs are (camera, object) or (object, object)", who, i, q, a, b); return SUO_ERR_ARG; }
        }
    }
    std::lock_guard<std::mutex> lock(g_arena.mu);
    Staged st;
    rc = stage_problems(probs, n_prob, g_arena, st, who, plan.form.data(), pairs);
    if (rc != SUO_OK) return rc;
    const void* P = g_arena.dev + st.o_structs;
    hipStream_t s = g_arena.stream;
    if (plan.diag) { rc = launch_pose_cov_diag(P, n_prob, s); if (rc != SUO_OK) return rc; }
    if (plan.coupled) { rc = launch_pose_cov_coupled(P, n_prob, plan.max_free_obj, s, pairs != nullptr); if (rc != SUO_OK) return rc; }
    if (plan.graph) { rc = launch_pose_cov_graph(P, n_prob, plan.graph_free_obj, plan.graph_cam, *std::max_element(pairs->n, pairs->n + n_prob), s); if (rc != SUO_OK) return rc; }
    if (pairs) { rc = launch_pose_cov_pairs(P, n_prob, *std::max_element(pairs->n, pairs->n + n_prob), s); if (rc != SUO_OK) return rc; }
    SUO_HIP_CHECK(hipMemcpyAsync(g_arena.host + st.cov_begin, g_arena.dev + st.cov_begin, st.cov_end - st.cov_begin, hipMemcpyDeviceToHost, s));
    SUO_HIP_CHECK(hipStreamSynchronize(s));
    const int ns = pairs ? 3 : 2;
    for (int i = 0; i < n_prob; ++i) {
        const LmProblem& S = st.prep[i].S;
        if (cam_cov && cam_cov[i]) memcpy(cam_cov[i], g_arena.mirror(S.cam_cov), sizeof(double) * 36 * (size_t)S.n_cam);
        if (obj_cov && obj_cov[i]) memcpy(obj_cov[i], g_arena.mirror(S.obj_cov), sizeof(double) * 36 * (size_t)S.n_obj);
        if (cross && cross[i]) memcpy(cross[i], g_arena.mirror(S.cov_cross), sizeof(double) * 36 * (size_t)S.n_cpair);
        if (rel && rel[i]) memcpy(rel[i], g_arena.mirror(S.cov_rel), sizeof(double) * 36 * (size_t)S.n_cpair);
        if (status) memcpy(status + ns * i, g_arena.mirror(S.cov_status), sizeof(int) * ns);
    }
    return SUO_OK;
}

// suo_residual_statistics: the graph entry's plan, staging and launches, asked for the cross blocks of every problem's own (camera, object) pairs -- in the order
// prep_problem deals them (by camera, then by object), so that pair p of the staged problem is pair p of the request -- and csrc/resid_stats.hip behind them.
// Forms 0 and 1 couple nothing (Sigma_co = 0): they get no pairs.
struct ResidOut {
    double* const* cam_cov; double* const* obj_cov; double* const* chi2; double* const* pcov; double* const* lev; double* const* t; double* const* cam_stat;
    double* const* obj_stat; double* summary; int* status;
};
static int resid_batch(const suo_ba_problem* probs, int n_prob, const ResidOut& out) {
    const char* who = "suo_residual_statistics";
    CovPlan plan;
    int rc = plan_cov_batch(probs, n_prob, plan, true);
    if (rc != SUO_OK) return rc;
    std::vector<std::vector<int32_t>> pa(n_prob), pb(n_prob);
    std::vector<int> np(n_prob, 0);
    std::vector<const int32_t*> pa_ptr(n_prob), pb_ptr(n_prob);
    int max_pairs = 0, max_edges = 0, max_vertices = 0;
    for (int i = 0; i < n_prob; ++i) {
        const suo_ba_problem& q = probs[i];
        max_edges = std::max(max_edges, q.n_edge);
        max_vertices = std::max(max_vertices, q.n_cam + q.n_obj);
        if (plan.form[i] >= 2) {
            if (q.n_edge > 0 && (!q.edge_cam || !q.edge_obj)) { suo_set_error("%s: null edge lists in problem %d", who, i); return SUO_ERR_ARG; }
            std::vector<uint8_t> seen((size_t)q.n_cam * q.n_obj, 0);
            for (int e = 0; e < q.n_edge; ++e) {
                if (q.edge_cam[e] < 0 || q.edge_cam[e] >= q.n_cam || q.edge_obj[e] < 0 || q.edge_obj[e] >= q.n_obj) {
                    suo_set_error("%s: edge %d of problem %d references a missing vertex", who, e, i);
                    return SUO_ERR_ARG;
                }
                seen[(size_t)q.edge_cam[e] * q.n_obj + q.edge_obj[e]] = 1;
            }
            for (int c = 0; c < q.n_cam; ++c)
                for (int o = 0; o < q.n_obj; ++o)
                    if (seen[(size_t)c * q.n_obj + o]) { pa[i].push_back(c); pb[i].push_back(q.n_cam + o); }
        }
        np[i] = (int)pa[i].size(); pa_ptr[i] = pa[i].data(); pb_ptr[i] = pb[i].data();
        max_pairs = std::max(max_pairs, np[i]);
    }
    const CovPairs pairs{np.data(), pa_ptr.data(), pb_ptr.data()};
    std::lock_guard<std::mutex> lock(g_arena.mu);
    Staged st;
    rc = stage_problems(probs, n_prob, g_arena, st, who, plan.form.data(), &pairs, true);
    if (rc != SUO_OK) return rc;
    const void* P = g_arena.dev + st.o_structs;
    hipStream_t s = g_arena.stream;
    if (plan.diag) { rc = launch_pose_cov_diag(P, n_prob, s); if (rc != SUO_OK) return rc; }
    if (plan.coupled) { rc = launch_pose_cov_coupled(P, n_prob, plan.max_free_obj, s, true); if (rc != SUO_OK) return rc; }
    if (plan.graph) { rc = launch_pose_cov_graph(P, n_prob, plan.graph_free_obj, plan.graph_cam, max_pairs, s); if (rc != SUO_OK) return rc; }
    if (max_pairs > 0) { rc = launch_pose_cov_pairs(P, n_prob, max_pairs, s); if (rc != SUO_OK) return rc; }
    rc = launch_resid_stats(P, g_arena.dev + st.o_rs, n_prob, max_edges, max_vertices, s);
    if (rc != SUO_OK) return rc;
    SUO_HIP_CHECK(hipMemcpyAsync(g_arena.host + st.cov_begin, g_arena.dev + st.cov_begin, st.cov_end - st.cov_begin, hipMemcpyDeviceToHost, s));
    SUO_HIP_CHECK(hipStreamSynchronize(s));
    auto member = [&](double* const* list, int i) { return list ? list[i] : nullptr; };
    for (int i = 0; i < n_prob; ++i) {
        const LmProblem& S = st.prep[i].S;
        const RsProblem& R = st.prep[i].R;
        const size_t E = S.n_edge, C = S.n_cam, O = S.n_obj;
        if (double* d = member(out.cam_cov, i)) memcpy(d, g_arena.mirror(S.cam_cov), sizeof(double) * 36 * C);
        if (double* d = member(out.obj_cov, i)) memcpy(d, g_arena.mirror(S.obj_cov), sizeof(double) * 36 * O);
        if (double* d = member(out.chi2, i)) memcpy(d, g_arena.mirror(R.chi2), sizeof(double) * E);
        if (double* d = member(out.pcov, i)) memcpy(d, g_arena.mirror(R.pcov), sizeof(double) * 3 * E);
        if (double* d = member(out.lev, i)) memcpy(d, g_arena.mirror(R.lev), sizeof(double) * E);
        if (double* d = member(out.t, i)) memcpy(d, g_arena.mirror(R.t), sizeof(double) * E);
        if (double* d = member(out.cam_stat, i)) memcpy(d, g_arena.mirror(R.vstat), sizeof(double) * 3 * C);
        if (double* d = member(out.obj_stat, i)) memcpy(d, g_arena.mirror(R.vstat) + 3 * C, sizeof(double) * 3 * O);
        if (out.summary) memcpy(out.summary + 6 * (size_t)i, g_arena.mirror(R.summary), sizeof(double) * 6);
        if (out.status) {
            memcpy(out.status + 4 * (size_t)i, g_arena.mirror(S.cov_status), sizeof(int) * 2);
            memcpy(out.status + 4 * (size_t)i + 2, g_arena.mirror(R.status), sizeof(int) * 2);
        }
    }
    return SUO_OK;
}

extern "C" {

int suo_residual_statistics_batch(const suo_ba_problem* probs, int n_prob, double* const* cam_cov, double* const* obj_cov, double* const* edge_chi2,
                                  double* const* edge_pcov, double* const* edge_lev, double* const* edge_t, double* const* cam_stat, double* const* obj_stat,
                                  double* summary, int* status) {
    if (n_prob <= 0) return SUO_OK;
    if (!probs) { suo_set_error("suo_residual_statistics_batch: null argument"); return SUO_ERR_ARG; }
    return resid_batch(probs, n_prob, ResidOut{cam_cov, obj_cov, edge_chi2, edge_pcov, edge_lev, edge_t, cam_stat, obj_stat, summary, status});
}

int suo_residual_statistics(const suo_ba_problem* problem, double* cam_cov, double* obj_cov, double* edge_chi2, double* edge_pcov, double* edge_lev, double* edge_t,
                            double* cam_stat, double* obj_stat, double* summary, int* status) {
    if (!problem) { suo_set_error("suo_residual_statistics: null argument"); return SUO_ERR_ARG; }
    return suo_residual_statistics_batch(problem, 1, &cam_cov, &obj_cov, &edge_chi2, &edge_pcov, &edge_lev, &edge_t, &cam_stat, &obj_stat, summary, status);
}

int suo_pose_covariances_batch(const suo_ba_problem* probs, int n_prob, double* const* cam_cov, double* const* obj_cov, int* status) {
    if (n_prob <= 0) return SUO_OK;
    if (!probs || !cam_cov || !obj_cov) { suo_set_error("suo_pose_covariances_batch: null argument"); return SUO_ERR_ARG; }
    return cov_batch(probs, n_prob, cam_cov, obj_cov, status, nullptr, nullptr, nullptr, "suo_pose_covariances");
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
    return cov_batch(probs, n_prob, cam_cov, obj_cov, status, &pairs, cross, rel, "suo_pose_covariances_pairs");
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
    return cov_batch(probs, n_prob, cam_cov, obj_cov, status, &pairs, cross, rel, "suo_pose_covariances_graph", true);
}

int suo_pose_covariances_graph(const suo_ba_problem* problem, int n_pair, const int32_t* pair_a, const int32_t* pair_b, double* cam_cov, double* obj_cov, double* cross,
                               double* rel, int* status) {
    if (!problem) { suo_set_error("suo_pose_covariances_graph: null argument"); return SUO_ERR_ARG; }
    return suo_pose_covariances_graph_batch(problem, 1, &n_pair, &pair_a, &pair_b, &cam_cov, &obj_cov, &cross, &rel, status);
}

}  // extern "C"
