// Staging of the covariance entries (csrc/cov_stage.h): plan and validation, the layout and filling of the rooms beside the staged problems, chain, fetch.
#include <string.h>

#include <algorithm>

#include "cov_stage.h"

namespace suo {

static_assert(POSE_COV_GRAPH_MAX_OBJ == SUO_POSE_COV_GRAPH_MAX_OBJ, "the cap the header documents");

int plan_cov_batch(const suo_ba_problem* probs, int n_prob, const CovRequest& rq, CovStaged& cs) {
    const CovPairs* pairs = rq.pairs;
    CovPlan& plan = cs.plan;
    plan.form.assign(n_prob, 0);
    for (int i = 0; i < n_prob; ++i) {
        const suo_ba_problem& q = probs[i];
        if (q.n_cam < 0 || q.n_obj < 0 || q.n_edge < 0 || (q.n_cam > 0 && !q.cam_fixed) || (q.n_obj > 0 && !q.obj_fixed)) {
            suo_set_error("suo_pose_covariances: bad sizes or null flags in problem %d", i);
            return SUO_ERR_ARG;
        }
        if (rq.resid && q.n_edge > 0 && (!q.edge_cam || !q.edge_obj)) { suo_set_error("%s: null edge lists in problem %d", rq.who, i); return SUO_ERR_ARG; }
        plan.max_cam = std::max(plan.max_cam, q.n_cam); plan.max_obj = std::max(plan.max_obj, q.n_obj);
        plan.max_edges = std::max(plan.max_edges, q.n_edge); plan.max_vertices = std::max(plan.max_vertices, q.n_cam + q.n_obj);
        if (rq.in_map) { plan.form[i] = 1; plan.diag = true; continue; }
        int nfo = 0, nfc = 0;
        for (int o = 0; o < q.n_obj; ++o) nfo += q.obj_fixed[o] ? 0 : 1;
        for (int c = 0; c < q.n_cam; ++c) nfc += q.cam_fixed[c] ? 0 : 1;
        if (nfc == 0) { plan.form[i] = 0; plan.diag = true; continue; }
        if (nfo == 0) { plan.form[i] = 1; plan.diag = true; continue; }
        if (rq.graph) {
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
    for (int i = 0; pairs && i < n_prob; ++i) {
        const int n = pairs->n[i], nc = probs[i].n_cam, nv = probs[i].n_cam + probs[i].n_obj;
        if (n < 0 || (n > 0 && (!pairs->a[i] || !pairs->b[i]))) { suo_set_error("%s: problem %d: n_pair = %d or null pair lists", rq.who, i, n); return SUO_ERR_ARG; }
        for (int q = 0; q < n; ++q) {
            const int a = pairs->a[i][q], b = pairs->b[i][q];
            if (a < 0 || a >= nv || b < 0 || b >= nv) { suo_set_error("%s: problem %d: pair %d = (%d, %d) names a vertex outside [0, %d)", rq.who, i, q, a, b, nv); return SUO_ERR_ARG; }
            if (!rq.graph && a < nc && b < nc) { suo_set_error("%s: problem %d: pair %d = (%d, %d) is (camera, camera); pairs are (camera, object) or (object, object)", rq.who, i, q, a, b); return SUO_ERR_ARG; }
        }
    }
    return prep_problems(probs, n_prob, cs.st, rq.who);
}

// The layout of everything the covariance kernels read and write beside the staged problems, inside the rooms of csrc/ba_stage.h (every array on a 16-byte boundary):
//   0 in       [RsProblem structs | TcProblem structs | per problem: cpair_a, cpair_b; order, vptr, vedge; sigma, in_map]
//   1 out      per problem: cam_cov, obj_cov, cov_status, cov_cross, cov_rel; the RsProblem's outputs; the TcProblem's
//   2 scratch  cov_form 3 (csrc/pose_cov_graph.hip): the reduced system, its inverse and every camera's Z, sized by the free objects -- no slot limit
// The pointers, counted from Staged::room (nullptr before stage_prepared: the sizing pass), go into Prep::S and the side structs, the sizes into
// Staged::room_bytes; fill: the input room is written through the pinned mirror.
static void lay_out_cov(const suo_ba_problem* probs, int n_prob, const CovRequest& rq, CovStaged& cs, bool fill) {
    const Arena& A = g_arena; Staged& st = cs.st;
    Layout I, U, X; I.base = st.room[0]; U.base = st.room[1]; X.base = st.room[2];          // (nullptr before stage_prepared)
    I.put(cs.rs_dev, rq.resid ? n_prob : 0); I.put(cs.tc_dev, rq.in_map ? n_prob : 0);
    cs.plan.max_pairs = 0;
    for (int i = 0; i < n_prob; ++i) {
        const suo_ba_problem& q = probs[i];
        const Prep& P = st.prep[i];
        LmProblem& S = st.prep[i].S;
        const size_t E = q.n_edge, C = q.n_cam, O = q.n_obj;
        S.cov_form = cs.plan.form[i];
        // the residual entry: the problem's own (camera, object) pairs, in the order prep_problem deals them; forms 0 and 1 couple nothing (Sigma_co = 0): no pairs
        S.n_cpair = rq.pairs ? rq.pairs->n[i] : (rq.resid && S.cov_form >= 2 ? (int)P.pair_cam.size() : 0);
        cs.plan.max_pairs = std::max(cs.plan.max_pairs, S.n_cpair);
        const size_t NC = S.n_cpair;
        I.put(S.cpair_a, NC); I.put(S.cpair_b, NC);
        U.put(S.cam_cov, 36 * C); U.put(S.obj_cov, 36 * O); U.put(S.cov_status, 3); U.put(S.cov_cross, 36 * NC); U.put(S.cov_rel, 36 * NC);
        if (S.cov_form == 3) {
            size_t nsm = 0;
            for (size_t o = 0; o < O; ++o) nsm += q.obj_fixed[o] ? 0 : 6;
            X.put(S.cov_S, nsm * (nsm + 1)); X.put(S.cov_Sinv, nsm * nsm); X.put(S.cov_Z, 6 * C * nsm); X.put(S.cov_hdr, 2 + O);
        }
        for (int p = 0; fill && p < S.n_cpair; ++p) {
            A.mirror(S.cpair_a)[p] = rq.pairs ? rq.pairs->a[i][p] : P.pair_cam[p];
            A.mirror(S.cpair_b)[p] = rq.pairs ? rq.pairs->b[i][p] : q.n_cam + P.pair_obj[p];
        }
        if (rq.resid) {
            RsProblem R;
            I.put(R.order, E); I.put(R.vptr, C + O + 1); I.put(R.vedge, 2 * E);
            U.put(R.chi2, E); U.put(R.pcov, 3 * E); U.put(R.lev, E); U.put(R.t, E); U.put(R.flag, E); U.put(R.vstat, 3 * (C + O)); U.put(R.summary, 6); U.put(R.status, 2);
            if (!fill) continue;          // (a request has resid or in_map, never both)
            // every vertex's edges by the caller's index, ascending: the order the per-vertex sums of csrc/resid_stats.hip walk
            const int V = q.n_cam + q.n_obj;
            memcpy(A.mirror(R.order), P.order.data(), sizeof(int) * E);
            int* vptr = A.mirror(R.vptr); int* vedge = A.mirror(R.vedge);
            std::fill(vptr, vptr + V + 1, 0);
            for (int e = 0; e < q.n_edge; ++e) { vptr[q.edge_cam[e] + 1]++; vptr[q.n_cam + q.edge_obj[e] + 1]++; }
            for (int v = 0; v < V; ++v) vptr[v + 1] += vptr[v];
            std::vector<int> at(vptr, vptr + V);
            for (int e = 0; e < q.n_edge; ++e) { vedge[at[q.edge_cam[e]]++] = e; vedge[at[q.n_cam + q.edge_obj[e]]++] = e; }
            A.mirror(cs.rs_dev)[i] = R;
        }
        if (rq.in_map) {
            TcProblem T;
            I.put(T.sigma, 36 * O * O); I.put(T.in_map, O);
            U.put(T.cam_cov, 36 * C); U.put(T.cross, 36 * C * O); U.put(T.rel, 36 * C * O);
            if (!fill) continue;
            // the map's covariance mirrored from the caller's upper triangle; rows and columns of objects not in the map are zeros
            const size_t ns = 6 * O;
            double* Sg = A.mirror(T.sigma);
            const double* M = rq.map_cov ? rq.map_cov[i] : nullptr;
            const uint8_t* im = rq.in_map[i].data();
            for (size_t r = 0; r < ns; ++r)
                for (size_t c = r; c < ns; ++c) {
                    const double v = (im[r / 6] && im[c / 6]) ? M[r * ns + c] : 0.0;
                    Sg[r * ns + c] = v; Sg[c * ns + r] = v;
                }
            memcpy(A.mirror(T.in_map), im, O);
            A.mirror(cs.tc_dev)[i] = T;
        }
    }
    st.room_bytes[0] = I.off; st.room_bytes[1] = U.off; st.room_bytes[2] = X.off;
}

// The tracking entry's map covariance travels in a copy of its own, as it did before, the problems on their way while the host mirrors it: in ONE copy a small
// problem left the runtime's copy kernel for the SDMA engine and the two latency-bound kernels behind it ran 5 us longer each (profiles/cov_stage.txt).
int stage_cov(const suo_ba_problem* probs, int n_prob, const CovRequest& rq, CovStaged& cs) {
    lay_out_cov(probs, n_prob, rq, cs, false);          // sizes first: prep_problems has found every problem's pairs
    int rc = stage_prepared(probs, n_prob, g_arena, cs.st);
    if (rc == SUO_OK && rq.in_map) { lay_out_cov(probs, n_prob, rq, cs, false); rc = upload(g_arena, cs.st, false); }
    if (rc != SUO_OK) return rc;
    lay_out_cov(probs, n_prob, rq, cs, true);
    return rq.in_map ? upload_room(g_arena, cs.st) : upload(g_arena, cs.st);
}

// rq.pairs or rq.resid: the coupled kernel's PAIRS instantiation; the pair kernel behind the chain with a caller's lists even where every list is empty
int launch_cov_chain(const CovRequest& rq, const CovStaged& cs, int n_prob) {
    const CovPlan& p = cs.plan;
    hipStream_t s = g_arena.stream;
    int rc = SUO_OK;
    if (p.diag) rc = launch_pose_cov_diag(cs.problems(), n_prob, s);
    if (rc == SUO_OK && p.coupled) rc = launch_pose_cov_coupled(cs.problems(), n_prob, p.max_free_obj, s, rq.pairs || rq.resid);
    if (rc == SUO_OK && p.graph) rc = launch_pose_cov_graph(cs.problems(), n_prob, p.graph_free_obj, p.graph_cam, p.max_pairs, s);
    if (rc == SUO_OK && (rq.pairs || p.max_pairs > 0)) rc = launch_pose_cov_pairs(cs.problems(), n_prob, p.max_pairs, s);
    return rc;
}

int fetch_cov(const CovStaged& cs) {
    SUO_HIP_CHECK(hipMemcpyAsync(g_arena.mirror(cs.st.room[1]), cs.st.room[1], cs.st.room_bytes[1], hipMemcpyDeviceToHost, g_arena.stream));
    SUO_HIP_CHECK(hipStreamSynchronize(g_arena.stream));
    return SUO_OK;
}

}  // namespace suo
