// Host-buffer entry points of the bundle adjustment (what the reference's FFI would bind):
//   suo_optimize / suo_optimize_batch <- the g2o calls of ObjectSLAM.optimize (lib/object_slam.py:703-903)
// plan_ba_batch decides ONCE which kernel every problem of a batch runs on; suo_optimize_batch executes that plan, suo_debug_lm_routes reports it.
#include <algorithm>

#include "ba_stage.h"
#include "tune.h"

using namespace suo;

// csrc/lm_frame2.hip takes one fixed camera, <= 16 objects, the edges that fit its LDS allotment, and -- its lanes keep their own edges'
// outlier flags in a 32-bit mask -- at most 32 edges per lane: 32 * G per object, G = 8 lanes (<= 8 objects) or 4 (9-16)
static bool frame2_takes(const suo_ba_problem& q) {
    if (q.n_cam != 1 || q.n_obj < 1 || q.n_obj > 16 || q.n_edge > lm_frame2_max_edges()) return false;
    int per_obj[16] = {0};
    for (int e = 0; e < q.n_edge; ++e) {
        const int o = q.edge_obj[e];
        if (o < 0 || o >= q.n_obj) return false;
        ++per_obj[o];
    }
    const int cap = 32 * (q.n_obj <= 8 ? 8 : 4);
    for (int o = 0; o < q.n_obj; ++o) if (per_obj[o] > cap) return false;
    return true;
}

struct BaSummary { int nfo = 0, nfc = 0; bool frame2 = false; };      // free objects, free cameras, frame2_takes
struct BaPlan {
    std::vector<BaSummary> sum;
    std::vector<int> route;                 // SUO_LM_ROUTE_* of every problem
    bool one_by_one = false;                // a PHASEWISE graph is present: every member runs alone, on the route it has alone
    int frame_max_obj = 0, max_edges = 0;   // otherwise ONE launch (or the PHASES driver) takes the batch: what its launcher is sized by
};

// Host only.  The ladder: any PHASEWISE graph -> one by one; else PHASES; else the one kernel the whole batch runs on.
static BaPlan plan_ba_batch(const suo_ba_problem* probs, int n_prob) {
    BaPlan plan;
    plan.sum.resize(n_prob);
    plan.route.assign(n_prob, SUO_LM_ROUTE_LM);
    bool cam_only = true, frame_only = true, all_frame2 = true, alone = true;
    static const int frame_kernel = (int)SUO_TUNE("SUO_LM_FRAME", 8);             // max objects per frame it takes; 0: off (A/B)
    static const int frame2 = (int)SUO_TUNE("SUO_LM_FRAME2", 1);                  // 0: one wave per object (A/B)
    for (int i = 0; i < n_prob; ++i) {
        const suo_ba_problem& q = probs[i];
        BaSummary& s = plan.sum[i];
        for (int o = 0; o < q.n_obj; ++o) s.nfo += q.obj_fixed[o] ? 0 : 1;
        for (int c = 0; c < q.n_cam; ++c) s.nfc += q.cam_fixed[c] ? 0 : 1;
        s.frame2 = frame2 != 0 && frame2_takes(q);
        // more than 16 free objects next to free cameras (T-LESS scenes): the reduced system outgrows the single-kernel paths;
        // those graphs run the phase kernels under the host schedule, one by one, the rest of the batch as usual
        if (s.nfo > 16 && s.nfc > 0) { plan.one_by_one = true; plan.route[i] = SUO_LM_ROUTE_PHASEWISE; }
        cam_only = cam_only && s.nfc == 1 && s.nfo == 0;
        alone = alone && q.n_cam == 1 && q.n_edge <= lm_cam2_max_edges();
        // (one wave per object takes <= SUO_LM_FRAME objects: the 16-wave build spills; one wave per frame takes 16)
        frame_only = frame_only && s.nfc == 0 && q.n_obj >= 1 && q.n_obj <= (s.frame2 ? 16 : frame_kernel) && q.n_obj <= 16;
        all_frame2 = all_frame2 && s.frame2;
        plan.frame_max_obj = std::max(plan.frame_max_obj, q.n_obj);
        plan.max_edges = std::max(plan.max_edges, q.n_edge);
    }
    if (plan.one_by_one) {
        for (int i = 0; i < n_prob; ++i)
            if (plan.route[i] != SUO_LM_ROUTE_PHASEWISE) plan.route[i] = plan_ba_batch(&probs[i], 1).route[0];
        return plan;
    }
    auto all = [&](int r) { plan.route.assign(n_prob, r); return plan; };
    // ONE large graph with free cameras and free objects (the global SLAM adjustment): the phase kernels of csrc/lm_dist.hip under the device-resident LM schedule,
    // driven from C (round 6).  Measured at 60 cameras x 8 objects: 106 us per LM trial (129 for the grid-barrier kernel rounds 4-5 ran instead, since removed); the Python-driven form of
    // this very schedule (suo_slam_amd/ba_dist.py, one rank) was already the faster route and ObjectSLAM.optimize could not reach it through one C call.
    static const int big_from = (int)SUO_TUNE("SUO_LM_BIG_EDGES", 512);       // (640 edges: 9.5 vs 12.2 ms, 1000: 10.9 vs 16.0, 350: 8.6 vs 6.1)
    if (n_prob == 1 && plan.max_edges >= big_from && plan.sum[0].nfo > 0 && plan.sum[0].nfc > 0) return all(SUO_LM_ROUTE_PHASES);
    // camera tracking (ObjectSLAM.optimize(curr_only=True)): one free camera, every object fixed -> one wave per problem; the camera alone in its graph
    // (what curr_only=True builds): registers / LDS only (csrc/lm_cam2.hip)
    static const int cam_kernel = (int)SUO_TUNE("SUO_LM_CAM", 1);                    // 0: general kernel (A/B)
    static const int cam2 = (int)suo::env_switch("SUO_LM_CAM2", 1);                  // 0: csrc/lm_cam.hip (A/B)
    if (cam_kernel != 0 && cam_only) return all(cam2 != 0 && alone ? SUO_LM_ROUTE_CAM2 : SUO_LM_ROUTE_CAM);
    // single-view frames (evaluate.py --nviews 1): no free camera -> block-diagonal system.  One fixed camera: one WAVE per frame, the objects side by side
    // (csrc/lm_frame2.hip); otherwise one wave per object (csrc/lm_frame.hip, launch_lm_frame's two builds)
    if (frame_kernel > 0 && frame_only) return all(all_frame2 ? SUO_LM_ROUTE_FRAME2 : (plan.frame_max_obj <= 8 ? SUO_LM_ROUTE_FRAME8 : SUO_LM_ROUTE_FRAME16));
    // frame-sized graphs: one 256-thread workgroup each (csrc/lm.hip); large graphs that the phase route above does not take (several in one call, or no free
    // object / no free camera): the 1024-thread single-workgroup build (csrc/lm_big.hip).
    return all(plan.max_edges >= big_from ? SUO_LM_ROUTE_LM_BIG : SUO_LM_ROUTE_LM);
}

// rows / 6 of the reduced system lm_kernel keeps in LDS: a Schur complement exists only where free objects meet free cameras
static int schur_objs(const BaSummary& s) { return (s.nfo > 0 && s.nfc > 0) ? s.nfo : 0; }

extern "C" {

int suo_optimize_batch(suo_ba_problem* probs, int n_prob) {
    if (n_prob <= 0) return SUO_OK;
    if (!probs) { suo_set_error("suo_optimize_batch: null argument"); return SUO_ERR_ARG; }
    const BaPlan plan = plan_ba_batch(probs, n_prob);
    if (plan.one_by_one) {
        for (int i = 0; i < n_prob; ++i) {
            int rc = plan.route[i] == SUO_LM_ROUTE_PHASEWISE ? optimize_phasewise(&probs[i]) : suo_optimize_batch(&probs[i], 1);
            if (rc != SUO_OK) return rc;
        }
        return SUO_OK;
    }
    if (plan.route[0] == SUO_LM_ROUTE_PHASES) return optimize_phases_one_rank(&probs[0]);
    std::lock_guard<std::mutex> lock(g_arena.mu);
    Staged st;
    int rc = stage_problems(probs, n_prob, g_arena, st, "suo_optimize");
    if (rc != SUO_OK) return rc;
    const void* P = g_arena.dev + st.o_structs;
    hipStream_t s = g_arena.stream;
    int lds_need = 0;       // (the LM routes: the largest dynamic LDS a problem of the batch asks for)
    for (int i = 0; i < n_prob; ++i)
        lds_need = std::max(lds_need, lm_lds_bytes(probs[i].n_cam, probs[i].n_obj, probs[i].n_edge, st.prep[i].S.n_pair, schur_objs(plan.sum[i])));
    switch (plan.route[0]) {
    case SUO_LM_ROUTE_CAM2: rc = launch_lm_cam2(P, n_prob, plan.max_edges, s); break;
    case SUO_LM_ROUTE_CAM: rc = launch_lm_cam(P, n_prob, s); break;
    case SUO_LM_ROUTE_FRAME2: rc = launch_lm_frame2(P, n_prob, plan.frame_max_obj, plan.max_edges, s); break;
    case SUO_LM_ROUTE_FRAME8:
    case SUO_LM_ROUTE_FRAME16: rc = launch_lm_frame(P, n_prob, plan.frame_max_obj, s); break;
    case SUO_LM_ROUTE_LM_BIG: rc = launch_lm_big(P, n_prob, lds_need, s); break;
    default: rc = launch_lm(P, n_prob, lds_need, s); break;
    }
    if (rc != SUO_OK) return rc;
    return fetch_results(probs, n_prob, g_arena, st);
}

int suo_optimize(suo_ba_problem* problem) { return suo_optimize_batch(problem, 1); }

// Test entry: see include/suo_hip.h.  Host only: the plan suo_optimize_batch would execute, and the pair count its staging would find.
int suo_debug_lm_routes(const suo_ba_problem* probs, int n_prob, int* route_out, int* lds_need_out) {
    if (n_prob <= 0) return SUO_OK;
    if (!probs || !route_out) { suo_set_error("suo_debug_lm_routes: null argument"); return SUO_ERR_ARG; }
    const BaPlan plan = plan_ba_batch(probs, n_prob);
    for (int i = 0; i < n_prob; ++i) {
        Prep P;
        int rc = prep_problem(probs[i], i, P, "suo_debug_lm_routes");
        if (rc != SUO_OK) return rc;
        route_out[i] = plan.route[i];
        if (!lds_need_out) continue;
        const suo_ba_problem& q = probs[i];
        const bool lm = plan.route[i] == SUO_LM_ROUTE_LM || plan.route[i] == SUO_LM_ROUTE_LM_BIG;       // (UNCAPPED: what a fully resident problem asks for)
        lds_need_out[i] = !lm ? -1 : (int)std::min<size_t>(lm_lds_bytes_uncapped(q.n_cam, q.n_obj, q.n_edge, (int)P.pair_cam.size(), schur_objs(plan.sum[i])), INT32_MAX);
    }
    return SUO_OK;
}

}  // extern "C"
