// Host-buffer entry points of the pose covariances (include/suo_hip.h: suo_pose_covariances / suo_pose_covariances_batch): staged through the arena of
// suo_optimize_batch (csrc/ba_stage.hip), one H2D, the kernels of csrc/pose_cov.hip, one D2H of the blocks.  The caller's problem is read only.
#include <string.h>

#include <algorithm>

#include "ba_stage.h"

using namespace suo;

// Which kernel of csrc/pose_cov.hip takes every problem of the batch, decided ONCE, on the host (the counterpart of csrc/ba_api.hip: plan_ba_batch).
// A problem's form depends on that problem alone, so a batch gives every member the bits it gets alone.
struct CovPlan {
    std::vector<int> form;           // LmProblem::cov_form: 0 no free camera, 1 no free object (and a free camera), 2 coupled
    bool diag = false, coupled = false;
    int max_free_obj = 0;            // over the coupled problems: sizes the reduced system's LDS
};
static int plan_cov_batch(const suo_ba_problem* probs, int n_prob, CovPlan& plan) {
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

extern "C" {

int suo_pose_covariances_batch(const suo_ba_problem* probs, int n_prob, double* const* cam_cov, double* const* obj_cov, int* status) {
    if (n_prob <= 0) return SUO_OK;
    if (!probs || !cam_cov || !obj_cov) { suo_set_error("suo_pose_covariances_batch: null argument"); return SUO_ERR_ARG; }
    CovPlan plan;
    int rc = plan_cov_batch(probs, n_prob, plan);
    if (rc != SUO_OK) return rc;
    std::lock_guard<std::mutex> lock(g_arena.mu);
    Staged st;
    rc = stage_problems(probs, n_prob, g_arena, st, "suo_pose_covariances", plan.form.data());
    if (rc != SUO_OK) return rc;
    const void* P = g_arena.dev + st.o_structs;
    hipStream_t s = g_arena.stream;
    if (plan.diag) { rc = launch_pose_cov_diag(P, n_prob, s); if (rc != SUO_OK) return rc; }
    if (plan.coupled) { rc = launch_pose_cov_coupled(P, n_prob, plan.max_free_obj, s); if (rc != SUO_OK) return rc; }
    SUO_HIP_CHECK(hipMemcpyAsync(g_arena.host + st.cov_begin, g_arena.dev + st.cov_begin, st.cov_end - st.cov_begin, hipMemcpyDeviceToHost, s));
    SUO_HIP_CHECK(hipStreamSynchronize(s));
    for (int i = 0; i < n_prob; ++i) {
        const LmProblem& S = st.prep[i].S;
        if (cam_cov[i]) memcpy(cam_cov[i], g_arena.mirror(S.cam_cov), sizeof(double) * 36 * (size_t)S.n_cam);
        if (obj_cov[i]) memcpy(obj_cov[i], g_arena.mirror(S.obj_cov), sizeof(double) * 36 * (size_t)S.n_obj);
        if (status) memcpy(status + 2 * i, g_arena.mirror(S.cov_status), sizeof(int) * 2);
    }
    return SUO_OK;
}

int suo_pose_covariances(const suo_ba_problem* problem, double* cam_cov, double* obj_cov, int* status) {
    if (!problem) { suo_set_error("suo_pose_covariances: null argument"); return SUO_ERR_ARG; }
    return suo_pose_covariances_batch(problem, 1, &cam_cov, &obj_cov, status);
}

}  // extern "C"
