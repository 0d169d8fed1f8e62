// Host entries of the consistency figures (include/suo_hip.h: suo_pose_nees, suo_keypoint_nees): argument rules, staging through the mesh database's grow-only
// scratch under db->mu, the launches of csrc/eval_bop.hip (bop_errors_kernel, as suo_pose_errors_bop launches it) and csrc/eval_nees.hip.  Blocking.
#include <math.h>
#include <string.h>

#include "../../include/suo_hip.h"
#include "suo_internal.h"
#include "mesh_db.h"
#include "eval_nees.h"

using namespace suo;

extern "C" int suo_pose_nees(void* h, int n, const int* model_index, const double* T_est, const double* T_gt, const double* cov, double* nees, double* xi,
                             int* sym_index, double* T_ref, int* status) {
    MeshDb* db = (MeshDb*)h;
    // (what can be refused without looking at the database comes first: a negative index is outside every database)
    if (n < 0) { suo_set_error("suo_pose_nees: n = %d is negative", n); return SUO_ERR_ARG; }
    if (n > 0 && (!model_index || !T_est || !T_gt || !cov || !nees)) { suo_set_error("suo_pose_nees: null model_index, T_est, T_gt, cov or nees"); return SUO_ERR_ARG; }
    for (int i = 0; i < n; ++i)
        if (model_index[i] < 0) { suo_set_error("suo_pose_nees: model_index[%d]=%d out of range", i, model_index[i]); return SUO_ERR_ARG; }
    if (!db) { suo_set_error("suo_pose_nees: null mesh database"); return SUO_ERR_ARG; }
    int rc;
    if ((rc = check_model_index("suo_pose_nees", db, n, model_index, nullptr))) return rc;
    if (status) status[0] = 0;
    if (n == 0) return SUO_OK;
    std::lock_guard<std::mutex> lk(db->mu);
    // the caller's part of the scratch: cov[n][36] (staged) | nees[n] | xi[n][6] | T_ref[n][12] | sym_index[n]
    const size_t o_cov = 0, o_nees = (size_t)n * 288, o_xi = o_nees + (size_t)n * 8, o_tref = o_xi + (size_t)n * 48, o_sym = o_tref + (size_t)n * 96, extra = o_sym + (size_t)n * 4;
    BopLayout L;
    if ((rc = bop_maxima_enqueue_locked(db, "suo_pose_nees", n, model_index, T_est, T_gt, nullptr, extra, &L))) return rc;
    char* xh = db->scratch_host + L.o_extra;
    char* xd = db->scratch_dev + L.o_extra;
    memcpy(xh + o_cov, cov, (size_t)n * 288);
    SUO_HIP_CHECK(hipMemcpyAsync(xd + o_cov, xh + o_cov, (size_t)n * 288, hipMemcpyHostToDevice, db->stream));
    PoseNeesArgs a;
    a.sym = L.args.sym; a.soff = L.args.soff; a.model = L.args.model; a.Te = L.args.Te; a.Tg = L.args.Tg; a.smax = L.args.smax; a.flags = L.args.flags;
    a.cov = (const double*)(xd + o_cov);
    a.nees = (double*)(xd + o_nees); a.xi = (double*)(xd + o_xi); a.Tref = (double*)(xd + o_tref); a.sym_index = (int*)(xd + o_sym);
    a.stride = L.args.stride; a.n = n;
    pose_nees_enqueue(a, db->stream);
    SUO_HIP_CHECK(hipGetLastError());
    SUO_HIP_CHECK(hipMemcpyAsync(xh + o_nees, xd + o_nees, extra - o_nees, hipMemcpyDeviceToHost, db->stream));
    SUO_HIP_CHECK(hipStreamSynchronize(db->stream));
    memcpy(nees, xh + o_nees, (size_t)n * 8);
    if (xi) memcpy(xi, xh + o_xi, (size_t)n * 48);
    if (T_ref) memcpy(T_ref, xh + o_tref, (size_t)n * 96);
    if (sym_index) memcpy(sym_index, xh + o_sym, (size_t)n * 4);
    if (status) {
        int n_nan = 0;
        for (int i = 0; i < n; ++i) n_nan += isnan(nees[i]) ? 1 : 0;
        status[0] = n_nan;
    }
    return SUO_OK;
}

extern "C" int suo_keypoint_nees(void* h, int n_det, const int* n_pts, const double* model_kp, const double* uv, const double* cov, const double* K,
                                 const double* T_ref, double* chi2, double* err) {
    MeshDb* db = (MeshDb*)h;
    if (n_det < 0) { suo_set_error("suo_keypoint_nees: n_det = %d is negative", n_det); return SUO_ERR_ARG; }
    if (n_det > 0 && !n_pts) { suo_set_error("suo_keypoint_nees: null n_pts"); return SUO_ERR_ARG; }
    long long sum = 0;
    for (int d = 0; d < n_det; ++d) {
        if (n_pts[d] < 0) { suo_set_error("suo_keypoint_nees: n_pts[%d]=%d is negative", d, n_pts[d]); return SUO_ERR_ARG; }
        sum += n_pts[d];
    }
    if (sum > 0 && (!model_kp || !uv || !cov || !K || !T_ref || !chi2)) { suo_set_error("suo_keypoint_nees: null model_kp, uv, cov, K, T_ref or chi2"); return SUO_ERR_ARG; }
    if (!db) { suo_set_error("suo_keypoint_nees: null mesh database"); return SUO_ERR_ARG; }
    if (sum == 0) return SUO_OK;
    if (sum > 0x7fffffffll / 4) { suo_set_error("suo_keypoint_nees: %lld keypoints in one call", sum); return SUO_ERR_ARG; }
    const size_t N = (size_t)sum;
    std::lock_guard<std::mutex> lk(db->mu);
    // staged: pts[N][3] | uv[N][2] | cov[N][4] | K[n_det][9] | T[n_det][12] | det[N]   then device-only: chi2[N] | err[N][2]
    const size_t o_pts = 0, o_uv = N * 24, o_cov = o_uv + N * 16, o_k = o_cov + N * 32, o_t = o_k + (size_t)n_det * 72, o_det = o_t + (size_t)n_det * 96;
    const size_t staged = (o_det + N * 4 + 15) & ~(size_t)15, o_chi2 = staged, o_err = o_chi2 + N * 8, total = o_err + N * 16;
    int rc;
    if ((rc = ensure_scratch(db, total))) return rc;
    char* sh = db->scratch_host;
    memcpy(sh + o_pts, model_kp, N * 24);
    memcpy(sh + o_uv, uv, N * 16);
    memcpy(sh + o_cov, cov, N * 32);
    memcpy(sh + o_k, K, (size_t)n_det * 72);
    memcpy(sh + o_t, T_ref, (size_t)n_det * 96);
    int* det = (int*)(sh + o_det);
    size_t at = 0;
    for (int d = 0; d < n_det; ++d)
        for (int j = 0; j < n_pts[d]; ++j) det[at++] = d;
    SUO_HIP_CHECK(hipMemcpyAsync(db->scratch_dev, sh, staged, hipMemcpyHostToDevice, db->stream));
    char* sd = db->scratch_dev;
    KpNeesArgs a;
    a.pts = (const double*)(sd + o_pts); a.uv = (const double*)(sd + o_uv); a.cov = (const double*)(sd + o_cov); a.det = (const int*)(sd + o_det);
    a.K = (const double*)(sd + o_k); a.T = (const double*)(sd + o_t);
    a.chi2 = (double*)(sd + o_chi2); a.err = (double*)(sd + o_err);
    a.total = (int)N;
    keypoint_nees_enqueue(a, db->stream);
    SUO_HIP_CHECK(hipGetLastError());
    SUO_HIP_CHECK(hipMemcpyAsync(sh + o_chi2, sd + o_chi2, total - o_chi2, hipMemcpyDeviceToHost, db->stream));
    SUO_HIP_CHECK(hipStreamSynchronize(db->stream));
    memcpy(chi2, sh + o_chi2, N * 8);
    if (err) memcpy(err, sh + o_err, N * 16);
    return SUO_OK;
}
