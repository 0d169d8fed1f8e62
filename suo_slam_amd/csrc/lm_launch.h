// Host launchers of the geometry kernels (csrc/pnp.hip, csrc/lm*.hip, csrc/lm_dist.hip), declared ONCE: the files that define them and the files that call them
// (csrc/pnp_api.hip, csrc/ba_*.hip, csrc/cov_stage.hip -- the one caller of the covariance chain --, csrc/*_cov_api.hip, csrc/frame_geom.hip) include this header,
// and default arguments live here only.
#pragma once
#include "suo_internal.h"

namespace suo {
// ---- PnP (csrc/pnp.hip; pnp_get_iterations: csrc/pnp_api.hip, on the host) ----
int pnp_get_iterations(double estimated_inliers);
constexpr int PNP_MAX_PER_LANE = 16;                    // the refinement strides 64 lanes over an object's points, 16 per lane at the most
constexpr int PNP_MAX_POINTS = 64 * PNP_MAX_PER_LANE;   // = 1024 points per object; the host entries refuse more (csrc/pnp_api.hip)
// launch_pnp_replay takes launch_pnp_batch_counts' width rule: 16 waves per object for n_obj <= SUO_PNP_WIDE_UPTO (32), else 4
int launch_pnp_replay(int n_obj, const int* offsets, const double* xs, const double* ys, double threshold, const int* iter_tab, const int* iter_tab_off,
                      int do_refine, const int* draws, int n_draws, double* T_out, int* status, int* best_out, int* iters_out, int* win_out, hipStream_t s);
int launch_pnp_batch(int n_obj, const int* offsets, const double* xs, const double* ys, double threshold, uint64_t seed,
                     const int* iter_tab, const int* iter_tab_off, int do_refine, double* T_out, int* status, int* best_out,
                     int* iters_out, hipStream_t s);
int launch_pnp_batch_counts(int n_obj, const int* offsets, const int* counts, const int* group_first, const double* xs, const double* ys, double threshold, uint64_t seed,
                            const int* iter_tab, const int* iter_tab_off, int do_refine, double* T_out, int* status, int* best_out,
                            int* iters_out, hipStream_t s, const uint64_t* seed_add = nullptr);
// test entry (suo_debug_pnp_refine): one wave per object through the refinement's own device functions; device pointers, arguments checked by the host entry
int launch_debug_pnp_refine(int n_obj, const int* offsets, const double* xs, const double* ys, double threshold, const int* mode, const double* start_qt,
                            const int* start_idx, const int* sel_in, const int* max_iter, const double* tol, double* out_d, int* out_i, int* sel0_out,
                            int* sel1_out, hipStream_t s);
// test entry (suo_debug_p3p): one thread per four-point problem through p3p_lambdatwist and p4p; device pointers, xs [n][4][3], ys [n][4][2]
int launch_debug_p3p(int n, const double* xs, const double* ys, int* valid, double* R, double* t, double* qt, int* status, hipStream_t s);
// ---- whole LM runs in one launch: problems_dev = n_problems LmProblem structs (csrc/lm_device.h) in device memory ----
int launch_lm(const void* problems_dev, int n_problems, int lds_bytes, hipStream_t s);
int launch_lm_big(const void* problems_dev, int n_problems, int lds_bytes, hipStream_t s);
int lm_lds_bytes(int C, int O, int E, int NP, int n_free_obj_schur);
size_t lm_lds_bytes_uncapped(int C, int O, int E, int NP, int n_free_obj_schur);
int launch_lm_cam(const void* problems_dev, int n_problems, hipStream_t s);
int launch_lm_cam2(const void* problems_dev, int n_problems, int max_edges, hipStream_t s);
int lm_cam2_max_edges();
int launch_lm_frame(const void* problems_dev, int n_problems, int max_obj, hipStream_t s);
int launch_lm_frame2(const void* problems_dev, int n_problems, int max_obj, int max_edges, hipStream_t s);
int lm_frame2_max_edges();
// ---- the phases of one LM trial (csrc/lm_dist.hip); ctl: the control block of the device-resident schedule, fold_ctl: its step folded into the tail kernel ----
size_t ba_scratch_doubles();
int launch_ba_init(const void* P, hipStream_t s);
int launch_ba_classify(const void* P, int keep_all, double* out, double* scratch, hipStream_t s);
int launch_ba_linearize(const void* P, int robust_on, double* out, double* scratch, int rank, int world, hipStream_t s, const double* ctl = nullptr, double* copy_to = nullptr,
                        int copy_n = 0, double* fold_ctl = nullptr);
int launch_ba_schur(const void* P, double lambda, int ns, double* out, double* scratch, hipStream_t s, const double* ctl = nullptr);
int launch_ba_solve_update(const void* P, double lambda, int ns, int robust_on, const double* HB, const double* St, int expect_ok, double* out,
                           double* scratch, double* big, hipStream_t s, const double* ctl = nullptr, double* fold_ctl = nullptr);
int launch_ba_ctl_begin(double* ctl, int its, int world, hipStream_t s);
int launch_ba_ctl_lin(const void* P, double* ctl, const double* lin, double* scratch, hipStream_t s);
int launch_ba_ctl_decide(const void* P, double* ctl, const double* red, hipStream_t s);
int launch_ba_copy(const double* src, double* dst, int n, hipStream_t s);
int launch_ba_restore(const void* P, hipStream_t s);
int launch_ba_finalize(const void* P, hipStream_t s);
// ---- 6x6 marginal pose covariances at the state of the problems (csrc/pose_cov.hip); each kernel takes the problems whose LmProblem::cov_form names it ----
int launch_pose_cov_diag(const void* problems_dev, int n_problems, hipStream_t s);                        // cov_form 0 / 1: one wave per problem
// cov_form 2: one workgroup per problem, <= 16 free objects; pairs: the instantiation that also writes the cross blocks of LmProblem::cpair_a / cpair_b
int launch_pose_cov_coupled(const void* problems_dev, int n_problems, int max_free_obj, hipStream_t s, bool pairs = false);
int launch_pose_cov_pairs(const void* problems_dev, int n_problems, int max_pairs, hipStream_t s);        // every form, behind the two: cross / rel of the pairs
// cov_form 3 (csrc/pose_cov_graph.hip): free cameras next to up to POSE_COV_GRAPH_MAX_OBJ free objects, the reduced system in the arena's scratch -- four launches
// (factor, columns of the inverse, cameras, cross blocks of the pairs), sized by the largest form-3 problem; launch_pose_cov_pairs goes behind it.
// The cap: a lane of the column kernel holds 6 * cap / 64 elements of a row in registers and a wave ns doubles in LDS; S, Sigma_OO cost 2 * 8 * (6 cap)^2 bytes of
// scratch per problem (2.4 MB at 64), mirrored by the arena's pinned host copy.
constexpr int POSE_COV_GRAPH_MAX_OBJ = 64;
int launch_pose_cov_graph(const void* problems_dev, int n_problems, int max_free_obj, int max_cam, int max_pairs, hipStream_t s);
// ---- per-edge leverages, studentised residuals and the chi2 scale (csrc/resid_stats.hip): behind the covariance kernels of every form and the pair kernel, the
// problems staged by stage_cov with CovRequest::resid (csrc/cov_stage.h): an RsProblem each and their own (camera, object) pairs as cpair_a / cpair_b; an edge
// kernel and a reduction, two launches
int launch_resid_stats(const void* problems_dev, const void* rs_dev /* RsProblem [n_problems] */, int n_problems, int max_edges, int max_vertices, hipStream_t s);
// ---- consider covariance of tracked cameras (csrc/track_cov.hip): behind launch_pose_cov_diag on problems of cov_form 1; tc_dev = n_problems TcProblem structs
// (csrc/track_cov.h) laid out by stage_cov, one workgroup per (problem, camera)
int launch_track_cov(const void* problems_dev, const void* tc_dev, int n_problems, int max_cam, int max_obj, hipStream_t s);
int launch_debug_cholesky(const double* A, const double* b, int ns, double* x, int* ok, hipStream_t s);
int launch_debug_pose_oplus(const double* T_in, const double* u, int n, double* T_out, double* q_out, hipStream_t s);    // q_out may be nullptr (device pointers)
}  // namespace suo
