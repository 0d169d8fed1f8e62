// Staging shared by the covariance entries (csrc/pose_cov_api.hip, csrc/track_cov_api.hip): one plan, one layout of everything that rides beside the staged problems,
// one launch chain, one fetch.  An entry describes what it wants (CovRequest), plans (and with it preps), stages, launches the chain and its own tail kernel, fetches, scatters.
#pragma once
#include "ba_stage.h"
#include "track_cov.h"

namespace suo {

struct CovPairs { const int* n; const int32_t* const* a; const int32_t* const* b; };      // per problem: the count and the two index lists
// What an entry asks for beside cam_cov / obj_cov / cov_status of every problem.
struct CovRequest {
    const char* who;                            // the entry the caller called, for the error texts
    bool graph = false;                         // (camera, camera) pairs are served and coupled problems may take form 3
    const CovPairs* pairs = nullptr;            // the caller's vertex pairs: cov_cross / cov_rel
    bool resid = false;                         // an RsProblem per problem, and every form >= 2 problem's own (camera, object) pairs as its vertex pairs
    // the tracking entry (every object fixed, checked by the entry): a TcProblem per problem, sigma mirrored from the upper triangle of map_cov[i]; in_map [n_prob][n_obj]
    const double* const* map_cov = nullptr;
    const std::vector<uint8_t>* in_map = nullptr;
};
// Which kernel of csrc/pose_cov.hip takes every problem of the batch, decided ONCE, on the host (the counterpart of csrc/ba_api.hip: plan_ba_batch).
// A problem's form depends on that problem alone, so a batch gives every member the bits it gets alone.
struct CovPlan {
    std::vector<int> form;           // LmProblem::cov_form: 0 no free camera, 1 no free object (and a free camera), 2 coupled in LDS, 3 coupled in device memory
    bool diag = false, coupled = false, graph = false;
    int max_free_obj = 0;            // over the form-2 problems: sizes the reduced system's LDS
    int graph_free_obj = 0, graph_cam = 0;      // over the form-3 problems: size the grids of csrc/pose_cov_graph.hip
    int max_cam = 0, max_obj = 0, max_edges = 0, max_vertices = 0;      // over all problems: size the grids of the entries' own kernels
    int max_pairs = 0;               // over LmProblem::n_cpair, known once the problems are prepared (stage_cov): sizes the pair grids
};
struct CovStaged {
    Staged st;                       // st.room[1]: the output room, every array fetch_cov brings back
    CovPlan plan;
    RsProblem* rs_dev = nullptr; TcProblem* tc_dev = nullptr;      // a struct per problem with CovRequest::resid / in_map, on the device (Arena::mirror: the host's)
    const void* problems() const { return g_arena.dev + st.o_structs; }
};

// The form of every problem -- sizes and flags checked first --, then the caller's pair lists validated.  graph: a coupled problem the old entries answer -- at most
// 16 free objects, no (camera, camera) pair -- keeps form 2 and with it their bits; every other coupled problem takes form 3, up to POSE_COV_GRAPH_MAX_OBJ free
// objects.  The old entries refuse what form 2 does not hold.  The tracking entry's problems take form 1 whether a camera is free or not: it reads Hcc^-1.
int plan_cov_batch(const suo_ba_problem* probs, int n_prob, const CovRequest& rq, CovStaged& cs);      // into cs.plan; then prep_problems into cs.st
// The caller holds g_arena.mu until it has scattered.
int stage_cov(const suo_ba_problem* probs, int n_prob, const CovRequest& rq, CovStaged& cs);
int launch_cov_chain(const CovRequest& rq, const CovStaged& cs, int n_prob);      // diag -> coupled -> graph -> pairs, each where the plan names it
int fetch_cov(const CovStaged& cs);                         // one D2H of the output room, and the sync
inline double* cov_buffer(double* const* list, int i) { return list ? list[i] : nullptr; }      // problem i's buffer of an optional list of optional buffers

}  // namespace suo
