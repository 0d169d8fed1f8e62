// Staging shared by the host entries of the geometry kernels (csrc/pnp_api.hip, csrc/ba_api.hip, csrc/ba_ctx.hip, csrc/ba_drive.hip): the caller's host arrays go
// into one device arena (one H2D), results come back in one D2H; everything between the two copies runs on the GPU.
#pragma once
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/suo_hip.h"
#include "lm_device.h"
#include "lm_launch.h"

namespace suo {

// grow-only device arena + pinned host mirror on a stream of its own
struct Arena {
    char* dev = nullptr; char* host = nullptr; size_t cap = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    int ensure(size_t bytes);
    template <class T> std::remove_const_t<T>* mirror(T* d) const { return (std::remove_const_t<T>*)(host + ((const char*)d - dev)); }   // host copy of a device array
};
extern Arena g_arena;       // one per process for suo_pnp* and suo_optimize_batch (guarded by its mutex: the reference is single-threaded)

struct Layout {
    size_t off = 0;
    size_t take(size_t bytes) { size_t o = off; off = (off + bytes + 15) & ~(size_t)15; return o; }
};

// One problem, prepared on the host: edges sorted by (camera, object) pair (order[k] = the caller's index of sorted edge k), the pair lists and their CSRs;
// S: the LmProblem the kernels read, every pointer a DEVICE address inside the arena (Arena::mirror gives the host copy)
struct Prep {
    std::vector<int> order, edge_pair, pair_cam, pair_obj, pair_start, cam_ptr, cam_idx, obj_ptr, obj_idx, cam_obj;
    LmProblem S;
    RsProblem R;             // stage_problems(..., resid = true) only
};
struct Staged {
    std::vector<Prep> prep;
    size_t o_structs = 0, o_rs = 0, in_end = 0, out_end = 0, total = 0;      // arena: [LmProblem structs | inputs | in_end: outputs | out_end: scratch | total]
    size_t cov_begin = 0, cov_end = 0;                             // inside the scratch: every problem's cam_cov / obj_cov / cov_status / cov_cross / cov_rel (csrc/pose_cov_api.hip reads them back)
    size_t o_extra = 0;                                            // stage_problems(..., extra): that many bytes behind the scratch, the caller's to lay out (csrc/track_cov_api.hip)
};

// `who`: the entry the caller called, for the error texts.  prep_problem is the host half of stage_problems (validation, stable sort by pair, pair CSR).
int prep_problem(const suo_ba_problem& q, int index, Prep& P, const char* who);
// cov_form (optional, [n_prob]): LmProblem::cov_form of every problem (csrc/pose_cov_api.hip: plan_cov_batch); pairs (optional): its vertex pairs
struct CovPairs { const int* n; const int32_t* const* a; const int32_t* const* b; };      // per problem: the count and the two index lists
// resid: also the arrays of suo_residual_statistics (one RsProblem per problem at o_rs), its outputs inside [cov_begin, cov_end); without it they take no room
// extra: bytes reserved at Staged::o_extra, neither filled nor copied here
int stage_problems(const suo_ba_problem* probs, int n_prob, Arena& A, Staged& st, const char* who, const int* cov_form = nullptr, const CovPairs* pairs = nullptr,
                   bool resid = false, size_t extra = 0);
int fetch_results(suo_ba_problem* probs, int n_prob, Arena& A, Staged& st);

}  // namespace suo

// ---- phase-wise bundle adjustment context (csrc/ba_ctx.hip; multi-GPU global BA, drivers: csrc/ba_drive.hip and suo_slam_amd/ba_dist.py) ------------
struct suo_ba_ctx {
    suo::Arena arena;       // the device-resident problem (private: lives across calls)
    suo::Staged st;
    int n_cam = 0, n_obj = 0, ns = 0;
    double* d_io = nullptr; double* h_io = nullptr; size_t io_doubles = 0;   // [out | in | workgroup partials (device only)]
    size_t io_cap = 0, big_cap = 0;                                           // capacities of the (possibly recycled) buffers, in doubles
    double* d_big = nullptr;     // reduced system + right-hand side in global memory when it has more than 96 rows (> 16 free objects)
    int device = 0;              // the device its buffers live on (hipGetDevice at creation)
    bool on_caller_stream = false;      // a *_dev entry has enqueued work on a stream this context does not own: destroy must not park the buffers under it
    hipStream_t on(void* stream) { on_caller_stream = true; return (hipStream_t)stream; }
    double* scratch() const { return d_io + io_doubles; }
    const void* dev_problem() const { return arena.dev + st.o_structs; }
};

namespace suo {
int ba_ctx_create(suo_ba_problem* p, suo_ba_ctx** out, const char* who);
// One unit of the device-resident LM schedule on ONE rank (no exchange between its phases): linearize -> schur -> solve_update, the control steps riding in the
// tail kernels in front of them -- 12 launches.
int ba_unit_one_rank(suo_ba_ctx* c, int robust_on, double* ctl, double* lin_local, double* lin, double* sch, double* red, hipStream_t s);
// the routes of suo_optimize_batch that run the phase kernels (csrc/ba_drive.hip)
int optimize_phasewise(suo_ba_problem* q);
int optimize_phases_one_rank(suo_ba_problem* q);
}  // namespace suo
