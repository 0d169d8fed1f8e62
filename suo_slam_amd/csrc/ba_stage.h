// Staging shared by the host entries of the geometry kernels (csrc/pnp_api.hip, csrc/ba_api.hip, csrc/ba_ctx.hip, csrc/ba_drive.hip): the caller's host arrays go
// into one device arena (one H2D), results come back in one D2H; everything between the two copies runs on the GPU.  It stages what suo_optimize_batch needs and
// nothing else; an entry with arrays of its own beside the problems (the covariance entries: csrc/cov_stage.hip) asks for rooms (Staged::room_bytes).
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
    char* base = nullptr;                      // what put() counts from; nullptr in a sizing pass
    size_t take(size_t bytes) { size_t o = off; off = (off + bytes + 15) & ~(size_t)15; return o; }
    template <class T> void put(T*& p, size_t n) { p = (T*)((uintptr_t)base + take(sizeof(T) * n)); }
};

// One problem, prepared on the host: edges sorted by (camera, object) pair (order[k] = the caller's index of sorted edge k), the pair lists and their CSRs;
// S: the LmProblem the kernels read, every pointer a DEVICE address inside the arena (Arena::mirror gives the host copy)
struct Prep {
    std::vector<int> order, edge_pair, pair_cam, pair_obj, pair_start, cam_ptr, cam_idx, obj_ptr, obj_idx, cam_obj;
    LmProblem S;
};
struct Staged {
    std::vector<Prep> prep;
    size_t o_structs = 0, in_end = 0, out_end = 0, total = 0;      // arena: [LmProblem structs | inputs, room 0 | in_end: outputs | out_end: scratch, rooms 1, 2 | total]
    // Rooms of the caller's beside the problems (csrc/cov_stage.hip), 16-byte aligned: [0] inputs, inside [0, in_end); [1] outputs and [2] scratch, behind the LM
    // scratch.  room_bytes: asked for before stage_prepared; room: their DEVICE addresses after it.
    size_t room_bytes[3] = {0, 0, 0};
    char* room[3] = {nullptr, nullptr, nullptr};
};

// `who`: the entry the caller called, for the error texts.  Staging is three steps: prep_problems, the host half (prep_problem of every problem: validation,
// stable sort by pair, pair CSR) -- room sizes may depend on what it finds --; stage_prepared, the arena layout and the LM inputs into the pinned mirror -- the
// caller may then set pointer fields of Prep::S and write its rooms through Arena::mirror --; upload, the LmProblem structs into the mirror and the H2D of
// [0, in_end), or without room 0, which upload_room then sends in a copy of its own.  stage_problems: all three, no rooms.
int prep_problem(const suo_ba_problem& q, int index, Prep& P, const char* who);
int prep_problems(const suo_ba_problem* probs, int n_prob, Staged& st, const char* who);
int stage_prepared(const suo_ba_problem* probs, int n_prob, Arena& A, Staged& st);
int upload(Arena& A, Staged& st, bool with_room = true);
int upload_room(Arena& A, Staged& st);
int stage_problems(const suo_ba_problem* probs, int n_prob, Arena& A, Staged& st, const char* who);
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
