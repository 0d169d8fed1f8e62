// The mesh database behind suo_mesh_db_create and what its entries share on the host.  Shared by the ADD / ADD-S kernels (csrc/eval.hip, row N1), the BOP-19
// MSSD / MSPD kernels (csrc/eval_bop.hip, row N5) and the NEES entries over them (csrc/eval_nees_api.hip), the rasteriser and VSD (csrc/raster.hip,
// csrc/eval_vsd.hip, row N6), ADD / ADI / PROJ and CUS (csrc/eval_points.hip, csrc/eval_masks.hip, row N4), gt_info (csrc/gt_info_api.hip, row N7) and
// models_info (csrc/model_info_api.hip, row N8).  The database's buffers, their one growth rule, the range check of model_index and the staged block of a
// call's pairs are declared here and defined once, in csrc/eval.hip.
#pragma once
#include <mutex>
#include <vector>

#include "suo_internal.h"

namespace suo {

struct MeshDb {
    int n_models = 0;
    std::vector<int> off;         // [n_models + 1] point offsets
    int max_pts = 0;
    float* pts_dev = nullptr;     // [off.back()][3]
    int* off_dev = nullptr;
    // symmetry transformations (csrc/eval_bop.hip): absent until suo_mesh_db_set_symmetries or the first suo_pose_errors_bop (identity alone)
    std::vector<int> sym_off;     // [n_models + 1]
    double* sym_dev = nullptr;    // [sym_off.back()][12] row-major 3x4 [R|t]
    int* sym_off_dev = nullptr;
    // triangles (csrc/raster.hip): absent until suo_mesh_db_set_faces; a model with no faces cannot be rendered
    std::vector<int> face_off;    // [n_models + 1], empty until set
    int* faces_dev = nullptr;     // [face_off.back()][3] vertex indices into the model's own points
    int* face_off_dev = nullptr;
    // per-call scratch, grow-only
    char* scratch_dev = nullptr; char* scratch_host = nullptr; size_t scratch_cap = 0;
    // the rasteriser's own, grow-only: staged poses + triangle records, and the rendered depth images (they stay on the device for csrc/eval_vsd.hip)
    char* ras_dev = nullptr; char* ras_host = nullptr; size_t ras_cap = 0;
    char* img_dev = nullptr; size_t img_cap = 0;
    char* test_dev = nullptr; size_t test_cap = 0;      // the test depth images of a VSD call (csrc/eval_vsd.hip): device only, the host never reads them back
    hipStream_t stream = nullptr;
    std::mutex mu;
};

// csrc/eval.hip.  What the entries over the database share before their kernels:
// grow_buffer: a grow-only device buffer, with a pinned host twin when host is not null; a re-growth at least doubles, rounded up to 4 KB.  Every grow-only
// buffer above goes through it; ensure_scratch is grow_buffer on the scratch pair.
// check_model_index: SUO_ERR_ARG with "<who>: model_index[i]=m out of range" for the first index outside the database; *pmax (may be null) the most points
// of a model named.
// stage_pairs_locked: the staged block of a call's pairs -- both poses, the camera matrix and the model index of each, laid out where it is defined -- at
// offset 0 of a scratch of total_bytes (>= pair_block_bytes(n), the block's 16-byte-aligned size; the rest is the caller's), K == NULL staged as the
// identity, and its one upload enqueued on db->stream.  *out names the four arrays on the device.  Caller holds db->mu and has checked the arguments.
struct PairBlock { const double* Te; const double* Tg; const double* K; const int* model; size_t staged; };
inline size_t pair_block_bytes(int n) { return ((size_t)n * (96 + 96 + 72 + 4) + 15) & ~(size_t)15; }
int grow_buffer(char** dev, char** host, size_t* cap, size_t bytes);
int ensure_scratch(MeshDb* db, size_t bytes);
int check_model_index(const char* who, const MeshDb* db, int n, const int* model_index, int* pmax);
int stage_pairs_locked(MeshDb* db, int n, const int* model_index, const double* T_est, const double* T_gt, const double* K, size_t total_bytes, PairBlock* out);

// csrc/eval_bop.hip.  The arguments of bop_errors_kernel / bop_errors_min_kernel.
struct BopArgs {
    const float* pts; const int* off;            // mesh database
    const double* sym; const int* soff;          // its symmetry sets [soff[m] .. soff[m + 1])[12]
    const int* model;                            // [n]
    const double* Te; const double* Tg;          // [n][12] row-major 3x4
    const double* K;                             // [n][9]
    unsigned long long* smax;                    // [n][stride][2] bit patterns of max_i d^2: 3-D, 2-D
    unsigned* flags;                             // [n] bit 0: a non-finite 3-D distance, bit 1: a non-finite 2-D distance
    double* out;                                 // [n][2] min_s max_i d^2
    int stride, chunk;
};

// bop_maxima_enqueue_locked: what suo_pose_errors_bop and suo_pose_nees (csrc/eval_nees_api.hip) share -- stage n pairs into the database's scratch and enqueue
// bop_errors_kernel on db->stream.  On return L->args.smax is the [n][stride][2] block of merged squared maxima per symmetry (bit patterns; 3-D, 2-D) and
// L->args.flags the sticky non-finite flags, both complete once the stream reaches what the caller enqueues next; o_out / o_flags are scratch offsets, and
// `extra` bytes at o_extra (256-aligned, behind everything the kernels touch) are the caller's.  K may be NULL (the 2-D half is then not meaningful).
// Caller holds db->mu and has checked the arguments.
struct BopLayout { BopArgs args; size_t o_out, o_flags, o_extra; };
int bop_maxima_enqueue_locked(MeshDb* db, const char* who, int n, const int* model_index, const double* T_est, const double* T_gt, const double* K, size_t extra,
                              BopLayout* L);

// csrc/raster.hip.  check_render_args: the argument rules of suo_render_depth (SUO_ERR_ARG with the message set, nothing launched).
// render_depth_locked: enqueue n renders on db->stream (caller holds db->mu and has checked the arguments); on return *img_dev is [n][height][width]
// float32 depth and *rbox_dev [n][4] the renders' clipped pixel boxes (x0, y0, x1, y1; x0 > x1: nothing drawn), both valid until the next render.
// render_setup_locked: the first half of a render, shared with csrc/gt_info_api.hip -- stages the n renders and enqueues raster_setup_kernel; *args then
// names the triangle records and the renders' pixel boxes on the device (args->out is left null: the tile pass and its epilogue are the caller's).
struct RasterArgs;
int render_setup_locked(MeshDb* db, const char* who, int n, const int* model_index, const double* T, const double* K, int width, int height, RasterArgs* args);
int check_render_args(const char* who, MeshDb* db, int n, const int* model_index, const double* T, const double* K, int width, int height);
int render_depth_locked(MeshDb* db, int n, const int* model_index, const double* T, const double* K, int width, int height, float** img_dev, int** rbox_dev);

}  // namespace suo
