// The mesh database behind suo_mesh_db_create: shared by the ADD / ADD-S kernels (csrc/eval.hip, row N1) and the BOP-19
// MSSD / MSPD kernels (csrc/eval_bop.hip, row N5).
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
    // per-call scratch, grow-only
    char* scratch_dev = nullptr; char* scratch_host = nullptr; size_t scratch_cap = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
};

int ensure_scratch(MeshDb* db, size_t bytes);     // csrc/eval.hip

}  // namespace suo
