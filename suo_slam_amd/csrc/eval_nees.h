// Kernels of the consistency figures (csrc/eval_nees.hip), launched by csrc/eval_nees_api.hip.
#pragma once
#include "suo_internal.h"

namespace suo {

struct PoseNeesArgs {
    const double* sym; const int* soff;          // the database's symmetry sets [soff[m] .. soff[m + 1])[12]
    const int* model;                            // [n]
    const double* Te; const double* Tg;          // [n][12] row-major 3x4
    const unsigned long long* smax;              // [n][stride][2] merged squared maxima of bop_errors_kernel (bit patterns); [..][0] is the 3-D one
    const unsigned* flags;                       // [n] bit 0: a non-finite 3-D distance
    const double* cov;                           // [n][36]
    double* nees;                                // [n]
    double* xi;                                  // [n][6]
    double* Tref;                                // [n][12]
    int* sym_index;                              // [n]
    int stride, n;
};

struct KpNeesArgs {
    const double* pts;                           // [sum][3]
    const double* uv;                            // [sum][2]
    const double* cov;                           // [sum][4]
    const int* det;                              // [sum] detection of the keypoint
    const double* K;                             // [n_det][9]
    const double* T;                             // [n_det][12]
    double* chi2;                                // [sum]
    double* err;                                 // [sum][2]
    int total;
};

void pose_nees_enqueue(const PoseNeesArgs& a, hipStream_t stream);
void keypoint_nees_enqueue(const KpNeesArgs& a, hipStream_t stream);

}  // namespace suo
