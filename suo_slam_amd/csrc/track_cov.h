// The arrays of suo_tracking_covariances (csrc/track_cov.hip), one struct per problem beside its LmProblem (whose size the LM kernels copy: it stays as it is);
// csrc/cov_stage.hip lays them out -- structs, sigma and in_map in the input room (an H2D of its own, behind the problems'), the three outputs in the output room
// of the one D2H.
// The LmProblem is staged with cov_form 1 and with the edges of the objects that are not in the map taken out of edge_inlier, so that LmProblem::cam_cov, written
// by pose_cov_diag_kernel in front of track_cov_kernel, is Hcc^-1 over the counted edges: the entry's fixed_map_cov.
#pragma once
#include <stdint.h>

namespace suo {

struct TcProblem {
    const double* sigma;         // [6 n_obj][6 n_obj] the map's covariance, mirrored from the caller's upper triangle; rows and columns of objects not in the map are zeros
    const uint8_t* in_map;       // [n_obj]
    double* cam_cov;             // [n_cam][36]        Hcc^-1 + G Sigma G^T
    double* cross;               // [n_cam][n_obj][36] -(G Sigma)[:, o]
    double* rel;                 // [n_cam][n_obj][36] the covariance of T_c T_o
};

}  // namespace suo
