// What csrc/viz.hip (kernels) and csrc/viz_api.hip (host entry) share: the device records of a view's primitives.  The rules: include/suo_hip.h, "A view's
// three-panel visualisation".
#pragma once
#include "suo_internal.h"

namespace suo {

constexpr int VIZ_KP_COLOURS = 41, VIZ_BOX_COLOURS = 30;
constexpr int VIZ_BOX_INTS = 5, VIZ_STAMP_INTS = 8;

struct VizKp {                      // 48 bytes: a keypoint's black disc, colour disc and ellipse outline
    int x, y, r_outer, r_inner, colour, has_ellipse, A, B;
    double c, s;
};
struct VizOverlay {                 // 184 bytes: an overlay object, at its rank in paint order
    double T[12], K[9];
    int first, count, colour, pad;  // its points [first, first + count) of the mesh database
};

struct VizArgs {
    const uint8_t* frame; uint8_t* out; int H, W;
    const int* box; int n_box;                      // [n_box][5]
    const int* stamp; int n_stamp;                  // [n_stamp][8], sorted by channel, list order kept within a channel
    const VizKp* kp; int n_kp;
    const VizOverlay* ov; int n_ov; int max_pts;
    const float* pts;                               // the mesh database's points
    int* owner;                                     // [H][W], zero on entry
};

int viz_upload_tables(const uint8_t* kp_bgr);       // once, before the first launch: the stamp weights and the keypoint colours
int viz_enqueue(const VizArgs& a, hipStream_t s);   // viz_splat_kernel (when there are overlays) + viz_compose_kernel

}  // namespace suo
