// csrc/gt_info.hip (the kernels) and csrc/gt_info_api.hip (the host entries suo_gt_info / suo_gt_masks), row N7.
#pragma once
#include "raster_tile.h"

namespace suo {

// an instance's record on the device, ints: three counts, then two boxes as x0 y0 (minima) x1 y1 (maxima) in image coordinates
constexpr int GI_ALL = 0, GI_VALID = 1, GI_VISIB = 2, GI_OBJ = 3, GI_VIS = 7, GI_REC = 11;

struct GtInfoArgs {
    RasterArgs ras;                              // the canvas: w = mult * W, h = mult * H, principal point moved by (off_x, off_y) on the host
    const double* kim;                           // [n][4] fx fy cx cy of the image (the original K)
    const float* test; const int* image_index;   // [n_images][H][W] mm, [n]
    int* rec;                                    // [n][GI_REC]
    unsigned char* mask; unsigned char* mask_visib;      // [n][H][W] cleared, or nullptr
    float delta;
    int W, H, off_x, off_y;                      // the image window within the canvas
};

// enqueues gt_info_init_kernel and gt_info_kernel (tiles = tiles of the canvas) on the stream
void gt_info_enqueue(const GtInfoArgs& g, int n, int tiles, hipStream_t stream);

}  // namespace suo
