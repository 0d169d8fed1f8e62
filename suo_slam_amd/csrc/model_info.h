// Model statistics: what csrc/model_info.hip and csrc/model_info_api.hip share.
#pragma once
#include <math.h>

#include "suo_internal.h"

namespace suo {

constexpr int MI_BLOCK = 256;                    // threads per workgroup
constexpr int MI_NP = 4;                         // i-points per lane, in registers
constexpr int MI_ITILE = MI_BLOCK * MI_NP;       // i-points per work item
constexpr int MI_TILE = 256;                     // j-points per work item, staged in LDS
constexpr int MI_RATIO = MI_ITILE / MI_TILE;     // j-tiles under one i-tile
constexpr int MI_WG_CAP = 1024;                  // workgroups of the pair passes: 256 CUs x 4; each walks the work items from its index in steps of the grid
constexpr int MI_BOX_SPLIT = 8;                  // workgroups a model's box may take

static_assert(MI_TILE == MI_BLOCK, "one thread stages one j-point");
static_assert(MI_ITILE % MI_TILE == 0, "an i-tile begins at a j-tile boundary");

// The work items of a model of P points: i-tile a < Ti = ceil(P / MI_ITILE) against the j-tiles b = MI_RATIO a .. Tj - 1, Tj = ceil(P / MI_TILE) -- the
// j-tiles that hold a point j >= the i-tile's first.  Row a has Tj - MI_RATIO a of them (at least one), rows in order.
__host__ __device__ inline long long mi_items_before(long long a, long long tj) { return a * tj - (long long)MI_RATIO * (a * (a - 1) / 2); }
__host__ __device__ inline long long mi_items(int P) {
    const long long ti = ((long long)P + MI_ITILE - 1) / MI_ITILE, tj = ((long long)P + MI_TILE - 1) / MI_TILE;
    return mi_items_before(ti, tj);
}
// item t < mi_items(P) -> (a, b): the root of the row sum by a square root, then stepped to the exact row
__host__ __device__ inline void mi_item(long long t, int P, long long* a_out, long long* b_out) {
    const long long tj = ((long long)P + MI_TILE - 1) / MI_TILE;
    const double B = (double)tj + 0.5 * MI_RATIO;
    double disc = B * B - 2.0 * MI_RATIO * (double)t;
    if (disc < 0.0) disc = 0.0;
    long long a = (long long)((B - sqrt(disc)) / MI_RATIO);
    if (a < 0) a = 0;
    while (a > 0 && mi_items_before(a, tj) > t) --a;
    while (mi_items_before(a + 1, tj) <= t) ++a;
    *a_out = a;
    *b_out = (long long)MI_RATIO * a + (t - mi_items_before(a, tj));
}

// float32 <-> an unsigned key of the same order (-0 below +0): the box pass takes its minima and maxima with integer atomics
__host__ __device__ inline unsigned mi_key(unsigned bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
__host__ __device__ inline unsigned mi_unkey(unsigned key) { return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key; }

struct ModelInfoArgs {
    const float* pts; const int* off;            // mesh database
    const int* model;                            // [n]
    const long long* first;                      // [n + 1] work items before item z
    unsigned* flags;                             // [n] bit 0: a non-finite coordinate
    unsigned* box;                               // [n][6] keys of min x, y, z, max x, y, z
    unsigned long long* dmax;                    // [n] bit pattern of max d^2
    unsigned long long* pairkey;                 // [n] (i << 32) | j of the lowest diametral pair, or null
    unsigned long long* tmax;                    // [total] bit pattern of each work item's maximum, or null
    int n; long long total;
};

// enqueue the box pass, the maximum pass and (pairkey != null) the pair pass on s; pmax: the call's largest model
void model_info_enqueue(const ModelInfoArgs& g, int pmax, hipStream_t s);

}  // namespace suo
