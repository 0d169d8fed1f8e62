// The tile pass of the depth rasteriser, shared by its two epilogues: csrc/raster.hip stores the tile's depth, csrc/gt_info.hip (row N7) reduces it to counts,
// boxes and masks while the z-buffer is still in LDS.  The rules are those of include/suo_hip.h (suo_render_depth); both kernels run this very code, so a
// sample has the same bits in either.
#pragma once
#include <limits.h>
#include <math.h>

#include "suo_internal.h"

namespace suo {

constexpr int RS_BLOCK = 256;
constexpr int RS_TILE = 64;                      // tile side in pixels
constexpr int RS_SMALL = 32;                     // most samples of (triangle box ∩ tile) a single lane walks

struct RasterArgs {
    const float* pts; const int* off;            // mesh database
    const int* faces; const int* foff;
    const int* model;                            // [n]
    const double* T; const double* K;            // [n][12], [n][9]
    const int* rec_off;                          // [n] first triangle record of a render
    int4* box;                                   // [records] clipped pixel box x0, y0, x1, y1 (x0 > x1: draws nothing)
    double* geo;                                 // [records][9] u0 v0 u1 v1 u2 v2 1/Z0 1/Z1 1/Z2
    int* rbox;                                   // [n][4] the render's box, staged as INT_MAX, INT_MAX, -1, -1
    float* out;                                  // [n][h][w]; unused by csrc/gt_info.hip
    int w, h, tiles_x;
};

// One triangle, ready to be sampled.  With s = sign(area2) the weights w_i = s E_i(sample) are >= 0 inside for either winding; E_0 belongs to the edge 1 -> 2
// (the weight of vertex 0), E_1 to 2 -> 0, E_2 to 0 -> 1, E_PQ(p) = (Qx - Px)(py - Py) - (Qy - Py)(px - Px).  The inward normal of an edge is
// s (-(Qy - Py), Qx - Px); the edge is a left edge when its x component is positive, a top edge (rows grow downwards) when that is zero and y positive.
struct Tri {
    double u0, v0, u1, v1, u2, v2, q0, q1, q2, s, A;
    bool tl0, tl1, tl2;
};

__device__ __forceinline__ bool top_left(double s, double dx, double dy) {
    const double nx = s * -dy, ny = s * dx;
    return nx > 0.0 || (nx == 0.0 && ny > 0.0);
}

__device__ __forceinline__ Tri load_tri(const double* g) {
    Tri t;
    t.u0 = g[0]; t.v0 = g[1]; t.u1 = g[2]; t.v1 = g[3]; t.u2 = g[4]; t.v2 = g[5]; t.q0 = g[6]; t.q1 = g[7]; t.q2 = g[8];
    const double area2 = (t.u1 - t.u0) * (t.v2 - t.v0) - (t.v1 - t.v0) * (t.u2 - t.u0);
    t.s = area2 < 0.0 ? -1.0 : 1.0;
    t.A = t.s * area2;
    t.tl0 = top_left(t.s, t.u2 - t.u1, t.v2 - t.v1);
    t.tl1 = top_left(t.s, t.u0 - t.u2, t.v0 - t.v2);
    t.tl2 = top_left(t.s, t.u1 - t.u0, t.v1 - t.v0);
    return t;
}

// the sample of pixel (x, y) against one triangle; zb: the tile's z-buffer, (lx, ly) the pixel within the tile
__device__ __forceinline__ void shade(const Tri& t, int x, int y, unsigned* zb, int lx, int ly) {
    const double px = (double)x + 0.5, py = (double)y + 0.5;
    const double w0 = t.s * ((t.u2 - t.u1) * (py - t.v1) - (t.v2 - t.v1) * (px - t.u1));
    const double w1 = t.s * ((t.u0 - t.u2) * (py - t.v2) - (t.v0 - t.v2) * (px - t.u2));
    const double w2 = t.s * ((t.u1 - t.u0) * (py - t.v0) - (t.v1 - t.v0) * (px - t.u0));
    const bool in = (w0 > 0.0 || (w0 == 0.0 && t.tl0)) && (w1 > 0.0 || (w1 == 0.0 && t.tl1)) && (w2 > 0.0 || (w2 == 0.0 && t.tl2));
    if (!in) return;
    const double iz = ((w0 * t.q0 + w1 * t.q1) + w2 * t.q2) / t.A;
    const float z = (float)(1.0 / iz);
    atomicMin(&zb[ly * RS_TILE + lx], __float_as_uint(z));
}

// does the tile [X0, X1] x [Y0, Y1] meet the pixel box of render r?  Uniform over the workgroup.
__device__ __forceinline__ bool tile_meets_render(const RasterArgs& a, int r, int X0, int Y0, int X1, int Y1) {
    const int rx0 = a.rbox[r * 4], ry0 = a.rbox[r * 4 + 1], rx1 = a.rbox[r * 4 + 2], ry1 = a.rbox[r * 4 + 3];
    return rx0 <= X1 && rx1 >= X0 && ry0 <= Y1 && ry1 >= Y0;
}

// Draws render r into the tile's z-buffer zb[RS_TILE * RS_TILE] (LDS, at 0xFFFFFFFF; nbig[0..1] at 0; a barrier passed since).  It scans the render's triangle
// boxes coalesced, RS_BLOCK at a time; a lane whose triangle meets the tile in at most RS_SMALL samples walks them itself, larger ones go to the LDS list big
// that the whole workgroup then takes sample-parallel.  Every thread of the workgroup calls it; it ends on a barrier.
__device__ __forceinline__ void draw_tile(const RasterArgs& a, int r, int X0, int Y0, int X1, int Y1, unsigned* zb, int* big, int* nbig) {
    const int tid = threadIdx.x;
    const int m = a.model[r], F = a.foff[m + 1] - a.foff[m];
    const int4* box = a.box + a.rec_off[r];
    const double* geo = a.geo + (size_t)a.rec_off[r] * 9;
    int phase = 0;
    for (int base = 0; base < F; base += RS_BLOCK, phase ^= 1) {
        const int f = base + tid;
        if (f < F) {
            const int4 b = box[f];
            const int ix0 = max(b.x, X0), iy0 = max(b.y, Y0), ix1 = min(b.z, X1), iy1 = min(b.w, Y1);
            if (ix0 <= ix1 && iy0 <= iy1) {
                if ((ix1 - ix0 + 1) * (iy1 - iy0 + 1) > RS_SMALL) big[atomicAdd(&nbig[phase], 1)] = f;      // at most one entry per lane: the list cannot overflow
                else {
                    const Tri t = load_tri(geo + (size_t)f * 9);
                    for (int y = iy0; y <= iy1; ++y)
                        for (int x = ix0; x <= ix1; ++x) shade(t, x, y, zb, x - X0, y - Y0);
                }
            }
        }
        __syncthreads();
        if (tid == 0) nbig[phase ^ 1] = 0;                                  // the next chunk's counter: nobody touches it before the barrier below
        const int nb = nbig[phase];
        for (int e = 0; e < nb; ++e) {
            const int g = big[e];
            const int4 b = box[g];
            const int ix0 = max(b.x, X0), iy0 = max(b.y, Y0), ix1 = min(b.z, X1), iy1 = min(b.w, Y1);
            const int bw = ix1 - ix0 + 1, cnt = bw * (iy1 - iy0 + 1);
            if (tid < cnt) {
                const Tri t = load_tri(geo + (size_t)g * 9);
                for (int p = tid; p < cnt; p += RS_BLOCK) {
                    const int y = iy0 + p / bw, x = ix0 + p % bw;
                    shade(t, x, y, zb, x - X0, y - Y0);
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace suo
