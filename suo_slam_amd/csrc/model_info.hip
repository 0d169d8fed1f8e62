// Model statistics: 3-D bounding box and diameter of the mesh database's models.
//
// Replaces bop_toolkit's scripts/calc_model_info.py with misc.py:279-293 (calc_pts_diameter), on the database's float32 points widened exactly to fp64:
//   min_c = min_i p_ic,   size_c = max_i p_ic - min_c
//   d^2(i, j) = ((dx dx + dy dy) + dz dz),  dx = p_ix - p_jx ...,   diameter = sqrt(max_{i <= j} d^2)
// fp64 with + - x only, in that association, no contraction; minima and maxima are exact and sqrt is monotone and correctly rounded, so the one square root
// the host takes of the maximum equals the toolkit's maximum of square roots bit for bit.
//
// Three kernels a call, each launched once for all of its n items:
//   box    one to MI_BOX_SPLIT workgroups an item: float32 minima and maxima through order-preserving integer keys (mi_key) and integer atomics, and the
//          item's flag when a coordinate is not finite.  Finiteness is decided here; a flagged item takes no part in what follows, so no NaN reaches an atomic.
//   max    the work items (item, i-tile a, j-tile b) of csrc/model_info.h, b >= MI_RATIO a: the upper triangle only, items of every model in one list that
//          MI_WG_CAP workgroups walk, so a large model and many small ones share the grid.  A lane keeps MI_NP = 4 i-points in registers (12 doubles); the
//          MI_TILE = 256 j-points are staged once into LDS as fp64 SoA and every lane reads the same j (a broadcast: 3 ds_read_b64 per 36 VALU operations).
//          Per pair 3 subtractions, 3 products, 2 sums, 1 maximum = 9 fp64 VALU operations.  d^2(i, j) = d^2(j, i) exactly, so the pairs i > j that a
//          diagonal tile also forms change nothing, and a ragged tile repeats the model's last point (a pair that exists): nothing is read past the points.
//          Reduced per wave by shuffles, per workgroup in LDS, then one 64-bit atomicMax on the bit pattern (d^2 >= +0 finite: ordered like its pattern;
//          csrc/eval_bop.hip does the same) and, when the pair is asked for, the work item's own maximum stored at its index.
//   pair   only when asked: the work items whose stored maximum equals the item's rescan their tile for d^2 == max with i <= j < P and keep the lowest
//          (i << 32) | j by a 64-bit atomicMin -- the lowest i, then the lowest j, whatever the grid or the batch.
// Every result is a minimum or maximum of values that do not depend on which lane forms them: an item in a batch has the bits it has alone.
// Measured: profiles/model_info.txt.
#include <algorithm>

#include "../../include/suo_hip.h"
#include "suo_internal.h"
#include "model_info.h"

#pragma clang fp contract(off)

namespace suo {

// the item of work item w: first[z] <= w < first[z + 1] (every item has at least one)
__device__ __forceinline__ int mi_find(const long long* first, int n, long long w) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (first[mid] <= w) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(MI_BLOCK) void model_info_box_kernel(ModelInfoArgs g) {
    __shared__ unsigned red[MI_BLOCK / 64][6];
    const int z = blockIdx.x, m = g.model[z];
    const int p0 = g.off[m], P = g.off[m + 1] - p0;
    unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    bool bad = false;
    for (long long i = (long long)blockIdx.y * MI_BLOCK + threadIdx.x; i < P; i += (long long)gridDim.y * MI_BLOCK) {
        const float* p = g.pts + (size_t)(p0 + i) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned u = __float_as_uint(p[c]);
            if ((u & 0x7f800000u) == 0x7f800000u) { bad = true; continue; }
            const unsigned k = mi_key(u);
            lo[c] = min(lo[c], k); hi[c] = max(hi[c], k);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { lo[c] = min(lo[c], (unsigned)__shfl_xor((int)lo[c], o)); hi[c] = max(hi[c], (unsigned)__shfl_xor((int)hi[c], o)); }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { red[threadIdx.x >> 6][c] = lo[c]; red[threadIdx.x >> 6][3 + c] = hi[c]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        unsigned v = red[0][threadIdx.x];
        for (int w = 1; w < MI_BLOCK / 64; ++w) v = threadIdx.x < 3 ? min(v, red[w][threadIdx.x]) : max(v, red[w][threadIdx.x]);
        if (threadIdx.x < 3) atomicMin(&g.box[(size_t)z * 6 + threadIdx.x], v);
        else atomicMax(&g.box[(size_t)z * 6 + threadIdx.x], v);
    }
    if (bad) atomicOr(&g.flags[z], 1u);
}

// what the two pair passes share: the work item's place, its j-tile staged into LDS and its i-points in registers
struct MiTile { int z, P, p0; long long i0, j0; unsigned long long top; };       // z < 0: nothing to do for this work item; top: the item's maximum (pair pass)

// Where work item w lies: a search over first[], a square root and a few integer steps -- the same for the whole workgroup, so one lane does it and the
// others read the result from LDS.  pair: the pair pass, which takes only the work items whose stored maximum equals the item's.  The barrier in front keeps
// the lane from overwriting a place that a slower wave has yet to read (and ends every read of the tile the item before staged); the one behind publishes it.
__device__ __forceinline__ MiTile mi_place(const ModelInfoArgs& g, long long w, bool pair, MiTile* shared) {
    __syncthreads();
    if (threadIdx.x == 0) {
        MiTile t;
        t.z = mi_find(g.first, g.n, w);
        t.top = 0;
        if (g.flags[t.z]) t.z = -1;                               // a flagged item is not scanned: tmax holds nothing for it
        else if (pair && g.tmax[w] != (t.top = g.dmax[t.z])) t.z = -1;
        if (t.z >= 0) {
            const int m = g.model[t.z];
            t.p0 = g.off[m];
            t.P = g.off[m + 1] - t.p0;
            long long a, b;
            mi_item(w - g.first[t.z], t.P, &a, &b);
            t.i0 = a * MI_ITILE; t.j0 = b * MI_TILE;
        } else {
            t.P = 0; t.p0 = 0; t.i0 = t.j0 = 0;
        }
        *shared = t;
    }
    __syncthreads();
    return *shared;
}

__device__ __forceinline__ void mi_load(const ModelInfoArgs& g, const MiTile& t, double* sx, double* sy, double* sz, double* px, double* py, double* pz) {
    const int tid = threadIdx.x;
    {   // past the last point: the last point again
        const int j = (int)min(t.j0 + tid, (long long)t.P - 1);
        const float* p = g.pts + (size_t)(t.p0 + j) * 3;
        sx[tid] = (double)p[0]; sy[tid] = (double)p[1]; sz[tid] = (double)p[2];
    }
#pragma unroll
    for (int k = 0; k < MI_NP; ++k) {
        const int i = (int)min(t.i0 + k * MI_BLOCK + tid, (long long)t.P - 1);
        const float* p = g.pts + (size_t)(t.p0 + i) * 3;
        px[k] = (double)p[0]; py[k] = (double)p[1]; pz[k] = (double)p[2];
    }
}

__global__ __launch_bounds__(MI_BLOCK) void model_info_max_kernel(ModelInfoArgs g) {
    __shared__ double sx[MI_TILE], sy[MI_TILE], sz[MI_TILE];
    __shared__ double red[MI_BLOCK / 64];
    __shared__ MiTile place;
    const int tid = threadIdx.x;
    for (long long w = blockIdx.x; w < g.total; w += gridDim.x) {
        const MiTile t = mi_place(g, w, false, &place);
        if (t.z < 0) continue;                                   // the whole workgroup
        double px[MI_NP], py[MI_NP], pz[MI_NP], mx[MI_NP];
        mi_load(g, t, sx, sy, sz, px, py, pz);
#pragma unroll
        for (int k = 0; k < MI_NP; ++k) mx[k] = 0.0;
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < MI_TILE; ++j) {
            const double xj = sx[j], yj = sy[j], zj = sz[j];
#pragma unroll
            for (int k = 0; k < MI_NP; ++k) {
                const double dx = px[k] - xj, dy = py[k] - yj, dz = pz[k] - zj;
                mx[k] = fmax(mx[k], (dx * dx + dy * dy) + dz * dz);
            }
        }
        double v = fmax(fmax(mx[0], mx[1]), fmax(mx[2], mx[3]));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
        if ((tid & 63) == 0) red[tid >> 6] = v;
        __syncthreads();
        if (tid == 0) {                                          // red is written again only behind the next item's barriers
#pragma unroll
            for (int k = 1; k < MI_BLOCK / 64; ++k) v = fmax(v, red[k]);
            const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
            atomicMax(&g.dmax[t.z], bits);
            if (g.tmax) g.tmax[w] = bits;
        }
    }
}
static_assert(MI_NP == 4, "model_info_max_kernel merges four maxima by name");

__global__ __launch_bounds__(MI_BLOCK) void model_info_pair_kernel(ModelInfoArgs g) {
    __shared__ double sx[MI_TILE], sy[MI_TILE], sz[MI_TILE];
    __shared__ MiTile place;
    const int tid = threadIdx.x;
    for (long long w = blockIdx.x; w < g.total; w += gridDim.x) {
        const MiTile t = mi_place(g, w, true, &place);
        if (t.z < 0) continue;                                   // the whole workgroup
        const double top = __longlong_as_double((long long)t.top);
        double px[MI_NP], py[MI_NP], pz[MI_NP];
        mi_load(g, t, sx, sy, sz, px, py, pz);
        __syncthreads();
        unsigned long long key = ~0ull;
        const int nj = (int)min((long long)MI_TILE, t.P - t.j0);
        for (int jj = 0; jj < nj; ++jj) {
            const double xj = sx[jj], yj = sy[jj], zj = sz[jj];
            const long long j = t.j0 + jj;
#pragma unroll
            for (int k = 0; k < MI_NP; ++k) {
                const long long i = t.i0 + k * MI_BLOCK + tid;
                const double dx = px[k] - xj, dy = py[k] - yj, dz = pz[k] - zj;
                const double d = (dx * dx + dy * dy) + dz * dz;
                if (d == top && i <= j) key = min(key, ((unsigned long long)i << 32) | (unsigned long long)j);      // i <= j < P
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) key = min(key, (unsigned long long)__shfl_xor((long long)key, o));
        if ((tid & 63) == 0 && key != ~0ull) atomicMin(&g.pairkey[t.z], key);
    }
}

void model_info_enqueue(const ModelInfoArgs& g, int pmax, hipStream_t s) {
    const int split = (int)std::min<long long>(MI_BOX_SPLIT, ((long long)pmax + MI_ITILE - 1) / MI_ITILE);
    hipLaunchKernelGGL(model_info_box_kernel, dim3(g.n, split), dim3(MI_BLOCK), 0, s, g);
    const int wgs = (int)std::min<long long>(MI_WG_CAP, g.total);
    hipLaunchKernelGGL(model_info_max_kernel, dim3(wgs), dim3(MI_BLOCK), 0, s, g);
    if (g.pairkey) hipLaunchKernelGGL(model_info_pair_kernel, dim3(wgs), dim3(MI_BLOCK), 0, s, g);
}

}  // namespace suo
