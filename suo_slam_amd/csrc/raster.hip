// Depth rasteriser of the BOP-19 VSD error: what bop_toolkit's default Python renderer draws into its depth image
// (renderer_py.py:124-143, 185-226, 428-457, 524-556) under OpenGL's rasterisation rules, restated without a GL.  The rules are fixed in include/suo_hip.h
// (camera space and projection in fp64, pixel-centre samples, fp64 edge functions with the top-left rule, both windings, perspective-correct eye-space Z
// rounded once to float32, nearest fragment wins, a triangle with a vertex at Z <= 0 skipped whole); tests/vsd_ref.py restates them in numpy.
//
// Shape.  Scattered global atomics are an order of magnitude slower than LDS ones on this chip, so the z-buffer of a 64 x 64-pixel tile lives in LDS.
//   raster_setup_kernel   one thread per (render, triangle): the six screen coordinates, the three 1 / Z and the clipped pixel box of the triangle, and by
//                         one integer atomic per wave the render's own clipped pixel box.  A triangle that draws nothing gets an empty box.
//   raster_tile_kernel    one workgroup per (render, tile of the image): 4096 uint32 in LDS at 0xFFFFFFFF.  It scans the render's triangle boxes coalesced,
//                         256 at a time; a lane whose triangle meets the tile in at most RS_SMALL samples walks them itself, larger ones go to an LDS list
//                         that the whole workgroup then takes sample-parallel (a 12-face box filling the image does not serialise on one lane).  A covered
//                         sample does atomicMin on the bit pattern of its positive float32 depth; the tile leaves with plain stores, 0xFFFFFFFF -> 0.0f.
// The grid covers the tiles of the whole image, not of the render's box: that box is known on the device only, and a workgroup whose tile misses it writes
// its zeros and leaves without reading a triangle -- cheaper than a host round trip between the two kernels, and no memset of the images is needed.
// An integer minimum does not depend on the order of its operands and a sample's value does not depend on the lane that computes it, so a render has the
// same bits alone, in a batch and for any tiling.  The tile pass itself (sampling, the two routes of a triangle) is csrc/raster_tile.h: csrc/gt_info.hip
// runs it under another epilogue.
#include <limits.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/suo_hip.h"
#include "suo_internal.h"
#include "mesh_db.h"
#include "raster_tile.h"

namespace suo {

__global__ __launch_bounds__(RS_BLOCK) void raster_setup_kernel(RasterArgs a) {
    const int r = blockIdx.y, m = a.model[r];
    const int F = a.foff[m + 1] - a.foff[m];
    if ((int)blockIdx.x * RS_BLOCK >= F) return;
    const int f = blockIdx.x * RS_BLOCK + threadIdx.x;
    int bx0 = INT_MAX, by0 = INT_MAX, bx1 = -1, by1 = -1;
    if (f < F) {
        const double* T = a.T + (size_t)r * 12;
        const double fx = a.K[(size_t)r * 9], fy = a.K[(size_t)r * 9 + 4], cx = a.K[(size_t)r * 9 + 2], cy = a.K[(size_t)r * 9 + 5];
        const int* fv = a.faces + ((size_t)a.foff[m] + f) * 3;
        const float* pts = a.pts + (size_t)a.off[m] * 3;
        double u[3], v[3], q[3];
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float* p = pts + (size_t)fv[k] * 3;
            const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
            const double X = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
            const double Y = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
            const double Z = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
            ok = ok && Z > 0.0;
            u[k] = fx * (X / Z) + cx;
            v[k] = fy * (Y / Z) + cy;
            q[k] = 1.0 / Z;
        }
        const double area2 = (u[1] - u[0]) * (v[2] - v[0]) - (v[1] - v[0]) * (u[2] - u[0]);
        ok = ok && fabs(area2) < INFINITY && area2 != 0.0;
        int4 b = make_int4(1, 1, 0, 0);
        if (ok) {
            // samples x + 0.5 within [umin, umax]: x from ceil(umin - 0.5) to floor(umax - 0.5), clipped to the image (in fp64: the coordinates may be huge)
            const double x0 = fmax(ceil(fmin(fmin(u[0], u[1]), u[2]) - 0.5), 0.0), x1 = fmin(floor(fmax(fmax(u[0], u[1]), u[2]) - 0.5), (double)(a.w - 1));
            const double y0 = fmax(ceil(fmin(fmin(v[0], v[1]), v[2]) - 0.5), 0.0), y1 = fmin(floor(fmax(fmax(v[0], v[1]), v[2]) - 0.5), (double)(a.h - 1));
            if (x0 <= x1 && y0 <= y1) {
                b = make_int4((int)x0, (int)y0, (int)x1, (int)y1);
                bx0 = b.x; by0 = b.y; bx1 = b.z; by1 = b.w;
            }
        }
        const size_t rec = (size_t)a.rec_off[r] + f;
        a.box[rec] = b;
        double* g = a.geo + rec * 9;
        g[0] = u[0]; g[1] = v[0]; g[2] = u[1]; g[3] = v[1]; g[4] = u[2]; g[5] = v[2]; g[6] = q[0]; g[7] = q[1]; g[8] = q[2];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        bx0 = min(bx0, __shfl_xor(bx0, o)); by0 = min(by0, __shfl_xor(by0, o));
        bx1 = max(bx1, __shfl_xor(bx1, o)); by1 = max(by1, __shfl_xor(by1, o));
    }
    if ((threadIdx.x & 63) == 0 && bx0 <= bx1) {
        atomicMin(&a.rbox[r * 4], bx0); atomicMin(&a.rbox[r * 4 + 1], by0);
        atomicMax(&a.rbox[r * 4 + 2], bx1); atomicMax(&a.rbox[r * 4 + 3], by1);
    }
}

__global__ __launch_bounds__(RS_BLOCK) void raster_tile_kernel(RasterArgs a) {
    __shared__ unsigned zb[RS_TILE * RS_TILE];
    __shared__ int big[RS_BLOCK];
    __shared__ int nbig[2];
    const int r = blockIdx.y, tid = threadIdx.x;
    const int X0 = ((int)blockIdx.x % a.tiles_x) * RS_TILE, Y0 = ((int)blockIdx.x / a.tiles_x) * RS_TILE;
    const int X1 = min(X0 + RS_TILE, a.w) - 1, Y1 = min(Y0 + RS_TILE, a.h) - 1;
    for (int i = tid; i < RS_TILE * RS_TILE; i += RS_BLOCK) zb[i] = 0xFFFFFFFFu;
    if (tid < 2) nbig[tid] = 0;
    __syncthreads();
    if (tile_meets_render(a, r, X0, Y0, X1, Y1)) draw_tile(a, r, X0, Y0, X1, Y1, zb, big, nbig);      // uniform over the workgroup
    // the tile leaves: 0xFFFFFFFF -> 0.0f; four pixels of a row per lane, one 16-byte store where the row allows
    float* out = a.out + (size_t)r * a.h * a.w;
    const bool vec = (a.w & 3) == 0;
    for (int i = tid; i < RS_TILE * RS_TILE / 4; i += RS_BLOCK) {
        const int ly = i / (RS_TILE / 4), lx = (i % (RS_TILE / 4)) * 4, x = X0 + lx, y = Y0 + ly;
        if (y >= a.h || x >= a.w) continue;
        float4 d;
        const unsigned* z = &zb[ly * RS_TILE + lx];
        d.x = z[0] == 0xFFFFFFFFu ? 0.0f : __uint_as_float(z[0]);
        d.y = z[1] == 0xFFFFFFFFu ? 0.0f : __uint_as_float(z[1]);
        d.z = z[2] == 0xFFFFFFFFu ? 0.0f : __uint_as_float(z[2]);
        d.w = z[3] == 0xFFFFFFFFu ? 0.0f : __uint_as_float(z[3]);
        float* o = out + (size_t)y * a.w + x;
        if (vec) *(float4*)o = d;                                              // w % 4 == 0 and x % 4 == 0: the whole quad is inside the row and 16-byte aligned
        else {
            o[0] = d.x;
            if (x + 1 < a.w) o[1] = d.y;
            if (x + 2 < a.w) o[2] = d.z;
            if (x + 3 < a.w) o[3] = d.w;
        }
    }
}

int check_render_args(const char* who, MeshDb* db, int n, const int* model_index, const double* T, const double* K, int width, int height) {
    if (!db || n < 0 || width < 1 || height < 1 || (n > 0 && (!model_index || !T || !K))) { suo_set_error("%s: bad argument", who); return SUO_ERR_ARG; }
    if (n > 65535 || (long long)width * height > (1LL << 28)) { suo_set_error("%s: %d renders of %d x %d exceed one call", who, n, width, height); return SUO_ERR_ARG; }
    for (int i = 0; i < n; ++i) {
        const int m = model_index[i];
        if (m < 0 || m >= db->n_models) { suo_set_error("%s: model_index[%d]=%d out of range", who, i, m); return SUO_ERR_ARG; }
        if (db->face_off.empty() || db->face_off[m + 1] == db->face_off[m]) { suo_set_error("%s: model %d has no faces (suo_mesh_db_set_faces)", who, m); return SUO_ERR_ARG; }
        for (int e = 0; e < 12; ++e)
            if (!std::isfinite(T[(size_t)i * 12 + e])) { suo_set_error("%s: pose %d is not finite", who, i); return SUO_ERR_ARG; }
        for (int e = 0; e < 9; ++e)
            if (!std::isfinite(K[(size_t)i * 9 + e])) { suo_set_error("%s: camera matrix %d is not finite", who, i); return SUO_ERR_ARG; }
    }
    return SUO_OK;
}

int render_setup_locked(MeshDb* db, const char* who, int n, const int* model_index, const double* T, const double* K, int width, int height, RasterArgs* out) {
    long long records = 0;
    int fmax_ = 0;
    std::vector<int> rec_off(n);
    for (int i = 0; i < n; ++i) {
        const int F = db->face_off[model_index[i] + 1] - db->face_off[model_index[i]];
        rec_off[i] = (int)records;
        records += F;
        fmax_ = std::max(fmax_, F);
        if (records > INT_MAX / 16) { suo_set_error("%s: %lld triangle records exceed one call", who, records); return SUO_ERR_ARG; }
    }
    // staged block: T[n][12] | K[n][9] | model[n] | rec_off[n] | rbox[n][4]   then device-only: box[records] (16 bytes each) | geo[records][9]
    const size_t o_t = 0, o_k = (size_t)n * 96, o_model = o_k + (size_t)n * 72, o_rec = o_model + (size_t)n * 4, o_rbox = o_rec + (size_t)n * 4;
    const size_t staged = (o_rbox + (size_t)n * 16 + 15) & ~(size_t)15;
    const size_t o_box = staged, o_geo = o_box + (size_t)records * 16, total = o_geo + (size_t)records * 72;
    int rc;
    if ((rc = grow_buffer(&db->ras_dev, &db->ras_host, &db->ras_cap, total))) return rc;
    memcpy(db->ras_host + o_t, T, (size_t)n * 96);
    memcpy(db->ras_host + o_k, K, (size_t)n * 72);
    memcpy(db->ras_host + o_model, model_index, (size_t)n * 4);
    memcpy(db->ras_host + o_rec, rec_off.data(), (size_t)n * 4);
    int* rb = (int*)(db->ras_host + o_rbox);
    for (int i = 0; i < n; ++i) { rb[4 * i] = INT_MAX; rb[4 * i + 1] = INT_MAX; rb[4 * i + 2] = -1; rb[4 * i + 3] = -1; }
    SUO_HIP_CHECK(hipMemcpyAsync(db->ras_dev, db->ras_host, staged, hipMemcpyHostToDevice, db->stream));
    RasterArgs a;
    a.pts = db->pts_dev; a.off = db->off_dev; a.faces = db->faces_dev; a.foff = db->face_off_dev;
    a.T = (const double*)(db->ras_dev + o_t); a.K = (const double*)(db->ras_dev + o_k);
    a.model = (const int*)(db->ras_dev + o_model); a.rec_off = (const int*)(db->ras_dev + o_rec); a.rbox = (int*)(db->ras_dev + o_rbox);
    a.box = (int4*)(db->ras_dev + o_box); a.geo = (double*)(db->ras_dev + o_geo);
    a.out = nullptr; a.w = width; a.h = height;
    a.tiles_x = (width + RS_TILE - 1) / RS_TILE;
    hipLaunchKernelGGL(raster_setup_kernel, dim3((fmax_ + RS_BLOCK - 1) / RS_BLOCK, n), dim3(RS_BLOCK), 0, db->stream, a);
    SUO_HIP_CHECK(hipGetLastError());
    *out = a;
    return SUO_OK;
}

int render_depth_locked(MeshDb* db, int n, const int* model_index, const double* T, const double* K, int width, int height, float** img_out, int** rbox_out) {
    int rc;
    if ((rc = grow_buffer(&db->img_dev, nullptr, &db->img_cap, (size_t)n * height * width * sizeof(float)))) return rc;
    RasterArgs a;
    if ((rc = render_setup_locked(db, "suo_render_depth", n, model_index, T, K, width, height, &a))) return rc;
    a.out = (float*)db->img_dev;
    const int tiles = a.tiles_x * ((height + RS_TILE - 1) / RS_TILE);
    hipLaunchKernelGGL(raster_tile_kernel, dim3(tiles, n), dim3(RS_BLOCK), 0, db->stream, a);
    SUO_HIP_CHECK(hipGetLastError());
    *img_out = a.out;
    if (rbox_out) *rbox_out = a.rbox;
    return SUO_OK;
}

}  // namespace suo

using namespace suo;

extern "C" int suo_mesh_db_set_faces(void* h, const int* n_faces, const int* faces) {
    MeshDb* db = (MeshDb*)h;
    if (!db || !n_faces || !faces) { suo_set_error("suo_mesh_db_set_faces: bad argument"); return SUO_ERR_ARG; }
    std::vector<int> off(db->n_models + 1, 0);
    for (int i = 0; i < db->n_models; ++i) {
        if (n_faces[i] < 0 || n_faces[i] > INT_MAX / 16 - off[i]) { suo_set_error("suo_mesh_db_set_faces: model %d has %d faces", i, n_faces[i]); return SUO_ERR_ARG; }
        off[i + 1] = off[i] + n_faces[i];
        const int P = db->off[i + 1] - db->off[i];
        for (size_t e = (size_t)off[i] * 3; e < (size_t)off[i + 1] * 3; ++e)
            if (faces[e] < 0 || faces[e] >= P) { suo_set_error("suo_mesh_db_set_faces: model %d: vertex index %d outside its %d points", i, faces[e], P); return SUO_ERR_ARG; }
    }
    std::lock_guard<std::mutex> lk(db->mu);
    int* f_dev = nullptr; int* o_dev = nullptr;
    const size_t fbytes = std::max<size_t>((size_t)off.back() * 3 * sizeof(int), 4), obytes = off.size() * sizeof(int);
    hipError_t e = hipMalloc((void**)&f_dev, fbytes);
    if (e == hipSuccess) e = hipMalloc((void**)&o_dev, obytes);
    if (e == hipSuccess && off.back() > 0) e = hipMemcpy(f_dev, faces, (size_t)off.back() * 3 * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(o_dev, off.data(), obytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (f_dev) (void)hipFree(f_dev);
        if (o_dev) (void)hipFree(o_dev);
        suo_set_error("suo_mesh_db_set_faces: %s", hipGetErrorString(e));
        return SUO_ERR_HIP;
    }
    if (db->faces_dev) (void)hipFree(db->faces_dev);
    if (db->face_off_dev) (void)hipFree(db->face_off_dev);
    db->faces_dev = f_dev; db->face_off_dev = o_dev; db->face_off = off;
    return SUO_OK;
}

extern "C" int suo_render_depth(void* h, int n, const int* model_index, const double* T, const double* K, int width, int height, float* depth_out) {
    MeshDb* db = (MeshDb*)h;
    if (n > 0 && !depth_out) { suo_set_error("suo_render_depth: bad argument"); return SUO_ERR_ARG; }
    if (!db) { suo_set_error("suo_render_depth: bad argument"); return SUO_ERR_ARG; }
    std::lock_guard<std::mutex> lk(db->mu);
    int rc;
    if ((rc = check_render_args("suo_render_depth", db, n, model_index, T, K, width, height))) return rc;
    if (n == 0) return SUO_OK;
    float* img = nullptr;
    if ((rc = render_depth_locked(db, n, model_index, T, K, width, height, &img, nullptr))) return rc;
    SUO_HIP_CHECK(hipMemcpyAsync(depth_out, img, (size_t)n * height * width * sizeof(float), hipMemcpyDeviceToHost, db->stream));
    SUO_HIP_CHECK(hipStreamSynchronize(db->stream));
    return SUO_OK;
}
