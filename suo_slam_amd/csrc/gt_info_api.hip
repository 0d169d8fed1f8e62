// Host entries of row N7: suo_gt_info and suo_gt_masks (include/suo_hip.h) over the kernels of csrc/gt_info.hip.  Both check every argument before anything
// is launched, upload the test depth images once, and take the instances in launches of at most GI_MAX_INSTANCES (fewer when their triangle records or mask
// bytes would exceed one launch's buffers); an instance's values do not depend on the launch it falls into.
#include <limits.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/suo_hip.h"
#include "suo_internal.h"
#include "mesh_db.h"
#include "gt_info.h"

namespace suo {

constexpr int GI_MAX_INSTANCES = 1024;                   // instances of one launch
constexpr long long GI_MAX_RECORDS = 1LL << 22;          // triangle records of one launch (88 bytes each), unless a single instance has more
constexpr size_t GI_MAX_MASK_BYTES = (size_t)256 << 20;  // mask bytes of one launch, unless a single instance has more

// mult: 3 for the info form (the scripts' canvas), 1 for the mask form
static int gt_info_run(const char* who, int mult, MeshDb* db, int n, const int* model_index, const double* T, const double* K, int width, int height, int n_images,
                       const float* depth_test, const int* image_index, double delta, long long* px_counts, int* bbox_obj, int* bbox_visib, uint8_t* mask,
                       uint8_t* mask_visib) {
    // everything that needs no database first
    if (n < 0 || width < 1 || height < 1) { suo_set_error("%s: bad argument (n >= 0, width and height >= 1)", who); return SUO_ERR_ARG; }
    if (!std::isfinite(delta)) { suo_set_error("%s: delta is not finite", who); return SUO_ERR_ARG; }
    // 3 * width and 3 * height must stay ints with room to spare, and the canvas within what one render call takes (2^28 samples)
    if (width > (1 << 28) || height > (1 << 28) || 9LL * width * height > (1LL << 28)) {
        suo_set_error("%s: a canvas of 3 x %d by 3 x %d overflows the rasteriser's pixel boxes", who, width, height);
        return SUO_ERR_ARG;
    }
    if (n > 0 && (!model_index || !T || !K || !depth_test || !image_index)) { suo_set_error("%s: null pointer", who); return SUO_ERR_ARG; }
    if (n > 0 && n_images < 1) { suo_set_error("%s: n_images=%d with %d instances", who, n_images, n); return SUO_ERR_ARG; }
    if (n > 0 && mult == 3 && (!px_counts || !bbox_obj || !bbox_visib)) { suo_set_error("%s: null pointer", who); return SUO_ERR_ARG; }
    for (int i = 0; i < n; ++i) {
        if (image_index[i] < 0 || image_index[i] >= n_images) { suo_set_error("%s: image_index[%d]=%d out of range", who, i, image_index[i]); return SUO_ERR_ARG; }
        for (int e = 0; e < 12; ++e)
            if (!std::isfinite(T[(size_t)i * 12 + e])) { suo_set_error("%s: pose %d is not finite", who, i); return SUO_ERR_ARG; }
        for (int e = 0; e < 9; ++e)
            if (!std::isfinite(K[(size_t)i * 9 + e])) { suo_set_error("%s: camera matrix %d is not finite", who, i); return SUO_ERR_ARG; }
    }
    if (!db) { suo_set_error("%s: null mesh database", who); return SUO_ERR_ARG; }
    const int off_x = mult == 3 ? width : 0, off_y = mult == 3 ? height : 0, cw = mult * width, ch = mult * height;
    // the canvas camera: the principal point moved by the offset, the sum formed here in fp64 as the script forms it
    std::vector<double> Kc(K, K + (size_t)n * 9);
    for (int i = 0; i < n; ++i) {
        Kc[(size_t)i * 9 + 2] = K[(size_t)i * 9 + 2] + (double)off_x;
        Kc[(size_t)i * 9 + 5] = K[(size_t)i * 9 + 5] + (double)off_y;
    }
    std::lock_guard<std::mutex> lk(db->mu);
    int rc;
    // the launches, each checked whole before the first one runs
    const size_t hw = (size_t)height * width;
    const bool masks = mult == 1 && (mask || mask_visib);
    std::vector<int> cut{0};
    for (int b = 0; b < n;) {
        int e = b;
        long long records = 0;
        while (e < n && e - b < GI_MAX_INSTANCES) {
            const int m = model_index[e];
            const long long F = (m >= 0 && m < db->n_models && !db->face_off.empty()) ? db->face_off[m + 1] - db->face_off[m] : 0;
            if (e > b && (records + F > GI_MAX_RECORDS || (masks && (size_t)(e - b + 1) * hw * 2 > GI_MAX_MASK_BYTES))) break;
            records += F;
            ++e;
        }
        if ((rc = check_render_args(who, db, e - b, model_index + b, T + (size_t)b * 12, Kc.data() + (size_t)b * 9, cw, ch))) return rc;
        cut.push_back(e);
        b = e;
    }
    if (n == 0) return SUO_OK;
    if (mult == 1 && !mask && !mask_visib) return SUO_OK;

    const size_t test_bytes = (size_t)n_images * hw * 4;
    if ((rc = grow_buffer(&db->test_dev, nullptr, &db->test_cap, test_bytes))) return rc;
    SUO_HIP_CHECK(hipMemcpyAsync(db->test_dev, depth_test, test_bytes, hipMemcpyHostToDevice, db->stream));
    for (size_t c = 0; c + 1 < cut.size(); ++c) {
        const int b = cut[c], m = cut[c + 1] - cut[c];
        // staged: kim[m][4] | image_index[m]   then written by the device: rec[m][GI_REC]
        const size_t o_kim = 0, o_ii = (size_t)m * 32, staged = (o_ii + (size_t)m * 4 + 15) & ~(size_t)15, o_rec = staged, total = o_rec + (size_t)m * GI_REC * 4;
        if ((rc = ensure_scratch(db, total))) return rc;
        double* kim = (double*)(db->scratch_host + o_kim);
        for (int i = 0; i < m; ++i) {
            const double* k = K + (size_t)(b + i) * 9;
            kim[4 * i] = k[0]; kim[4 * i + 1] = k[4]; kim[4 * i + 2] = k[2]; kim[4 * i + 3] = k[5];
        }
        memcpy(db->scratch_host + o_ii, image_index + b, (size_t)m * 4);
        SUO_HIP_CHECK(hipMemcpyAsync(db->scratch_dev, db->scratch_host, staged, hipMemcpyHostToDevice, db->stream));
        GtInfoArgs g;
        g.mask = g.mask_visib = nullptr;
        if (masks) {
            const size_t each = (size_t)m * hw;
            if ((rc = grow_buffer(&db->img_dev, nullptr, &db->img_cap, 2 * each))) return rc;
            SUO_HIP_CHECK(hipMemsetAsync(db->img_dev, 0, 2 * each, db->stream));
            if (mask) g.mask = (unsigned char*)db->img_dev;
            if (mask_visib) g.mask_visib = (unsigned char*)db->img_dev + each;
        }
        if ((rc = render_setup_locked(db, who, m, model_index + b, T + (size_t)b * 12, Kc.data() + (size_t)b * 9, cw, ch, &g.ras))) return rc;
        g.kim = (const double*)(db->scratch_dev + o_kim); g.image_index = (const int*)(db->scratch_dev + o_ii); g.rec = (int*)(db->scratch_dev + o_rec);
        g.test = (const float*)db->test_dev;
        g.delta = (float)delta; g.W = width; g.H = height; g.off_x = off_x; g.off_y = off_y;
        gt_info_enqueue(g, m, g.ras.tiles_x * ((ch + RS_TILE - 1) / RS_TILE), db->stream);
        SUO_HIP_CHECK(hipGetLastError());
        if (mult == 3) SUO_HIP_CHECK(hipMemcpyAsync(db->scratch_host + o_rec, db->scratch_dev + o_rec, (size_t)m * GI_REC * 4, hipMemcpyDeviceToHost, db->stream));
        if (g.mask) SUO_HIP_CHECK(hipMemcpyAsync(mask + (size_t)b * hw, g.mask, (size_t)m * hw, hipMemcpyDeviceToHost, db->stream));
        if (g.mask_visib) SUO_HIP_CHECK(hipMemcpyAsync(mask_visib + (size_t)b * hw, g.mask_visib, (size_t)m * hw, hipMemcpyDeviceToHost, db->stream));
        SUO_HIP_CHECK(hipStreamSynchronize(db->stream));
        if (mult != 3) continue;
        const int* rec = (const int*)(db->scratch_host + o_rec);
        for (int i = 0; i < m; ++i) {
            const int* q = rec + (size_t)i * GI_REC;
            long long* pc = px_counts + (size_t)(b + i) * 3;
            pc[0] = q[GI_ALL]; pc[1] = q[GI_VALID]; pc[2] = q[GI_VISIB];
            int* bo = bbox_obj + (size_t)(b + i) * 4;
            int* bv = bbox_visib + (size_t)(b + i) * 4;
            if (q[GI_VISIB] == 0) { for (int e = 0; e < 4; ++e) bo[e] = bv[e] = -1; continue; }      // also when px_count_all > 0, as in the script
            bo[0] = q[GI_OBJ]; bo[1] = q[GI_OBJ + 1]; bo[2] = q[GI_OBJ + 2] - q[GI_OBJ]; bo[3] = q[GI_OBJ + 3] - q[GI_OBJ + 1];
            bv[0] = q[GI_VIS]; bv[1] = q[GI_VIS + 1]; bv[2] = q[GI_VIS + 2] - q[GI_VIS]; bv[3] = q[GI_VIS + 3] - q[GI_VIS + 1];
        }
    }
    return SUO_OK;
}

}  // namespace suo

using namespace suo;

extern "C" int suo_gt_info(void* h, int n, const int* model_index, const double* T, const double* K, int width, int height, int n_images,
                           const float* depth_test, const int* image_index, double delta, long long* px_counts, int* bbox_obj, int* bbox_visib) {
    return gt_info_run("suo_gt_info", 3, (MeshDb*)h, n, model_index, T, K, width, height, n_images, depth_test, image_index, delta, px_counts, bbox_obj, bbox_visib,
                       nullptr, nullptr);
}

extern "C" int suo_gt_masks(void* h, int n, const int* model_index, const double* T, const double* K, int width, int height, int n_images,
                            const float* depth_test, const int* image_index, double delta, uint8_t* mask, uint8_t* mask_visib) {
    return gt_info_run("suo_gt_masks", 1, (MeshDb*)h, n, model_index, T, K, width, height, n_images, depth_test, image_index, delta, nullptr, nullptr, nullptr, mask,
                       mask_visib);
}
