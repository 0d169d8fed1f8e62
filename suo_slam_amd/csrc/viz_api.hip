// Host entries of a view's visualisation (include/suo_hip.h): suo_viz_create / _destroy / _view / _colours over the kernels of csrc/viz.hip.  suo_viz_view
// checks every argument before anything is launched, packs the descriptor into one pinned block (a ring of SUO_VIZ_RING), and enqueues one copy, the clearing
// of the owner plane and the two kernels on the caller's stream; it never waits for the device.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/suo_hip.h"
#include "suo_internal.h"
#include "mesh_db.h"
#include "viz.h"

namespace suo {

// kp_config.kp_colors() and utils.bbox_color()'s table (BGR), recorded from the reference as data: tests/golden/viz_golden.npz holds both, tests/test_viz_ref.py compares
static const uint8_t VIZ_KP_BGR[VIZ_KP_COLOURS][3] = {
    {0,255,243}, {255,23,0}, {102,255,0}, {255,0,150}, {40,0,255}, {172,255,0}, {0,61,255}, {255,61,0}, {255,164,0}, {191,0,255}, {0,131,255},
    {255,0,253}, {0,255,0}, {223,0,255}, {0,196,255}, {32,255,0}, {0,255,102}, {0,93,255}, {255,94,0}, {255,235,0}, {255,0,79}, {255,197,0},
    {0,255,70}, {0,23,255}, {255,0,215}, {0,164,255}, {204,255,0}, {69,255,0}, {0,255,32}, {255,0,8}, {139,255,0}, {0,255,172}, {0,255,140},
    {255,0,112}, {0,255,205}, {0,234,255}, {255,0,182}, {241,255,0}, {255,0,41}, {255,132,0}, {8,0,255}};
static const uint8_t VIZ_BOX_BGR[VIZ_BOX_COLOURS][3] = {
    {40,0,255}, {0,1,255}, {0,50,255}, {0,99,255}, {0,147,255}, {0,196,255}, {0,239,255}, {0,255,221}, {0,255,172}, {0,255,124}, {0,255,75},
    {0,255,27}, {16,255,0}, {64,255,0}, {112,255,0}, {161,255,0}, {209,255,0}, {255,251,0}, {255,208,0}, {255,159,0}, {255,110,0}, {255,61,0},
    {255,12,0}, {255,0,36}, {255,0,79}, {255,0,128}, {255,0,177}, {255,0,226}, {234,0,255}, {191,0,255}};

constexpr size_t viz_align(size_t b) { return (b + 15) & ~(size_t)15; }
// one slot of the staging, at its largest
constexpr size_t VIZ_SLOT_BYTES = viz_align((size_t)SUO_VIZ_MAX_OBJ * VIZ_BOX_INTS * 4) + viz_align((size_t)SUO_VIZ_MAX_KP * VIZ_STAMP_INTS * 4) +
                                  viz_align((size_t)SUO_VIZ_MAX_KP * sizeof(VizKp)) + viz_align((size_t)SUO_VIZ_MAX_OBJ * sizeof(VizOverlay));

}  // namespace suo

using namespace suo;

struct suo_viz {
    int H = 0, W = 0;
    int* owner = nullptr;            // [H][W]
    char* dev = nullptr;             // one slot
    char* host = nullptr;            // SUO_VIZ_RING slots, pinned
    int next = 0;
};

extern "C" int suo_viz_colours(uint8_t* kp_bgr, uint8_t* box_bgr) {
    if (!kp_bgr || !box_bgr) { suo_set_error("suo_viz_colours: null pointer"); return SUO_ERR_ARG; }
    memcpy(kp_bgr, VIZ_KP_BGR, sizeof(VIZ_KP_BGR));
    memcpy(box_bgr, VIZ_BOX_BGR, sizeof(VIZ_BOX_BGR));
    return SUO_OK;
}

extern "C" void suo_viz_destroy(suo_viz* v) {
    if (!v) return;
    if (v->owner) (void)hipFree(v->owner);
    if (v->dev) (void)hipFree(v->dev);
    if (v->host) (void)hipHostFree(v->host);
    delete v;
}

extern "C" int suo_viz_create(int H, int W, suo_viz** out) {
    if (!out) { suo_set_error("suo_viz_create: null pointer"); return SUO_ERR_ARG; }
    *out = nullptr;
    if (H < 1 || W < 1 || (long long)H * W >= (1LL << 31)) { suo_set_error("suo_viz_create: bad size %d x %d (H, W >= 1 and H W < 2^31)", H, W); return SUO_ERR_ARG; }
    int rc = viz_upload_tables(&VIZ_KP_BGR[0][0]);
    if (rc) return rc;
    suo_viz* v = new suo_viz;
    v->H = H; v->W = W;
    if (hipMalloc((void**)&v->owner, (size_t)H * W * sizeof(int)) != hipSuccess || hipMalloc((void**)&v->dev, VIZ_SLOT_BYTES) != hipSuccess ||
        hipHostMalloc((void**)&v->host, VIZ_SLOT_BYTES * SUO_VIZ_RING, hipHostMallocDefault) != hipSuccess) {
        suo_set_error("suo_viz_create: allocation failed (%d x %d)", H, W);
        suo_viz_destroy(v);
        return SUO_ERR_HIP;
    }
    *out = v;
    return SUO_OK;
}

extern "C" int suo_viz_view(suo_viz* v, const suo_viz_view_desc* d, void* mesh_db, uint8_t* out_dev, void* stream) {
    const char* who = "suo_viz_view";
    if (!v || !d || !out_dev) { suo_set_error("%s: null pointer", who); return SUO_ERR_ARG; }
    if (!d->frame) { suo_set_error("%s: null frame", who); return SUO_ERR_ARG; }
    if (d->n_box < 0 || d->n_stamp < 0 || d->n_kp < 0 || d->n_overlay < 0) { suo_set_error("%s: negative count", who); return SUO_ERR_ARG; }
    if (d->n_kp > SUO_VIZ_MAX_KP || d->n_stamp > SUO_VIZ_MAX_KP) {
        suo_set_error("%s: %d keypoints and %d prior stamps exceed the %d (16 objects x 41 keypoints) of one view", who, d->n_kp, d->n_stamp, SUO_VIZ_MAX_KP);
        return SUO_ERR_ARG;
    }
    if (d->n_box > SUO_VIZ_MAX_OBJ || d->n_overlay > SUO_VIZ_MAX_OBJ) {
        suo_set_error("%s: %d boxes and %d overlay objects exceed the %d of one view", who, d->n_box, d->n_overlay, SUO_VIZ_MAX_OBJ);
        return SUO_ERR_ARG;
    }
    if ((d->n_box && !d->box) || (d->n_stamp && !d->stamp) || (d->n_kp && (!d->kp || !d->kp_cs)) ||
        (d->n_overlay && (!d->overlay_model || !d->overlay_colour || !d->overlay_T || !d->overlay_K))) {
        suo_set_error("%s: null array with a positive count", who);
        return SUO_ERR_ARG;
    }
    for (int i = 0; i < d->n_stamp; ++i)
        if (d->stamp[i * VIZ_STAMP_INTS] < 0 || d->stamp[i * VIZ_STAMP_INTS] >= VIZ_KP_COLOURS) {
            suo_set_error("%s: stamp %d has channel %d", who, i, d->stamp[i * VIZ_STAMP_INTS]);
            return SUO_ERR_ARG;
        }
    constexpr int R_MAX = 1 << 20;
    for (int i = 0; i < d->n_kp; ++i) {
        const int32_t* q = d->kp + (size_t)i * 8;
        if (q[2] < 0 || q[3] < 0 || q[2] > R_MAX || q[3] > R_MAX || (q[5] && (q[6] < 0 || q[7] < 0 || q[6] > R_MAX || q[7] > R_MAX))) {
            suo_set_error("%s: keypoint %d has a radius or half-axis outside [0, 2^20]", who, i);
            return SUO_ERR_ARG;
        }
        if (q[5] && (!std::isfinite(d->kp_cs[2 * i]) || !std::isfinite(d->kp_cs[2 * i + 1]))) {
            suo_set_error("%s: keypoint %d has a non-finite ellipse direction", who, i);
            return SUO_ERR_ARG;
        }
    }
    MeshDb* db = (MeshDb*)mesh_db;
    if (d->n_overlay && !db) { suo_set_error("%s: overlay objects without a mesh database", who); return SUO_ERR_ARG; }
    for (int i = 0; i < d->n_overlay; ++i)
        if (d->overlay_model[i] < 0 || d->overlay_model[i] >= db->n_models) {
            suo_set_error("%s: overlay %d has model index %d outside [0, %d)", who, i, d->overlay_model[i], db->n_models);
            return SUO_ERR_ARG;
        }

    // the slot: boxes | stamps (sorted by channel, stable) | keypoints | overlays
    const size_t o_box = 0, o_stamp = o_box + viz_align((size_t)d->n_box * VIZ_BOX_INTS * 4), o_kp = o_stamp + viz_align((size_t)d->n_stamp * VIZ_STAMP_INTS * 4),
                 o_ov = o_kp + viz_align((size_t)d->n_kp * sizeof(VizKp)), total = o_ov + viz_align((size_t)d->n_overlay * sizeof(VizOverlay));
    char* h = v->host + (size_t)v->next * VIZ_SLOT_BYTES;
    v->next = (v->next + 1) % SUO_VIZ_RING;
    if (d->n_box) memcpy(h + o_box, d->box, (size_t)d->n_box * VIZ_BOX_INTS * 4);
    {
        std::vector<int> order(d->n_stamp);
        for (int i = 0; i < d->n_stamp; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [d](int p, int q) { return d->stamp[p * VIZ_STAMP_INTS] < d->stamp[q * VIZ_STAMP_INTS]; });
        int* st = (int*)(h + o_stamp);
        for (int i = 0; i < d->n_stamp; ++i) memcpy(st + (size_t)i * VIZ_STAMP_INTS, d->stamp + (size_t)order[i] * VIZ_STAMP_INTS, VIZ_STAMP_INTS * 4);
    }
    VizKp* kp = (VizKp*)(h + o_kp);
    for (int i = 0; i < d->n_kp; ++i) {
        const int32_t* q = d->kp + (size_t)i * 8;
        kp[i] = VizKp{q[0], q[1], q[2], q[3], q[4], q[5] != 0, q[5] ? q[6] : 0, q[5] ? q[7] : 0, q[5] ? d->kp_cs[2 * i] : 1.0, q[5] ? d->kp_cs[2 * i + 1] : 0.0};
    }
    VizOverlay* ov = (VizOverlay*)(h + o_ov);
    int max_pts = 0;
    for (int i = 0; i < d->n_overlay; ++i) {
        const int m = d->overlay_model[i];
        memcpy(ov[i].T, d->overlay_T + (size_t)i * 12, sizeof(ov[i].T));
        memcpy(ov[i].K, d->overlay_K + (size_t)i * 9, sizeof(ov[i].K));
        ov[i].first = db->off[m]; ov[i].count = db->off[m + 1] - db->off[m]; ov[i].colour = d->overlay_colour[i]; ov[i].pad = 0;
        max_pts = std::max(max_pts, ov[i].count);
    }

    hipStream_t s = (hipStream_t)stream;
    if (total) SUO_HIP_CHECK(hipMemcpyAsync(v->dev, h, total, hipMemcpyHostToDevice, s));
    if (d->n_overlay) SUO_HIP_CHECK(hipMemsetAsync(v->owner, 0, (size_t)v->H * v->W * sizeof(int), s));
    VizArgs a;
    a.frame = d->frame; a.out = out_dev; a.H = v->H; a.W = v->W;
    a.box = (const int*)(v->dev + o_box); a.n_box = d->n_box;
    a.stamp = (const int*)(v->dev + o_stamp); a.n_stamp = d->n_stamp;
    a.kp = (const VizKp*)(v->dev + o_kp); a.n_kp = d->n_kp;
    a.ov = (const VizOverlay*)(v->dev + o_ov); a.n_ov = d->n_overlay; a.max_pts = max_pts;
    a.pts = db ? db->pts_dev : nullptr;
    a.owner = v->owner;
    return viz_enqueue(a, s);
}
