// Host entry of row N8: suo_model_info (include/suo_hip.h) over the kernels of csrc/model_info.hip.  Every argument is checked before anything is launched;
// the call stages its items into the database's scratch under db->mu, runs on db->stream and blocks; the outputs are written only once the device is done.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <vector>

#include "../../include/suo_hip.h"
#include "suo_internal.h"
#include "mesh_db.h"
#include "model_info.h"

using namespace suo;

extern "C" void suo_model_info_tiles(int* tile, int* itile) {
    if (tile) *tile = MI_TILE;
    if (itile) *itile = MI_ITILE;
}

extern "C" int suo_model_info(void* h, int n, const int* model_index, double* info_out, int* pair_out, int* flags_out) {
    MeshDb* db = (MeshDb*)h;
    if (!db) { suo_set_error("suo_model_info: null mesh database"); return SUO_ERR_ARG; }
    if (n < 0) { suo_set_error("suo_model_info: n = %d is negative", n); return SUO_ERR_ARG; }
    if (n == 0) return SUO_OK;
    if (!model_index || !info_out) { suo_set_error("suo_model_info: null model_index or info_out"); return SUO_ERR_ARG; }
    int pmax = 0, rc;
    if ((rc = check_model_index("suo_model_info", db, n, model_index, &pmax))) return rc;
    for (int i = 0; i < n; ++i)
        if (db->off[model_index[i] + 1] - db->off[model_index[i]] < 1) { suo_set_error("suo_model_info: model %d has no points", model_index[i]); return SUO_ERR_ARG; }
    std::lock_guard<std::mutex> lk(db->mu);
    // staged, in this order: first[n + 1] | dmax[n] | pairkey[n] | model[n] | flags[n] | box[n][6]   then, with the pair, written by the device: tmax[total]
    const size_t o_first = 0, o_dmax = o_first + (size_t)(n + 1) * 8, o_key = o_dmax + (size_t)n * 8, o_model = o_key + (size_t)n * 8, o_flags = o_model + (size_t)n * 4,
                 o_box = o_flags + (size_t)n * 4, staged = (o_box + (size_t)n * 24 + 15) & ~(size_t)15;
    std::vector<long long> first((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i) first[i + 1] = first[i] + mi_items(db->off[model_index[i] + 1] - db->off[model_index[i]]);
    const long long total = first[n];
    const size_t need = staged + (pair_out ? (size_t)total * 8 : 0);
    if ((rc = ensure_scratch(db, need))) return rc;
    char* hs = db->scratch_host;
    memcpy(hs + o_first, first.data(), (size_t)(n + 1) * 8);
    memset(hs + o_dmax, 0, (size_t)n * 8);                       // +0.0: the identity of max over d^2 >= 0
    memset(hs + o_key, 0xff, (size_t)n * 8);
    memcpy(hs + o_model, model_index, (size_t)n * 4);
    memset(hs + o_flags, 0, (size_t)n * 4);
    unsigned* bh = (unsigned*)(hs + o_box);
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < 6; ++c) bh[(size_t)i * 6 + c] = c < 3 ? 0xffffffffu : 0u;
    SUO_HIP_CHECK(hipMemcpyAsync(db->scratch_dev, hs, staged, hipMemcpyHostToDevice, db->stream));
    ModelInfoArgs g;
    char* ds = db->scratch_dev;
    g.pts = db->pts_dev; g.off = db->off_dev;
    g.first = (const long long*)(ds + o_first); g.dmax = (unsigned long long*)(ds + o_dmax);
    g.pairkey = pair_out ? (unsigned long long*)(ds + o_key) : nullptr;
    g.model = (const int*)(ds + o_model); g.flags = (unsigned*)(ds + o_flags); g.box = (unsigned*)(ds + o_box);
    g.tmax = pair_out ? (unsigned long long*)(ds + staged) : nullptr;
    g.n = n; g.total = total;
    model_info_enqueue(g, pmax, db->stream);
    SUO_HIP_CHECK(hipGetLastError());
    SUO_HIP_CHECK(hipMemcpyAsync(hs + o_dmax, ds + o_dmax, staged - o_dmax, hipMemcpyDeviceToHost, db->stream));
    SUO_HIP_CHECK(hipStreamSynchronize(db->stream));
    const unsigned long long* dmax = (const unsigned long long*)(hs + o_dmax);
    const unsigned long long* key = (const unsigned long long*)(hs + o_key);
    const unsigned* fl = (const unsigned*)(hs + o_flags);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int i = 0; i < n; ++i) {
        double* o = info_out + (size_t)i * 7;
        const bool bad = (fl[i] & 1u) != 0;
        if (flags_out) flags_out[i] = bad ? 1 : 0;
        if (bad) {
            for (int c = 0; c < 7; ++c) o[c] = nan;
            if (pair_out) pair_out[2 * i] = pair_out[2 * i + 1] = -1;
            continue;
        }
        for (int c = 0; c < 3; ++c) {
            const unsigned lo = mi_unkey(bh[(size_t)i * 6 + c]), hi = mi_unkey(bh[(size_t)i * 6 + 3 + c]);
            float flo, fhi;
            memcpy(&flo, &lo, 4); memcpy(&fhi, &hi, 4);
            o[c] = (double)flo;
            o[3 + c] = (double)fhi - (double)flo;
        }
        double d2;
        memcpy(&d2, &dmax[i], 8);
        o[6] = sqrt(d2);
        if (pair_out) { pair_out[2 * i] = (int)(key[i] >> 32); pair_out[2 * i + 1] = (int)(key[i] & 0xffffffffull); }
    }
    return SUO_OK;
}
