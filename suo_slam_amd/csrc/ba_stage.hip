// Staging of bundle-adjustment problems (csrc/ba_stage.h): host prep, arena layout, H2D of a batch; D2H and un-sorting of its results.
#include <string.h>

#include <algorithm>

#include "ba_stage.h"
#include "tune.h"

namespace suo {

Arena g_arena;

int Arena::ensure(size_t bytes) {
    if (!stream) {
        // highest priority: the geometry kernels are tiny (8 waves / 1 workgroup) and latency-bound; on its own
        // priority level the stream also gets its own hardware queue instead of sharing one with the CNN's streams.
        int lo = 0, hi = 0;
        SUO_HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
        static const int prio = (int)SUO_TUNE("SUO_GEOM_PRIO", 2);      // 2: highest, 1: default, 0: lowest (A/B only)
        SUO_HIP_CHECK(hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, prio == 2 ? hi : (prio == 0 ? lo : 0)));
    }
    if (bytes <= cap) return SUO_OK;
    size_t ncap = std::max(bytes, cap * 2);
    ncap = (ncap + 4095) & ~(size_t)4095;
    if (dev) (void)hipFree(dev);
    if (host) (void)hipHostFree(host);
    dev = nullptr; host = nullptr; cap = 0;
    SUO_HIP_CHECK(hipMalloc((void**)&dev, ncap));
    SUO_HIP_CHECK(hipHostMalloc((void**)&host, ncap, hipHostMallocDefault));
    cap = ncap;
    return SUO_OK;
}

int prep_problem(const suo_ba_problem& q, int index, Prep& P, const char* who) {
    if (q.n_cam < 0 || q.n_obj < 0 || q.n_edge < 0 || q.n_rounds < 0 || q.n_rounds > 8) { suo_set_error("%s: bad sizes", who); return SUO_ERR_ARG; }
    // sort edges by (cam, obj) pair, stable, so each pair is one contiguous segment
    P.order.resize(q.n_edge);
    for (int e = 0; e < q.n_edge; ++e) {
        if (q.edge_cam[e] < 0 || q.edge_cam[e] >= q.n_cam || q.edge_obj[e] < 0 || q.edge_obj[e] >= q.n_obj) {
            suo_set_error("%s: edge %d of problem %d references a missing vertex", who, e, index);
            return SUO_ERR_ARG;
        }
        P.order[e] = e;
    }
    std::stable_sort(P.order.begin(), P.order.end(), [&](int a, int b) {
        if (q.edge_cam[a] != q.edge_cam[b]) return q.edge_cam[a] < q.edge_cam[b];
        return q.edge_obj[a] < q.edge_obj[b];
    });
    P.edge_pair.resize(q.n_edge);
    for (int k = 0; k < q.n_edge; ++k) {
        const int e = P.order[k];
        if (k == 0 || q.edge_cam[e] != q.edge_cam[P.order[k - 1]] || q.edge_obj[e] != q.edge_obj[P.order[k - 1]]) {
            P.pair_cam.push_back(q.edge_cam[e]);
            P.pair_obj.push_back(q.edge_obj[e]);
            P.pair_start.push_back(k);
        }
        P.edge_pair[k] = (int)P.pair_cam.size() - 1;
    }
    P.pair_start.push_back(q.n_edge);
    const int np = (int)P.pair_cam.size();
    P.cam_ptr.assign(q.n_cam + 1, 0);
    P.obj_ptr.assign(q.n_obj + 1, 0);
    for (int p = 0; p < np; ++p) { P.cam_ptr[P.pair_cam[p] + 1]++; P.obj_ptr[P.pair_obj[p] + 1]++; }
    for (int c = 0; c < q.n_cam; ++c) P.cam_ptr[c + 1] += P.cam_ptr[c];
    for (int o = 0; o < q.n_obj; ++o) P.obj_ptr[o + 1] += P.obj_ptr[o];
    P.cam_idx.resize(np);
    P.obj_idx.resize(np);
    { std::vector<int> cc(P.cam_ptr.begin(), P.cam_ptr.end() - 1), oo(P.obj_ptr.begin(), P.obj_ptr.end() - 1);
      for (int p = 0; p < np; ++p) { P.cam_idx[cc[P.pair_cam[p]]++] = p; P.obj_idx[oo[P.pair_obj[p]]++] = p; } }
    P.cam_obj.assign((size_t)q.n_cam * q.n_obj, -1);                    // dense (camera, object) -> pair lookup for the Schur sums
    for (int p = 0; p < np; ++p) P.cam_obj[(size_t)P.pair_cam[p] * q.n_obj + P.pair_obj[p]] = p;
    return SUO_OK;
}

// The arena layout of a batch, every array on a 16-byte boundary: the structs, then every problem's inputs (one H2D up to in_end), then the outputs that are not
// inputs too (one D2H up to out_end), then device-only scratch.  Each Prep::S gets its sizes and its addresses, counted from `base`; the caller's rooms
// (Staged::room) close the inputs and the scratch.
static void lay_out(const suo_ba_problem* probs, int n_prob, char* base, Staged& st) {
    Layout L;
    L.base = base;
    auto room = [&](int k) { st.room[k] = (char*)((uintptr_t)base + L.take(st.room_bytes[k])); };
    st.o_structs = L.take(sizeof(LmProblem) * (size_t)n_prob);
    for (int i = 0; i < n_prob; ++i) {
        LmProblem& S = st.prep[i].S;
        S = LmProblem();
        S.n_cam = probs[i].n_cam; S.n_obj = probs[i].n_obj; S.n_edge = probs[i].n_edge; S.n_pair = (int)st.prep[i].pair_cam.size();
        const size_t E = S.n_edge, C = S.n_cam, O = S.n_obj, NP = S.n_pair;
        L.put(S.cam_T, 12 * C); L.put(S.obj_T, 12 * O); L.put(S.cam_fixed, C); L.put(S.obj_fixed, O);
        L.put(S.edge_pair, E); L.put(S.edge_k, 4 * E); L.put(S.edge_p, 3 * E); L.put(S.edge_uv, 2 * E); L.put(S.edge_info, 3 * E); L.put(S.edge_inlier, E);
        L.put(S.pair_cam, NP); L.put(S.pair_obj, NP); L.put(S.pair_start, NP + 1);
        L.put(S.cam_pair_ptr, C + 1); L.put(S.cam_pair_idx, NP); L.put(S.obj_pair_ptr, O + 1); L.put(S.obj_pair_idx, NP);
        L.put(S.cam_obj_pair, C * O);
    }
    room(0);
    st.in_end = L.off;
    for (int i = 0; i < n_prob; ++i) { LmProblem& S = st.prep[i].S; L.put(S.edge_chi2, S.n_edge); L.put(S.stats, 4); }
    st.out_end = L.off;
    for (int i = 0; i < n_prob; ++i) {
        LmProblem& S = st.prep[i].S;
        const size_t E = S.n_edge, C = S.n_cam, O = S.n_obj, NP = S.n_pair;
        L.put(S.cam, C); L.put(S.obj, O); L.put(S.cam_bak, C); L.put(S.obj_bak, O);
        L.put(S.err, 2 * E); L.put(S.level, E); L.put(S.pair_part, 90 * NP);
        L.put(S.Hcc, 36 * C); L.put(S.bc, 6 * C); L.put(S.Hoo, 36 * O); L.put(S.bo, 6 * O);
        L.put(S.Hcc_inv, 36 * C); L.put(S.Y, 36 * NP); L.put(S.yc, 6 * C); L.put(S.xc, 6 * C); L.put(S.xo, 6 * O); L.put(S.obj_slot, O);
        L.put(S.jac, 29 * E);
    }
    room(1); room(2);
    st.total = L.off;
}

int prep_problems(const suo_ba_problem* probs, int n_prob, Staged& st, const char* who) {
    st.prep.assign(n_prob, Prep());
    for (int i = 0; i < n_prob; ++i) {
        int rc = prep_problem(probs[i], i, st.prep[i], who);
        if (rc != SUO_OK) return rc;
    }
    return SUO_OK;
}

int stage_problems(const suo_ba_problem* probs, int n_prob, Arena& A, Staged& st, const char* who) {
    int rc = prep_problems(probs, n_prob, st, who);
    if (rc == SUO_OK) rc = stage_prepared(probs, n_prob, A, st);
    return rc != SUO_OK ? rc : upload(A, st);
}

// arena layout + pinned mirror of one prepared batch of problems
int stage_prepared(const suo_ba_problem* probs, int n_prob, Arena& A, Staged& st) {
    lay_out(probs, n_prob, nullptr, st);          // sizes first: the arena may move when it grows
    int rc = A.ensure(st.total);
    if (rc != SUO_OK) return rc;
    lay_out(probs, n_prob, A.dev, st);
    for (int i = 0; i < n_prob; ++i) {
        const suo_ba_problem& q = probs[i];
        Prep& P = st.prep[i];
        LmProblem& S = P.S;
        const int E = q.n_edge, np = S.n_pair;
        memcpy(A.mirror(S.cam_T), q.cam_T, sizeof(double) * 12 * q.n_cam);
        memcpy(A.mirror(S.obj_T), q.obj_T, sizeof(double) * 12 * q.n_obj);
        memcpy(A.mirror(S.cam_fixed), q.cam_fixed, q.n_cam);
        memcpy(A.mirror(S.obj_fixed), q.obj_fixed, q.n_obj);
        memcpy(A.mirror(S.edge_pair), P.edge_pair.data(), sizeof(int) * E);
        double* ek = A.mirror(S.edge_k); double* ep = A.mirror(S.edge_p); double* euv = A.mirror(S.edge_uv); double* ei = A.mirror(S.edge_info);
        uint8_t* inl = A.mirror(S.edge_inlier);
        for (int k = 0; k < E; ++k) {
            const int e = P.order[k];
            memcpy(ek + 4 * k, q.edge_camk + 4 * e, sizeof(double) * 4);
            memcpy(ep + 3 * k, q.edge_p + 3 * e, sizeof(double) * 3);
            memcpy(euv + 2 * k, q.edge_uv + 2 * e, sizeof(double) * 2);
            memcpy(ei + 3 * k, q.edge_info + 3 * e, sizeof(double) * 3);
            inl[k] = q.edge_inlier[e];
        }
        memcpy(A.mirror(S.pair_cam), P.pair_cam.data(), sizeof(int) * np);
        memcpy(A.mirror(S.pair_obj), P.pair_obj.data(), sizeof(int) * np);
        memcpy(A.mirror(S.pair_start), P.pair_start.data(), sizeof(int) * (np + 1));
        memcpy(A.mirror(S.cam_pair_ptr), P.cam_ptr.data(), sizeof(int) * (q.n_cam + 1));
        memcpy(A.mirror(S.cam_pair_idx), P.cam_idx.data(), sizeof(int) * np);
        memcpy(A.mirror(S.obj_pair_ptr), P.obj_ptr.data(), sizeof(int) * (q.n_obj + 1));
        memcpy(A.mirror(S.obj_pair_idx), P.obj_idx.data(), sizeof(int) * np);
        memcpy(A.mirror(S.cam_obj_pair), P.cam_obj.data(), sizeof(int) * P.cam_obj.size());
        for (int k = 0; k < 8; ++k) S.its[k] = k < q.n_rounds ? q.its[k] : 0;
        S.n_rounds = q.n_rounds; S.init_with_outliers = q.init_with_outliers; S.chi2_thr = q.chi2_thr; S.huber_delta = q.huber_delta;
    }
    return SUO_OK;
}

int upload(Arena& A, Staged& st, bool with_room) {
    for (size_t i = 0; i < st.prep.size(); ++i) memcpy(A.host + st.o_structs + sizeof(LmProblem) * i, &st.prep[i].S, sizeof(LmProblem));
    SUO_HIP_CHECK(hipMemcpyAsync(A.dev, A.host, with_room ? st.in_end : (size_t)(st.room[0] - A.dev), hipMemcpyHostToDevice, A.stream));
    return SUO_OK;
}

int upload_room(Arena& A, Staged& st) {
    SUO_HIP_CHECK(hipMemcpyAsync(st.room[0], A.mirror(st.room[0]), st.room_bytes[0], hipMemcpyHostToDevice, A.stream));
    return SUO_OK;
}

// D2H of poses / inlier flags / chi2 / stats and un-sorting into the caller's arrays
int fetch_results(suo_ba_problem* probs, int n_prob, Arena& A, Staged& st) {
    SUO_HIP_CHECK(hipMemcpyAsync(A.host, A.dev, st.out_end, hipMemcpyDeviceToHost, A.stream));
    SUO_HIP_CHECK(hipStreamSynchronize(A.stream));
    for (int i = 0; i < n_prob; ++i) {
        suo_ba_problem& q = probs[i];
        const Prep& P = st.prep[i];
        memcpy(q.cam_T, A.mirror(P.S.cam_T), sizeof(double) * 12 * q.n_cam);
        memcpy(q.obj_T, A.mirror(P.S.obj_T), sizeof(double) * 12 * q.n_obj);
        const uint8_t* inl = A.mirror(P.S.edge_inlier);
        const double* chi2 = A.mirror(P.S.edge_chi2);
        for (int k = 0; k < q.n_edge; ++k) {
            const int e = P.order[k];
            q.edge_inlier[e] = inl[k];
            if (q.edge_chi2) q.edge_chi2[e] = chi2[k];
        }
        memcpy(q.stats, A.mirror(P.S.stats), sizeof(int) * 4);
        if (q.stats[0] < 0) {
            suo_set_error("suo_optimize: %d free objects with free cameras exceeds the Schur limit of 16", q.n_obj);
            return SUO_ERR_ARG;
        }
    }
    return SUO_OK;
}

}  // namespace suo
