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
// inputs too (one D2H up to out_end), then device-only scratch.  Each Prep::S gets its sizes and its addresses, counted from `base`.
static void lay_out(const suo_ba_problem* probs, int n_prob, const int* cov_form, const CovPairs* pairs, bool resid, size_t extra, char* base, Staged& st) {
    Layout L;
    auto put = [&](auto*& p, size_t n) { p = (std::remove_reference_t<decltype(p)>)((uintptr_t)base + L.take(sizeof(*p) * n)); };
    st.o_structs = L.take(sizeof(LmProblem) * (size_t)n_prob);
    st.o_rs = L.take(resid ? sizeof(RsProblem) * (size_t)n_prob : 0);
    for (int i = 0; i < n_prob; ++i) {
        LmProblem& S = st.prep[i].S;
        S = LmProblem();
        S.n_cam = probs[i].n_cam; S.n_obj = probs[i].n_obj; S.n_edge = probs[i].n_edge; S.n_pair = (int)st.prep[i].pair_cam.size();
        const size_t E = S.n_edge, C = S.n_cam, O = S.n_obj, NP = S.n_pair;
        put(S.cam_T, 12 * C); put(S.obj_T, 12 * O); put(S.cam_fixed, C); put(S.obj_fixed, O);
        put(S.edge_pair, E); put(S.edge_k, 4 * E); put(S.edge_p, 3 * E); put(S.edge_uv, 2 * E); put(S.edge_info, 3 * E); put(S.edge_inlier, E);
        put(S.pair_cam, NP); put(S.pair_obj, NP); put(S.pair_start, NP + 1);
        put(S.cam_pair_ptr, C + 1); put(S.cam_pair_idx, NP); put(S.obj_pair_ptr, O + 1); put(S.obj_pair_idx, NP);
        put(S.cam_obj_pair, C * O);
        S.n_cpair = pairs ? pairs->n[i] : 0;
        put(S.cpair_a, (size_t)S.n_cpair); put(S.cpair_b, (size_t)S.n_cpair);
        RsProblem& R = st.prep[i].R;
        R = RsProblem();
        if (resid) { put(R.order, E); put(R.vptr, C + O + 1); put(R.vedge, 2 * E); }
    }
    st.in_end = L.off;
    for (int i = 0; i < n_prob; ++i) { LmProblem& S = st.prep[i].S; put(S.edge_chi2, S.n_edge); put(S.stats, 4); }
    st.out_end = L.off;
    for (int i = 0; i < n_prob; ++i) {
        LmProblem& S = st.prep[i].S;
        const size_t E = S.n_edge, C = S.n_cam, O = S.n_obj, NP = S.n_pair;
        put(S.cam, C); put(S.obj, O); put(S.cam_bak, C); put(S.obj_bak, O);
        put(S.err, 2 * E); put(S.level, E); put(S.pair_part, 90 * NP);
        put(S.Hcc, 36 * C); put(S.bc, 6 * C); put(S.Hoo, 36 * O); put(S.bo, 6 * O);
        put(S.Hcc_inv, 36 * C); put(S.Y, 36 * NP); put(S.yc, 6 * C); put(S.xc, 6 * C); put(S.xo, 6 * O); put(S.obj_slot, O);
        put(S.jac, 29 * E);
    }
    st.cov_begin = L.off;
    for (int i = 0; i < n_prob; ++i) { LmProblem& S = st.prep[i].S; put(S.cam_cov, 36 * (size_t)S.n_cam); put(S.obj_cov, 36 * (size_t)S.n_obj); put(S.cov_status, 3);
                                       put(S.cov_cross, 36 * (size_t)S.n_cpair); put(S.cov_rel, 36 * (size_t)S.n_cpair);
                                       if (!resid) continue;
                                       const size_t E = S.n_edge, V = (size_t)S.n_cam + S.n_obj;
                                       RsProblem& R = st.prep[i].R;
                                       put(R.chi2, E); put(R.pcov, 3 * E); put(R.lev, E); put(R.t, E); put(R.flag, E); put(R.vstat, 3 * V);
                                       put(R.summary, 6); put(R.status, 2); }
    st.cov_end = L.off;
    // cov_form 3 (csrc/pose_cov_graph.hip): the reduced system, its inverse and every camera's Z in device memory, sized by the free objects -- no slot limit
    for (int i = 0; cov_form && i < n_prob; ++i) {
        if (cov_form[i] != 3) continue;
        LmProblem& S = st.prep[i].S;
        size_t nsm = 0;
        for (int o = 0; o < S.n_obj; ++o) nsm += probs[i].obj_fixed[o] ? 0 : 6;
        put(S.cov_S, nsm * (nsm + 1)); put(S.cov_Sinv, nsm * nsm); put(S.cov_Z, 6 * (size_t)S.n_cam * nsm); put(S.cov_hdr, 2 + (size_t)S.n_obj);
    }
    st.o_extra = L.take(extra);
    st.total = L.off;
}

// host prep + arena layout + H2D of one batch of problems
int stage_problems(const suo_ba_problem* probs, int n_prob, Arena& A, Staged& st, const char* who, const int* cov_form, const CovPairs* pairs, bool resid,
                   size_t extra) {
    st.prep.assign(n_prob, Prep());
    for (int i = 0; i < n_prob; ++i) {
        int rc = prep_problem(probs[i], i, st.prep[i], who);
        if (rc != SUO_OK) return rc;
    }
    lay_out(probs, n_prob, cov_form, pairs, resid, extra, nullptr, st);          // sizes first: the arena may move when it grows
    int rc = A.ensure(st.total);
    if (rc != SUO_OK) return rc;
    lay_out(probs, n_prob, cov_form, pairs, resid, extra, A.dev, st);
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
        S.cov_form = cov_form ? cov_form[i] : 0;
        if (S.n_cpair > 0) {
            memcpy(A.mirror(S.cpair_a), pairs->a[i], sizeof(int) * S.n_cpair);
            memcpy(A.mirror(S.cpair_b), pairs->b[i], sizeof(int) * S.n_cpair);
        }
        if (resid) {
            // every vertex's edges by the caller's index, ascending: the order the per-vertex sums of csrc/resid_stats.hip walk
            memcpy(A.mirror(P.R.order), P.order.data(), sizeof(int) * E);
            int* vptr = A.mirror(P.R.vptr); int* vedge = A.mirror(P.R.vedge);
            const int V = q.n_cam + q.n_obj;
            std::fill(vptr, vptr + V + 1, 0);
            for (int e = 0; e < E; ++e) { vptr[q.edge_cam[e] + 1]++; vptr[q.n_cam + q.edge_obj[e] + 1]++; }
            for (int v = 0; v < V; ++v) vptr[v + 1] += vptr[v];
            std::vector<int> at(vptr, vptr + V);
            for (int e = 0; e < E; ++e) { vedge[at[q.edge_cam[e]]++] = e; vedge[at[q.n_cam + q.edge_obj[e]]++] = e; }
            memcpy(A.host + st.o_rs + sizeof(RsProblem) * (size_t)i, &P.R, sizeof(RsProblem));
        }
        memcpy(A.host + st.o_structs + sizeof(LmProblem) * (size_t)i, &S, sizeof(LmProblem));
    }
    SUO_HIP_CHECK(hipMemcpyAsync(A.dev, A.host, st.in_end, hipMemcpyHostToDevice, A.stream));
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
