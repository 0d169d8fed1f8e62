// Drivers of the LM schedule over the phase kernels of a suo_ba_ctx (csrc/ba_ctx.hip): host-driven (optimize_phasewise), one rank under the device-resident
// schedule (optimize_phases_one_rank, the PHASES route of suo_optimize_batch), N ranks with collectives (suo_optimize_dist, suo_optimize_partitioned).
#include <math.h>
#include <string.h>

#include <algorithm>

#include "ba_comm.h"
#include "ba_stage.h"
#include "lm_schedule.h"
#include "tune.h"

using namespace suo;

// Exchange buffers of a driver of the device-resident schedule: one grow-only device block on the context's device + 16 pinned doubles the host looks at,
// process-wide under their own lock.  One instance per driver, so suo_optimize and suo_optimize_dist do not serialise each other.
struct BaExchange {
    std::mutex mu;
    double* d_buf = nullptr; size_t d_cap = 0; double* h_pin = nullptr; int dev = -1;
    int ensure(size_t need, int device) {
        if (need > d_cap || dev != device) {
            if (d_buf) (void)hipFree(d_buf);
            d_buf = nullptr; d_cap = 0;
            SUO_HIP_CHECK(hipMalloc((void**)&d_buf, need * sizeof(double)));
            d_cap = need; dev = device;
        }
        if (!h_pin) SUO_HIP_CHECK(hipHostMalloc((void**)&h_pin, 16 * sizeof(double), hipHostMallocPortable));
        return SUO_OK;
    }
    int look(const double* src, int n, hipStream_t s) {            // n <= 16 doubles of the device -> h_pin, stream drained
        SUO_HIP_CHECK(hipMemcpyAsync(h_pin, src, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
        SUO_HIP_CHECK(hipStreamSynchronize(s));
        return SUO_OK;
    }
};
// destroys a driver's contexts on every way out (the driver's stream first, when it is set: its queued launches read every context's buffers)
struct BaCtxGuard {
    std::vector<suo_ba_ctx*> c; hipStream_t s = nullptr;
    ~BaCtxGuard() { if (s) (void)hipStreamSynchronize(s); for (suo_ba_ctx* k : c) suo_ba_ctx_destroy(k); }
};

// ---- graphs whose reduced system does not fit the single-kernel paths (more than 16 free objects next to free cameras) ----
// The phase kernels above under g2o's LM schedule (optimization_algorithm_levenberg.cpp:58-150) and the robust rounds of
// ObjectSLAM.optimize (lib/object_slam.py:842-896), driven from the host: the one-rank form of suo_slam_amd/ba_dist.py.
int suo::optimize_phasewise(suo_ba_problem* q) {
    suo_ba_ctx* c = nullptr;
    int rc = ba_ctx_create(q, &c, "suo_optimize");
    if (rc != SUO_OK) return rc;
    BaCtxGuard guard{{c}};
    const int O = q->n_obj, ns = c->ns;
    std::vector<double> lin(2 + 27 * (size_t)O), sch((size_t)ns * ns + ns + 1), tot(27 * (size_t)O + (size_t)ns * ns + ns);
    double good = 0, red[4];
    int rounds = 0, lm_its = 0, lm_trials = 0, num_good = q->n_edge;
    if (q->init_with_outliers) { rc = suo_ba_classify(c, 1, &good); if (rc) return rc; }
    else { rc = suo_ba_classify(c, 0, &good); if (rc) return rc; num_good = (int)(good + 0.5); }
    bool robust_on = true;
    const int drop = lm_drop_round(q->n_rounds);
    for (int rnd = 0; rnd < q->n_rounds; ++rnd) {
        if (lm_round_exit(q->n_edge, num_good)) break;
        ++rounds;
        double lam = -1, ni = 2;
        // (unlike every other form of the schedule this loop does not ask whether any edge is active before it iterates: kept as it was)
        for (int it = 0; it < q->its[rnd]; ++it) {
            rc = suo_ba_linearize(c, robust_on, lin.data()); if (rc) return rc;
            double current_chi = lin[0];
            const double* HB = lin.data() + 1;
            if (it == 0) {                                          // computeLambdaInit: tau * max |diag H| over all free vertices
                double maxd = lin[1 + 27 * (size_t)O];
                for (int o = 0; o < O; ++o)
                    if (!q->obj_fixed[o]) for (int d = 0; d < 6; ++d) maxd = std::max(maxd, fabs(HB[27 * o + diag21[d]]));
                lam = lm_lambda_init(maxd); ni = 2;
            }
            LmTrials tr;
            do {
                rc = suo_ba_schur(c, lam, sch.data()); if (rc) return rc;
                double temp_chi = LM_CHI2_FAILED, scale = 0;
                if (sch[(size_t)ns * ns + ns] > 0.5) {
                    memcpy(tot.data(), HB, 27 * (size_t)O * sizeof(double));
                    memcpy(tot.data() + 27 * (size_t)O, sch.data(), ((size_t)ns * ns + ns) * sizeof(double));
                    rc = suo_ba_solve_update(c, lam, robust_on, tot.data(), red); if (rc) return rc;
                    if (red[3] > 0.5) { temp_chi = red[0]; scale = red[1] + red[2]; }
                }
                if (!tr.verdict<true>(lam, ni, current_chi, temp_chi, scale)) {
                    rc = suo_ba_restore(c); if (rc) return rc;
                    if (!tr.lam_finite) break;
                }
                tr.count(); ++lm_trials;
            } while (tr.another());
            ++lm_its;
            if (tr.terminate()) break;
        }
        rc = suo_ba_classify(c, 0, &good); if (rc) return rc;
        num_good = (int)(good + 0.5);
        if (rnd == drop) robust_on = false;
    }
    rc = suo_ba_ctx_download(c, q);
    q->stats[0] = rounds; q->stats[1] = lm_its; q->stats[2] = lm_trials; q->stats[3] = num_good;
    return rc;
}

// Units enqueued between two looks at the control block: a dead unit (enqueued past the end of a round) is ~50 us of empty launches on one rank and three
// all-reduces more on several, so the batches are half as long there.  The one place the constant lives (suo_slam_amd/ba_dist.py asks suo_ba_units_per_look).
static int ba_units_per_look(int world) { return (int)SUO_TUNE("SUO_BA_UNITS_PER_LOOK", world == 1 ? 12 : 6); }
int suo_ba_units_per_look(int world) { return ba_units_per_look(world < 1 ? 1 : world); }

// The robust rounds of ObjectSLAM.optimize over the device-resident LM schedule, shared by the one-rank route and the partitioned driver: units are enqueued blindly,
// `its` of them cover a round whose every trial is accepted, a rejected trial costs one more, and the host looks at the control block once per batch.
//   classify(keep_all, &n_good)  chi2 classification, the inlier count over ALL ranks      begin(its)  start of a round
//   unit(robust_on)              one unit of the schedule (with its collectives, if any)    look_ctl()  the control block's 16 doubles -> h_ctl, stream drained
template <class Classify, class Begin, class Unit, class Look>
static int lm_rounds(const suo_ba_problem* q, int batch, const double* h_ctl, int stats[4], Classify classify, Begin begin, Unit unit, Look look_ctl) {
    int rc, rounds = 0, lm_its = 0, lm_trials = 0, num_good = q->n_edge, tmp = 0;
    if (q->init_with_outliers) { rc = classify(1, &tmp); if (rc) return rc; }
    else { rc = classify(0, &num_good); if (rc) return rc; }
    int robust_on = 1;
    const int drop = lm_drop_round(q->n_rounds);
    for (int rnd = 0; rnd < q->n_rounds; ++rnd) {
        if (lm_round_exit(q->n_edge, num_good)) break;
        ++rounds;
        const int its = q->its[rnd];
        rc = begin(its); if (rc) return rc;
        int budget = std::min(its, batch);
        bool done = its <= 0;
        while (!done) {
            for (int u = 0; u < budget; ++u) { rc = unit(robust_on); if (rc) return rc; }
            rc = look_ctl(); if (rc) return rc;
            done = (int)h_ctl[3] == 2;
            budget = std::min(std::max(1, its - (int)h_ctl[4]) + 1, batch);
        }
        lm_its = (int)h_ctl[7]; lm_trials = (int)h_ctl[8];
        rc = classify(0, &num_good); if (rc) return rc;
        if (rnd == drop) robust_on = 0;
    }
    stats[0] = rounds; stats[1] = lm_its; stats[2] = lm_trials; stats[3] = num_good;
    return SUO_OK;
}

// One rank, device-resident schedule, driven from C: what suo_slam_amd/ba_dist.py: optimize_distributed does at world = 1 (units enqueued blindly, g2o's accept / reject
// arithmetic in the control block, the host looks at 16 doubles once per <= 12 units) without Python between the launches.
int suo::optimize_phases_one_rank(suo_ba_problem* q) {
    static BaExchange x;
    std::lock_guard<std::mutex> lock(x.mu);
    suo_ba_ctx* c = nullptr;
    int rc = ba_ctx_create(q, &c, "suo_optimize");
    if (rc != SUO_OK) return rc;
    BaCtxGuard guard{{c}};
    const int O = q->n_obj, ns = c->ns;
    const size_t n_lin = 2 + 27 * (size_t)O, n_sch = (size_t)ns * ns + ns + 1;
    const size_t need = 2 * n_lin + n_sch + 4 + 1 + 16;
    rc = x.ensure(need, c->device);
    if (rc != SUO_OK) return rc;
    hipStream_t s = c->arena.stream;
    SUO_HIP_CHECK(hipMemsetAsync(x.d_buf, 0, need * sizeof(double), s));
    double* lin_loc = x.d_buf; double* lin = lin_loc + n_lin; double* sch = lin + n_lin; double* red = sch + n_sch; double* good = red + 4; double* ctl = good + 1;
    auto classify = [&](int keep_all, int* n_good) -> int {
        int r = launch_ba_classify(c->dev_problem(), keep_all, good, c->scratch(), s);
        if (r != SUO_OK) return r;
        r = x.look(good, 1, s);
        *n_good = (int)(x.h_pin[0] + 0.5);
        return r;
    };
    int stats[4];
    rc = lm_rounds(q, ba_units_per_look(1), x.h_pin, stats, classify,
                   [&](int its) { return launch_ba_ctl_begin(ctl, its, 1, s); },
                   [&](int robust_on) { return ba_unit_one_rank(c, robust_on, ctl, lin_loc, lin, sch, red, s); },
                   [&]() { return x.look(ctl, 16, s); });
    if (rc) return rc;
    rc = suo_ba_ctx_download(c, q);
    memcpy(q->stats, stats, sizeof(stats));
    return rc;
}

// ---- the partitioned adjustment driven from C: suo_slam_amd/ba_dist.py: optimize_distributed without Python between the launches -------------------------------
// Rank `rank`'s share of the graph (ba_dist.py: split_problem): cameras c with c % world == rank in ascending order -- a camera's local index is its position in
// that list --, all objects, the edges of those cameras in the caller's order.  Host only.
static void ba_split(const suo_ba_problem& f, int rank, int world, std::vector<int>& cams, std::vector<int>& edges) {
    cams.clear(); edges.clear();
    for (int c = rank; c < f.n_cam; c += world) cams.push_back(c);
    for (int e = 0; e < f.n_edge; ++e)
        if (f.edge_cam[e] % world == rank) edges.push_back(e);
}
static int ba_split_check(const suo_ba_problem* f, int rank, int world, const char* who) {
    if (!f || world < 1 || rank < 0 || rank >= world || f->n_cam < 0 || f->n_obj < 0 || f->n_edge < 0) { suo_set_error("%s: bad problem, or rank %d of %d", who, rank, world); return SUO_ERR_ARG; }
    for (int e = 0; e < f->n_edge; ++e)
        if (f->edge_cam[e] < 0 || f->edge_cam[e] >= f->n_cam) { suo_set_error("%s: edge %d references a missing camera", who, e); return SUO_ERR_ARG; }
    return SUO_OK;
}
int suo_ba_split(const suo_ba_problem* full, int rank, int world, int* cams_out, int* n_cams, int* edges_out, int* n_edges) {
    if (!cams_out || !n_cams || !edges_out || !n_edges) { suo_set_error("suo_ba_split: null argument"); return SUO_ERR_ARG; }
    int rc = ba_split_check(full, rank, world, "suo_ba_split");
    if (rc != SUO_OK) return rc;
    std::vector<int> cams, edges;
    ba_split(*full, rank, world, cams, edges);
    std::copy(cams.begin(), cams.end(), cams_out);
    std::copy(edges.begin(), edges.end(), edges_out);
    *n_cams = (int)cams.size(); *n_edges = (int)edges.size();
    return SUO_OK;
}

// One rank of the partition in this process: its share as a problem of its own, its context, its exchange buffers (one slot of the driver's device block).
struct BaRank {
    int rank = 0;
    std::vector<int> cams, edges;
    std::vector<double> cam_T, obj_T, camk, p, uv, omega, chi2;
    std::vector<uint8_t> cam_fixed, inlier;
    std::vector<int32_t> ecam, eobj;
    suo_ba_problem q;
    suo_ba_ctx* c = nullptr;
    double *lin_loc = nullptr, *lin = nullptr, *sch = nullptr, *red = nullptr, *good = nullptr, *ctl = nullptr;
    void fill(const suo_ba_problem& f, int rank_, int world) {
        rank = rank_;
        ba_split(f, rank, world, cams, edges);
        const size_t C = cams.size(), E = edges.size();
        std::vector<int> local(f.n_cam, -1);
        cam_T.resize(12 * C); cam_fixed.resize(C);
        for (size_t i = 0; i < C; ++i) { local[cams[i]] = (int)i; memcpy(&cam_T[12 * i], f.cam_T + 12 * (size_t)cams[i], 12 * sizeof(double)); cam_fixed[i] = f.cam_fixed[cams[i]]; }
        obj_T.assign(f.obj_T, f.obj_T + 12 * (size_t)f.n_obj);
        ecam.resize(E); eobj.resize(E); camk.resize(4 * E); p.resize(3 * E); uv.resize(2 * E); omega.resize(3 * E); inlier.resize(E); chi2.assign(std::max<size_t>(E, 1), 0.0);
        for (size_t k = 0; k < E; ++k) {
            const size_t e = edges[k];
            ecam[k] = local[f.edge_cam[e]]; eobj[k] = f.edge_obj[e]; inlier[k] = f.edge_inlier[e];
            memcpy(&camk[4 * k], f.edge_camk + 4 * e, 4 * sizeof(double)); memcpy(&p[3 * k], f.edge_p + 3 * e, 3 * sizeof(double));
            memcpy(&uv[2 * k], f.edge_uv + 2 * e, 2 * sizeof(double)); memcpy(&omega[3 * k], f.edge_info + 3 * e, 3 * sizeof(double));
        }
        q = f;
        q.n_cam = (int)C; q.n_edge = (int)E;
        q.cam_T = cam_T.data(); q.cam_fixed = cam_fixed.data(); q.obj_T = obj_T.data();
        q.edge_cam = ecam.data(); q.edge_obj = eobj.data(); q.edge_camk = camk.data(); q.edge_p = p.data(); q.edge_uv = uv.data(); q.edge_info = omega.data();
        q.edge_inlier = inlier.data(); q.edge_chi2 = chi2.data();
    }
};

// Every rank passes the same full problem; the ranks of THIS process (one with RCCL, all `world` with the local backend) run the unit HipPhases.unit enqueues
// when collectives are in play -- the unfolded phases, each followed by its all-reduce -- phase by phase on ONE stream, eagerly.  Every rank looks at its own
// control block; the copies are equal because every decision is taken on all-reduced values (with the local backend the driver reads rank 0's).
static int optimize_dist(suo_ba_problem* full, suo_ba_comm* comm) {
    static BaExchange x;
    std::lock_guard<std::mutex> lock(x.mu);
    const int world = comm->world, n_here = comm->local ? world : 1;
    int rc = ba_split_check(full, comm->rank, world, "suo_optimize_dist");
    if (rc != SUO_OK) return rc;
    if (full->n_rounds < 0 || full->n_rounds > 8) { suo_set_error("suo_optimize_dist: bad sizes"); return SUO_ERR_ARG; }
    std::vector<BaRank> ranks(n_here);
    BaCtxGuard guard;
    for (int i = 0; i < n_here; ++i) {
        ranks[i].fill(*full, comm->local ? i : comm->rank, world);
        rc = ba_ctx_create(&ranks[i].q, &ranks[i].c, "suo_optimize_dist");
        if (rc != SUO_OK) return rc;
        guard.c.push_back(ranks[i].c);
    }
    suo_ba_ctx* c0 = ranks[0].c;
    if (comm->nccl && comm->device != c0->device) { suo_set_error("suo_optimize_dist: the communicator was created on device %d, the current device is %d", comm->device, c0->device); return SUO_ERR_ARG; }
    hipStream_t s = guard.s = c0->arena.stream;
    const int O = full->n_obj, ns = c0->ns;
    auto even = [](size_t n) { return (n + 1) & ~(size_t)1; };                  // every exchange buffer on a 16-byte boundary
    const size_t n_lin = 1 + 27 * (size_t)O + world, n_sch = (size_t)ns * ns + ns + 1, n_asm = 12 * (size_t)full->n_cam + 2 * (size_t)full->n_edge;
    const size_t stride = 2 * even(n_lin) + even(n_sch) + 4 + 2 + 16, asm_stride = even(std::max<size_t>(n_asm, 1));
    const size_t need = n_here * (stride + asm_stride);
    rc = x.ensure(need, c0->device);
    if (rc != SUO_OK) return rc;
    double* d_buf = x.d_buf;
    SUO_HIP_CHECK(hipMemsetAsync(d_buf, 0, n_here * stride * sizeof(double), s));
    for (int i = 0; i < n_here; ++i) {
        BaRank& k = ranks[i];
        k.lin_loc = d_buf + i * stride; k.lin = k.lin_loc + even(n_lin); k.sch = k.lin + even(n_lin); k.red = k.sch + even(n_sch); k.good = k.red + 4; k.ctl = k.good + 2;
    }
    double* d_asm = d_buf + n_here * stride;
    BaRank& k0 = ranks[0];
    auto reduce = [&](double* buf0, size_t st, size_t n) { return ba_comm_allreduce(comm, buf0, st, n, s); };
#define EACH_RANK(call) for (BaRank& k : ranks) { int r_ = (call); if (r_ != SUO_OK) return r_; }
    auto classify = [&](int keep_all, int* n_good) -> int {
        EACH_RANK(launch_ba_classify(k.c->dev_problem(), keep_all, k.good, k.c->scratch(), s));
        int r = reduce(k0.good, stride, 1); if (r) return r;
        r = x.look(k0.good, 1, s);
        *n_good = (int)(x.h_pin[0] + 0.5);
        return r;
    };
    int stats[4];
    rc = lm_rounds(full, ba_units_per_look(world), x.h_pin, stats, classify,
                   [&](int its) -> int { EACH_RANK(launch_ba_ctl_begin(k.ctl, its, world, s)); return SUO_OK; },
                   [&](int robust_on) -> int {
                       // (the reduce is in place and runs every unit: it starts from the rank's own totals in lin_loc, which the tail kernel copies over, live unit or not)
                       EACH_RANK(launch_ba_linearize(k.c->dev_problem(), robust_on, k.lin_loc, k.c->scratch(), k.rank, world, s, k.ctl, k.lin, (int)n_lin));
                       int r = reduce(k0.lin, stride, n_lin); if (r) return r;
                       EACH_RANK(launch_ba_ctl_lin(k.c->dev_problem(), k.ctl, k.lin, k.c->scratch(), s));
                       EACH_RANK(launch_ba_schur(k.c->dev_problem(), 0.0, ns, k.sch, k.c->scratch(), s, k.ctl));
                       r = reduce(k0.sch, stride, n_sch); if (r) return r;                     // the pose-graph reduce: [S | r | ok-count]
                       EACH_RANK(launch_ba_solve_update(k.c->dev_problem(), 0.0, ns, robust_on, k.lin + 1, k.sch, world, k.red, k.c->scratch(), k.c->d_big, s, k.ctl));
                       r = reduce(k0.red, stride, 3); if (r) return r;
                       EACH_RANK(launch_ba_ctl_decide(k.c->dev_problem(), k.ctl, k.red, s));
                       return SUO_OK;
                   },
                   [&]() { return x.look(k0.ctl, 16, s); });
    if (rc) return rc;
    // assemble the full result on every rank: each camera and edge is owned by exactly one rank, zeros elsewhere, one SUM
    SUO_HIP_CHECK(hipStreamSynchronize(s));
    std::vector<double> packed(n_here * asm_stride, 0.0);
    const size_t C12 = 12 * (size_t)full->n_cam, E = full->n_edge;
    for (int i = 0; i < n_here; ++i) {
        BaRank& k = ranks[i];
        rc = suo_ba_ctx_download(k.c, &k.q);
        if (rc != SUO_OK) return rc;
        double* out = packed.data() + i * asm_stride;
        for (size_t j = 0; j < k.cams.size(); ++j) memcpy(out + 12 * (size_t)k.cams[j], &k.cam_T[12 * j], 12 * sizeof(double));
        for (size_t j = 0; j < k.edges.size(); ++j) { out[C12 + k.edges[j]] = k.inlier[j]; out[C12 + E + k.edges[j]] = k.chi2[j]; }
    }
    if (n_asm) {
        SUO_HIP_CHECK(hipMemcpyAsync(d_asm, packed.data(), packed.size() * sizeof(double), hipMemcpyHostToDevice, s));
        rc = reduce(d_asm, asm_stride, n_asm); if (rc) return rc;
        SUO_HIP_CHECK(hipMemcpyAsync(packed.data(), d_asm, n_asm * sizeof(double), hipMemcpyDeviceToHost, s));
        SUO_HIP_CHECK(hipStreamSynchronize(s));
    }
#undef EACH_RANK
    memcpy(full->cam_T, packed.data(), C12 * sizeof(double));
    memcpy(full->obj_T, k0.obj_T.data(), 12 * (size_t)O * sizeof(double));
    for (size_t e = 0; e < E; ++e) {
        full->edge_inlier[e] = (uint8_t)(packed[C12 + e] + 0.5);
        if (full->edge_chi2) full->edge_chi2[e] = packed[C12 + E + e];
    }
    memcpy(full->stats, stats, sizeof(stats));
    return SUO_OK;
}

int suo_optimize_dist(suo_ba_problem* full, suo_ba_comm* comm) {
    if (!full || !comm) { suo_set_error("suo_optimize_dist: null %s", full ? "communicator" : "problem"); return SUO_ERR_ARG; }
    return optimize_dist(full, comm);
}

int suo_optimize_partitioned(suo_ba_problem* problem, int n_parts) {
    suo_ba_comm* comm = nullptr;
    int rc = suo_ba_comm_create_local(n_parts, &comm);
    if (rc != SUO_OK) return rc;
    rc = suo_optimize_dist(problem, comm);
    suo_ba_comm_destroy(comm);
    return rc;
}
