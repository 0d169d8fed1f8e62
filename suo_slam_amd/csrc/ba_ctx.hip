// The phase-wise bundle adjustment context (include/suo_hip.h: suo_ba_ctx): one problem resident on the device, the phases of an LM trial as separate entries
// -- host-synchronous (suo_ba_*), on caller-owned device buffers and streams (suo_ba_*_dev), under the device-resident schedule (suo_ba_lm_*_dev) -- and the
// debug entries that look into it.  Drivers: csrc/ba_drive.hip, suo_slam_amd/ba_dist.py.
#include <string.h>

#include <vector>

#include "ba_stage.h"
#include "tune.h"

using namespace suo;

// A context's buffers outlive it: a global adjustment of a SLAM run is create -> optimise -> destroy every few views, and creating / freeing its device arena, pinned
// staging, stream and exchange buffers cost 1.6-2 ms of a 10 ms adjustment (hipFree and hipHostFree synchronise the device).  suo_ba_ctx_destroy parks them here (at most
// four sets), suo_ba_ctx_create takes the first set OF ITS DEVICE back and grows what is too small.  Nothing read from them relies on their previous contents.
// The phase entries (suo_ba_*_dev) run on the CALLER's stream: a context that has used one is parked only after the whole device has drained (hipFree / hipHostFree
// used to imply that), so the next context never restages buffers a queued kernel still reads.
struct BaCtxBuffers {
    int device = -1;
    char* dev = nullptr; char* host = nullptr; size_t cap = 0; hipStream_t stream = nullptr;
    double* d_io = nullptr; double* h_io = nullptr; size_t io_cap = 0;      // io_cap: doubles of h_io; d_io holds io_cap + ba_scratch_doubles()
    double* d_big = nullptr; size_t big_cap = 0;
};
static std::mutex g_ba_pool_mu;
static std::vector<BaCtxBuffers> g_ba_pool;
static void ba_buffers_free(BaCtxBuffers& b) {
    if (b.d_io) (void)hipFree(b.d_io);
    if (b.d_big) (void)hipFree(b.d_big);
    if (b.h_io) (void)hipHostFree(b.h_io);
    if (b.dev) (void)hipFree(b.dev);
    if (b.host) (void)hipHostFree(b.host);
    if (b.stream) (void)hipStreamDestroy(b.stream);
    b = BaCtxBuffers();
}

int suo::ba_ctx_create(suo_ba_problem* p, suo_ba_ctx** out, const char* who) {
    if (!p || !out) { suo_set_error("%s: null argument", who); return SUO_ERR_ARG; }
    suo_ba_ctx* c = new suo_ba_ctx();
    BaCtxBuffers b;
    if (hipGetDevice(&c->device) != hipSuccess) { delete c; suo_set_error("%s: no current device", who); return SUO_ERR_HIP; }
    {
        std::lock_guard<std::mutex> lock(g_ba_pool_mu);
        for (size_t i = g_ba_pool.size(); i-- > 0;)
            if (g_ba_pool[i].device == c->device) { b = g_ba_pool[i]; g_ba_pool.erase(g_ba_pool.begin() + i); break; }
    }
    c->arena.dev = b.dev; c->arena.host = b.host; c->arena.cap = b.cap; c->arena.stream = b.stream;      // (Arena::ensure keeps what is large enough)
    c->d_io = b.d_io; c->h_io = b.h_io; c->io_cap = b.io_cap; c->d_big = b.d_big; c->big_cap = b.big_cap;
    int rc = stage_problems(p, 1, c->arena, c->st, who);
    if (rc != SUO_OK) { suo_ba_ctx_destroy(c); return rc; }
    c->n_cam = p->n_cam; c->n_obj = p->n_obj;
    int nfo = 0;
    for (int o = 0; o < p->n_obj; ++o) nfo += p->obj_fixed[o] ? 0 : 1;
    c->ns = 6 * nfo;
    const size_t big_need = nfo > 16 ? (size_t)c->ns * c->ns + c->ns : 0;
    if (big_need > c->big_cap) {
        if (c->d_big) (void)hipFree(c->d_big);
        c->d_big = nullptr; c->big_cap = 0;
        if (hipMalloc((void**)&c->d_big, big_need * sizeof(double)) != hipSuccess) { suo_set_error("%s: allocation failed", who); suo_ba_ctx_destroy(c); return SUO_ERR_HIP; }
        c->big_cap = big_need;
    }
    c->io_doubles = 2 * ((size_t)c->ns * c->ns + c->ns + 27 * (size_t)p->n_obj + 16);
    if (c->io_doubles > c->io_cap) {
        if (c->d_io) (void)hipFree(c->d_io);
        if (c->h_io) (void)hipHostFree(c->h_io);
        c->d_io = nullptr; c->h_io = nullptr; c->io_cap = 0;
        if (hipMalloc((void**)&c->d_io, (c->io_doubles + ba_scratch_doubles()) * sizeof(double)) != hipSuccess ||
            hipHostMalloc((void**)&c->h_io, c->io_doubles * sizeof(double), hipHostMallocDefault) != hipSuccess) {
            suo_set_error("%s: allocation failed", who); suo_ba_ctx_destroy(c); return SUO_ERR_HIP;
        }
        c->io_cap = c->io_doubles;
    }
    rc = launch_ba_init(c->dev_problem(), c->arena.stream);
    if (rc != SUO_OK) { suo_ba_ctx_destroy(c); return rc; }
    SUO_HIP_CHECK(hipStreamSynchronize(c->arena.stream));
    *out = c;
    return SUO_OK;
}

int suo::ba_unit_one_rank(suo_ba_ctx* c, int robust_on, double* ctl, double* lin_local, double* lin, double* sch, double* red, hipStream_t s) {
    int rc = launch_ba_linearize(c->dev_problem(), robust_on, lin_local, c->scratch(), 0, 1, s, ctl, lin, 1 + 27 * c->n_obj + 1, ctl);
    if (rc != SUO_OK) return rc;
    rc = launch_ba_schur(c->dev_problem(), 0.0, c->ns, sch, c->scratch(), s, ctl);
    if (rc != SUO_OK) return rc;
    return launch_ba_solve_update(c->dev_problem(), 0.0, c->ns, robust_on, lin + 1, sch, 1, red, c->scratch(), c->d_big, s, ctl, ctl);
}

extern "C" {

int suo_ba_ctx_create(suo_ba_problem* p, suo_ba_ctx** out) { return ba_ctx_create(p, out, "suo_ba_ctx_create"); }

void suo_ba_ctx_destroy(suo_ba_ctx* c) {
    if (!c) return;
    int cur = -1;
    const bool switched = hipGetDevice(&cur) == hipSuccess && cur != c->device && hipSetDevice(c->device) == hipSuccess;
    if (c->on_caller_stream) (void)hipDeviceSynchronize();          // work may still be queued on a stream that is not ours
    else if (c->arena.stream) (void)hipStreamSynchronize(c->arena.stream);
    BaCtxBuffers b;
    b.device = c->device;
    b.dev = c->arena.dev; b.host = c->arena.host; b.cap = c->arena.cap; b.stream = c->arena.stream;
    b.d_io = c->d_io; b.h_io = c->h_io; b.io_cap = c->io_cap; b.d_big = c->d_big; b.big_cap = c->big_cap;
    c->arena.dev = nullptr; c->arena.host = nullptr; c->arena.stream = nullptr;
    delete c;
    static const size_t keep = (int)SUO_TUNE("SUO_BA_CTX_POOL", 4);      // 0: free at once
    bool parked = false;
    {
        std::lock_guard<std::mutex> lock(g_ba_pool_mu);
        if (g_ba_pool.size() < keep) { g_ba_pool.push_back(b); parked = true; }
    }
    if (!parked) ba_buffers_free(b);
    if (switched) (void)hipSetDevice(cur);
}

int suo_ba_ctx_ns(const suo_ba_ctx* c) { return c ? c->ns : -1; }

static int ba_fetch(suo_ba_ctx* c, double* out, size_t n) {
    SUO_HIP_CHECK(hipMemcpyAsync(c->h_io, c->d_io, n * sizeof(double), hipMemcpyDeviceToHost, c->arena.stream));
    SUO_HIP_CHECK(hipStreamSynchronize(c->arena.stream));
    memcpy(out, c->h_io, n * sizeof(double));
    return SUO_OK;
}

int suo_ba_classify(suo_ba_ctx* c, int keep_all, double* num_good_local) {
    int rc = launch_ba_classify(c->dev_problem(), keep_all, c->d_io, c->scratch(), c->arena.stream);
    return rc != SUO_OK ? rc : ba_fetch(c, num_good_local, 1);
}

int suo_ba_linearize(suo_ba_ctx* c, int robust_on, double* out) {
    int rc = launch_ba_linearize(c->dev_problem(), robust_on, c->d_io, c->scratch(), 0, 1, c->arena.stream);
    return rc != SUO_OK ? rc : ba_fetch(c, out, 2 + 27 * (size_t)c->n_obj);
}

int suo_ba_schur(suo_ba_ctx* c, double lambda, double* out) {
    int rc = launch_ba_schur(c->dev_problem(), lambda, c->ns, c->d_io, c->scratch(), c->arena.stream);
    return rc != SUO_OK ? rc : ba_fetch(c, out, (size_t)c->ns * c->ns + c->ns + 1);
}

int suo_ba_solve_update(suo_ba_ctx* c, double lambda, int robust_on, const double* in, double* out) {
    const size_t n_in = 27 * (size_t)c->n_obj + (size_t)c->ns * c->ns + c->ns;
    double* h_in = c->h_io + c->io_doubles / 2;
    double* d_in = c->d_io + c->io_doubles / 2;
    memcpy(h_in, in, n_in * sizeof(double));
    SUO_HIP_CHECK(hipMemcpyAsync(d_in, h_in, n_in * sizeof(double), hipMemcpyHostToDevice, c->arena.stream));
    int rc = launch_ba_solve_update(c->dev_problem(), lambda, c->ns, robust_on, d_in, d_in + 27 * (size_t)c->n_obj, 0, c->d_io, c->scratch(),
                                    c->d_big, c->arena.stream);
    if (rc != SUO_OK) return rc;
    double dev_order[4];                       // device layout [chi2 | scale_cams | ok | scale_objs] -> documented host layout
    rc = ba_fetch(c, dev_order, 4);
    out[0] = dev_order[0]; out[1] = dev_order[1]; out[2] = dev_order[3]; out[3] = dev_order[2];
    return rc;
}

int suo_ba_restore(suo_ba_ctx* c) {
    int rc = launch_ba_restore(c->dev_problem(), c->arena.stream);
    if (rc != SUO_OK) return rc;
    SUO_HIP_CHECK(hipStreamSynchronize(c->arena.stream));
    return SUO_OK;
}

// ---- the same phases on caller-owned DEVICE buffers, stream-ordered, no host synchronisation: the buffers are what RCCL
// all-reduces in place between the phases (suo_slam_amd/ba_dist.py) ------------------------------------------------
int suo_ba_classify_dev(suo_ba_ctx* c, int keep_all, double* num_good_dev, void* stream) {
    return launch_ba_classify(c->dev_problem(), keep_all, num_good_dev, c->scratch(), c->on(stream));
}
int suo_ba_linearize_dev(suo_ba_ctx* c, int robust_on, int rank, int world, double* lin_dev, void* stream) {
    if (rank < 0 || rank >= world) { suo_set_error("suo_ba_linearize_dev: rank %d of %d", rank, world); return SUO_ERR_ARG; }
    return launch_ba_linearize(c->dev_problem(), robust_on, lin_dev, c->scratch(), rank, world, c->on(stream));
}
int suo_ba_schur_dev(suo_ba_ctx* c, double lambda, double* sch_dev, void* stream) {
    return launch_ba_schur(c->dev_problem(), lambda, c->ns, sch_dev, c->scratch(), c->on(stream));
}
int suo_ba_solve_update_dev(suo_ba_ctx* c, double lambda, int robust_on, int world, const double* lin_dev, const double* sch_dev, double* red_dev,
                            void* stream) {
    return launch_ba_solve_update(c->dev_problem(), lambda, c->ns, robust_on, lin_dev + 1, sch_dev, world, red_dev, c->scratch(), c->d_big,
                                  c->on(stream));
}
int suo_ba_restore_dev(suo_ba_ctx* c, void* stream) { return launch_ba_restore(c->dev_problem(), c->on(stream)); }

// ---- the same phases under the device-resident LM schedule (csrc/lm_dist.hip: ctl) ------------------------------------------------------
int suo_ba_lm_begin_dev(suo_ba_ctx* c, double* ctl_dev, int its, int world, void* stream) {
    if (!c || !ctl_dev || world < 1) { suo_set_error("suo_ba_lm_begin_dev: bad arguments"); return SUO_ERR_ARG; }
    return launch_ba_ctl_begin(ctl_dev, its, world, c->on(stream));
}
int suo_ba_lm_linearize_dev(suo_ba_ctx* c, int robust_on, int rank, int world, const double* ctl_dev, double* lin_local_dev, double* lin_dev, void* stream) {
    if (!c || !ctl_dev || !lin_local_dev || !lin_dev || rank < 0 || rank >= world) { suo_set_error("suo_ba_lm_linearize_dev: bad arguments"); return SUO_ERR_ARG; }
    // the reduce works in place and runs every unit: it starts from this rank's own totals every time (a trial on a standing linearisation
    // re-reduces the same numbers instead of reducing the already reduced ones) -- the tail kernel copies them over, live unit or not
    return launch_ba_linearize(c->dev_problem(), robust_on, lin_local_dev, c->scratch(), rank, world, c->on(stream), ctl_dev, lin_dev, 1 + 27 * c->n_obj + world);
}
int suo_ba_lm_schur_dev(suo_ba_ctx* c, double* ctl_dev, const double* lin_dev, double* sch_dev, void* stream) {
    if (!c || !ctl_dev || !lin_dev || !sch_dev) { suo_set_error("suo_ba_lm_schur_dev: null argument"); return SUO_ERR_ARG; }
    int rc = launch_ba_ctl_lin(c->dev_problem(), ctl_dev, lin_dev, c->scratch(), c->on(stream));
    if (rc != SUO_OK) return rc;
    return launch_ba_schur(c->dev_problem(), 0.0, c->ns, sch_dev, c->scratch(), c->on(stream), ctl_dev);
}
int suo_ba_lm_solve_update_dev(suo_ba_ctx* c, int robust_on, int world, const double* ctl_dev, const double* lin_dev, const double* sch_dev, double* red_dev,
                               void* stream) {
    if (!c || !ctl_dev || !lin_dev || !sch_dev || !red_dev) { suo_set_error("suo_ba_lm_solve_update_dev: null argument"); return SUO_ERR_ARG; }
    return launch_ba_solve_update(c->dev_problem(), 0.0, c->ns, robust_on, lin_dev + 1, sch_dev, world, red_dev, c->scratch(), c->d_big, c->on(stream),
                                  ctl_dev);
}
// One unit on ONE rank (ba_unit_one_rank): 12 launches instead of 14.  Same arithmetic in the same order as the four calls above with nothing in between:
// bit-identical (tests/test_gpu_geometry.py).
int suo_ba_lm_unit_one_rank_dev(suo_ba_ctx* c, int robust_on, double* ctl_dev, double* lin_local_dev, double* lin_dev, double* sch_dev, double* red_dev, void* stream) {
    if (!c || !ctl_dev || !lin_local_dev || !lin_dev || !sch_dev || !red_dev) { suo_set_error("suo_ba_lm_unit_one_rank_dev: null argument"); return SUO_ERR_ARG; }
    return ba_unit_one_rank(c, robust_on, ctl_dev, lin_local_dev, lin_dev, sch_dev, red_dev, c->on(stream));
}
int suo_ba_lm_decide_dev(suo_ba_ctx* c, double* ctl_dev, const double* red_dev, void* stream) {
    if (!c || !ctl_dev || !red_dev) { suo_set_error("suo_ba_lm_decide_dev: null argument"); return SUO_ERR_ARG; }
    return launch_ba_ctl_decide(c->dev_problem(), ctl_dev, red_dev, c->on(stream));
}

// Test entry: the workgroup Cholesky solve of the reduced system (csrc/lm_device.h: wg_cholesky_solve) on a dense symmetric ns x ns matrix (host, row-major; ns a multiple
// of 6, at most 96) -- x solves A x = b; *ok_out = 0 when a pivot was not positive (x is then meaningless).
int suo_debug_cholesky_solve(const double* A, const double* b, int ns, double* x_out, int* ok_out) {
    if (!A || !b || !x_out || !ok_out || ns <= 0) { suo_set_error("suo_debug_cholesky_solve: bad argument"); return SUO_ERR_ARG; }
    double* d = nullptr;
    const size_t n = (size_t)ns * ns + 2 * (size_t)ns + 1;
    SUO_HIP_CHECK(hipMalloc((void**)&d, n * sizeof(double)));
    struct Free { double* d; ~Free() { (void)hipFree(d); } } guard{d};
    SUO_HIP_CHECK(hipMemcpy(d, A, (size_t)ns * ns * sizeof(double), hipMemcpyHostToDevice));
    SUO_HIP_CHECK(hipMemcpy(d + (size_t)ns * ns, b, (size_t)ns * sizeof(double), hipMemcpyHostToDevice));
    int rc = launch_debug_cholesky(d, d + (size_t)ns * ns, ns, d + (size_t)ns * ns + ns, (int*)(d + (size_t)ns * ns + 2 * (size_t)ns), nullptr);
    if (rc != SUO_OK) return rc;
    SUO_HIP_CHECK(hipDeviceSynchronize());
    SUO_HIP_CHECK(hipMemcpy(x_out, d + (size_t)ns * ns + ns, (size_t)ns * sizeof(double), hipMemcpyDeviceToHost));
    SUO_HIP_CHECK(hipMemcpy(ok_out, d + (size_t)ns * ns + 2 * (size_t)ns, sizeof(int), hipMemcpyDeviceToHost));
    return SUO_OK;
}

// Test entry: the SE(3) update of every LM kernel (csrc/lm_device.h: pose_from_T, pose_oplus, pose_to_T), one thread per pose, on host arrays: T_out[i] =
// exp(u[i]) * T_in[i] (row-major 3x4; u = omega, upsilon) and, when q_out is given, the unit quaternion (w, x, y, z) the kernels keep after the update.
int suo_debug_pose_oplus(const double* T_in, const double* u, int n, double* T_out, double* q_out) {
    if (!T_in || !u || !T_out || n <= 0) { suo_set_error("suo_debug_pose_oplus: bad argument"); return SUO_ERR_ARG; }
    double* d = nullptr;
    const size_t nn = (size_t)n;
    SUO_HIP_CHECK(hipMalloc((void**)&d, nn * (12 + 6 + 12 + 4) * sizeof(double)));
    struct Free { double* d; ~Free() { (void)hipFree(d); } } guard{d};
    double *d_T = d, *d_u = d + 12 * nn, *d_out = d + 18 * nn, *d_q = d + 30 * nn;
    SUO_HIP_CHECK(hipMemcpy(d_T, T_in, 12 * nn * sizeof(double), hipMemcpyHostToDevice));
    SUO_HIP_CHECK(hipMemcpy(d_u, u, 6 * nn * sizeof(double), hipMemcpyHostToDevice));
    int rc = launch_debug_pose_oplus(d_T, d_u, n, d_out, d_q, nullptr);
    if (rc != SUO_OK) return rc;
    SUO_HIP_CHECK(hipDeviceSynchronize());
    SUO_HIP_CHECK(hipMemcpy(T_out, d_out, 12 * nn * sizeof(double), hipMemcpyDeviceToHost));
    if (q_out) SUO_HIP_CHECK(hipMemcpy(q_out, d_q, 4 * nn * sizeof(double), hipMemcpyDeviceToHost));
    return SUO_OK;
}

// Test entry: what the LM kernels linearise. After suo_ba_linearize (edge_pass_partial of csrc/lm_device.h, shared by every LM
// kernel) the context holds, per edge in the CALLER's edge order: jac[29] = [Jc 2x6 | Jo 2x6 | w*info (xx,xy,yy) | -w*info*err (2)]
// and err[2].  Inactive edges (outliers, fixed-fixed) keep whatever was there before: call it on all-inlier graphs.
int suo_debug_ba_jacobians(suo_ba_ctx* c, int n_edge, double* jac_out, double* err_out) {
    if (!c || !jac_out || !err_out) { suo_set_error("suo_debug_ba_jacobians: null argument"); return SUO_ERR_ARG; }
    const Prep& P = c->st.prep[0];
    if ((int)P.order.size() != n_edge) { suo_set_error("suo_debug_ba_jacobians: context has %d edges", (int)P.order.size()); return SUO_ERR_ARG; }
    std::vector<double> jac((size_t)29 * n_edge), err((size_t)2 * n_edge);
    SUO_HIP_CHECK(hipStreamSynchronize(c->arena.stream));
    SUO_HIP_CHECK(hipMemcpy(jac.data(), P.S.jac, jac.size() * sizeof(double), hipMemcpyDeviceToHost));
    SUO_HIP_CHECK(hipMemcpy(err.data(), P.S.err, err.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int k = 0; k < n_edge; ++k) {
        const int e = P.order[k];
        memcpy(jac_out + (size_t)29 * e, jac.data() + (size_t)29 * k, 29 * sizeof(double));
        err_out[2 * e] = err[2 * k]; err_out[2 * e + 1] = err[2 * k + 1];
    }
    return SUO_OK;
}

int suo_ba_ctx_download(suo_ba_ctx* c, suo_ba_problem* p) {
    int rc = launch_ba_finalize(c->dev_problem(), c->arena.stream);
    if (rc != SUO_OK) return rc;
    return fetch_results(p, 1, c->arena, c->st);
}

}  // extern "C"
