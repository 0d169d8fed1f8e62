// suo_ba_comm (include/suo_hip.h): the all-reduce of the partitioned bundle adjustment behind the C ABI.
//
//   RCCL    ncclAllReduce(ncclDouble, ncclSum) in place on the driver's stream.  The library is resolved with dlopen at first use, so libsuo_hip.so loads where no
//           RCCL is installed, and a process that already holds a copy (PyTorch's) runs its collectives through that copy and no second one.
//   local   `world` ranks inside one process, on one device and one stream: ba_local_allreduce_kernel sums the ranks' buffers, `stride` doubles apart in one
//           block, in ascending rank order and writes the sum back to every rank's buffer.  The largest message of the schedule is (6 n_obj)^2 + 6 n_obj + 1
//           doubles (74.5 KB at 16 objects), world <= 16: about a megabyte of L2-resident traffic at most, so the cost is the launch -- one launch, every thread
//           one 16-byte column of the block, all of a column's loads issued before the first add.
#include <dlfcn.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>

#include "../../include/suo_hip.h"
#include "ba_comm.h"

namespace suo {

// out[r][i] = ((b[0][i] + b[1][i]) + b[2][i]) + ... for every rank r: the order is part of the contract (numpy restates it bit for bit), so no tree and no atomics.
// vec: the block is 16-byte aligned and the stride even -- every rank's pair (2i, 2i + 1) is one 16-byte load / store; an odd n leaves one scalar element.
__global__ __launch_bounds__(256) void ba_local_allreduce_kernel(double* block, int world, size_t stride, size_t n, int vec) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, T = (size_t)gridDim.x * 256;
    if (vec) {
        const size_t n2 = n >> 1;
        for (size_t i = t; i < n2; i += T) {
            double2* col = (double2*)block + i;              // rank r's pair: col[r * stride / 2]
            const size_t s2 = stride >> 1;
            double2 v[SUO_BA_MAX_LOCAL_RANKS];
#pragma unroll
            for (int r = 0; r < SUO_BA_MAX_LOCAL_RANKS; ++r)
                if (r < world) v[r] = col[r * s2];
            double2 a = v[0];
#pragma unroll
            for (int r = 1; r < SUO_BA_MAX_LOCAL_RANKS; ++r)
                if (r < world) { a.x += v[r].x; a.y += v[r].y; }
#pragma unroll
            for (int r = 0; r < SUO_BA_MAX_LOCAL_RANKS; ++r)
                if (r < world) col[r * s2] = a;
        }
        if ((n & 1) && t == 0) {
            double* e = block + (n - 1);
            double a = e[0];
            for (int r = 1; r < world; ++r) a += e[r * stride];
            for (int r = 0; r < world; ++r) e[r * stride] = a;
        }
        return;
    }
    for (size_t i = t; i < n; i += T) {
        double* e = block + i;
        double a = e[0];
        for (int r = 1; r < world; ++r) a += e[r * stride];
        for (int r = 0; r < world; ++r) e[r * stride] = a;
    }
}

int launch_ba_local_allreduce(double* block, int world, size_t stride, size_t n, hipStream_t s) {
    if (!block || world < 1 || world > SUO_BA_MAX_LOCAL_RANKS || (world > 1 && stride < n)) {
        suo_set_error("local all-reduce: block %p, %d ranks (1..%d), stride %zu, n %zu", (void*)block, world, SUO_BA_MAX_LOCAL_RANKS, stride, n);
        return SUO_ERR_ARG;
    }
    if (n == 0) return SUO_OK;
    const int vec = ((uintptr_t)block % 16 == 0) && (stride % 2 == 0) && n >= 2;
    const size_t items = vec ? n / 2 : n;
    const size_t wgs = std::min<size_t>(256, (items + 255) / 256);            // one workgroup per CU at most, grid-strided beyond
    hipLaunchKernelGGL(ba_local_allreduce_kernel, dim3((unsigned)wgs), dim3(256), 0, s, block, world, stride, n, vec);
    SUO_HIP_CHECK(hipGetLastError());
    return SUO_OK;
}

// ---- RCCL through dlopen ------------------------------------------------------------------------------------------------------------------------------
// (the handful of declarations of rccl.h this file needs: the ABI NCCL has kept since 2.0)
struct RcclUniqueId { char internal[128]; };
typedef int (*fn_get_unique_id)(RcclUniqueId*);
typedef int (*fn_comm_init_rank)(void**, int, RcclUniqueId, int);
typedef int (*fn_all_reduce)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*fn_comm_destroy)(void*);
typedef const char* (*fn_error_string)(int);
constexpr int RCCL_DOUBLE = 8, RCCL_SUM = 0;

struct Rccl {
    void* handle = nullptr;
    fn_get_unique_id get_unique_id = nullptr;
    fn_comm_init_rank comm_init_rank = nullptr;
    fn_all_reduce all_reduce = nullptr;
    fn_comm_destroy comm_destroy = nullptr;
    fn_error_string error_string = nullptr;
};
static std::mutex g_rccl_mu;
static Rccl g_rccl;

// First a copy the process already holds (RTLD_NOLOAD matches the soname, whatever file it came from), then the caller's explicit path, then the loader path.
// A failure is not remembered: a later call may find the library (SUO_RCCL_LIB set meanwhile, another component having loaded it).
static int rccl_get(const Rccl** out) {
    std::lock_guard<std::mutex> lock(g_rccl_mu);
    if (!g_rccl.handle) {
        void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
        if (!h) {
            const char* path = getenv("SUO_RCCL_LIB");
            if (path && *path) {
                h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
                if (!h) { const char* e = dlerror(); suo_set_error("RCCL: SUO_RCCL_LIB=%s does not load: %s", path, e ? e : "?"); return SUO_ERR_MISSING; }
            } else {
                h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
                if (!h) { const char* e = dlerror(); suo_set_error("RCCL: no copy loaded in the process, SUO_RCCL_LIB not set, librccl.so.1: %s", e ? e : "?"); return SUO_ERR_MISSING; }
            }
        }
        Rccl r;
        r.handle = h;
        r.get_unique_id = (fn_get_unique_id)dlsym(h, "ncclGetUniqueId");
        r.comm_init_rank = (fn_comm_init_rank)dlsym(h, "ncclCommInitRank");
        r.all_reduce = (fn_all_reduce)dlsym(h, "ncclAllReduce");
        r.comm_destroy = (fn_comm_destroy)dlsym(h, "ncclCommDestroy");
        r.error_string = (fn_error_string)dlsym(h, "ncclGetErrorString");
        if (!r.get_unique_id || !r.comm_init_rank || !r.all_reduce || !r.comm_destroy || !r.error_string) {
            dlclose(h);
            suo_set_error("RCCL: the library lacks ncclGetUniqueId / ncclCommInitRank / ncclAllReduce / ncclCommDestroy / ncclGetErrorString");
            return SUO_ERR_MISSING;
        }
        g_rccl = r;
    }
    *out = &g_rccl;
    return SUO_OK;
}

#define SUO_RCCL_CHECK(R, expr)                                                                      \
    do {                                                                                             \
        int _e = (expr);                                                                             \
        if (_e != 0) { suo_set_error("%s -> %s", #expr, (R)->error_string(_e)); return SUO_ERR_HIP; } \
    } while (0)

int ba_comm_allreduce(suo_ba_comm* c, double* buf, size_t stride, size_t n, hipStream_t s) {
    if (!c || !buf) { suo_set_error("suo_ba_comm_allreduce: null argument"); return SUO_ERR_ARG; }
    ++c->calls;
    if (c->local) return launch_ba_local_allreduce(buf, c->world, stride, n, s);
    const Rccl* R = nullptr;
    int rc = rccl_get(&R);
    if (rc != SUO_OK) return rc;
    SUO_RCCL_CHECK(R, R->all_reduce(buf, buf, n, RCCL_DOUBLE, RCCL_SUM, c->nccl, s));
    return SUO_OK;
}

}  // namespace suo

using namespace suo;

extern "C" {

int suo_ba_comm_rccl_unique_id(void* id128) {
    if (!id128) { suo_set_error("suo_ba_comm_rccl_unique_id: null argument"); return SUO_ERR_ARG; }
    const Rccl* R = nullptr;
    int rc = rccl_get(&R);
    if (rc != SUO_OK) return rc;
    RcclUniqueId id;
    SUO_RCCL_CHECK(R, R->get_unique_id(&id));
    memcpy(id128, id.internal, sizeof(id.internal));
    return SUO_OK;
}

int suo_ba_comm_create_rccl(const void* id128, int rank, int world, suo_ba_comm** out) {
    if (!id128 || !out || world < 1 || rank < 0 || rank >= world) { suo_set_error("suo_ba_comm_create_rccl: rank %d of %d", rank, world); return SUO_ERR_ARG; }
    const Rccl* R = nullptr;
    int rc = rccl_get(&R);
    if (rc != SUO_OK) return rc;
    suo_ba_comm* c = new suo_ba_comm();
    c->rank = rank; c->world = world;
    if (hipGetDevice(&c->device) != hipSuccess) { delete c; suo_set_error("suo_ba_comm_create_rccl: no current device"); return SUO_ERR_HIP; }
    RcclUniqueId id;
    memcpy(id.internal, id128, sizeof(id.internal));
    int e = R->comm_init_rank(&c->nccl, world, id, rank);
    if (e != 0) { suo_set_error("ncclCommInitRank(rank %d of %d) -> %s", rank, world, R->error_string(e)); delete c; return SUO_ERR_HIP; }
    *out = c;
    return SUO_OK;
}

int suo_ba_comm_create_local(int world, suo_ba_comm** out) {
    if (!out || world < 1 || world > SUO_BA_MAX_LOCAL_RANKS) {
        suo_set_error("suo_ba_comm_create_local: %d ranks (1..%d)", world, SUO_BA_MAX_LOCAL_RANKS);
        return SUO_ERR_ARG;
    }
    suo_ba_comm* c = new suo_ba_comm();
    c->world = world; c->local = 1;
    *out = c;
    return SUO_OK;
}

void suo_ba_comm_destroy(suo_ba_comm* c) {
    if (!c) return;
    if (c->nccl) {
        const Rccl* R = nullptr;
        if (rccl_get(&R) == SUO_OK) (void)R->comm_destroy(c->nccl);
    }
    delete c;
}

int suo_ba_comm_rank(const suo_ba_comm* c) { return c ? c->rank : -1; }
int suo_ba_comm_world(const suo_ba_comm* c) { return c ? c->world : -1; }
uint64_t suo_ba_comm_calls(const suo_ba_comm* c) { return c ? c->calls : 0; }

int suo_ba_comm_allreduce(suo_ba_comm* c, double* buf_dev, size_t stride, size_t n, void* stream) {
    return ba_comm_allreduce(c, buf_dev, stride, n, (hipStream_t)stream);
}

int suo_debug_ba_local_allreduce(double* block_dev, int world, size_t stride, size_t n, void* stream) {
    int rc = launch_ba_local_allreduce(block_dev, world, stride, n, (hipStream_t)stream);
    if (rc != SUO_OK) return rc;
    if (!stream) SUO_HIP_CHECK(hipStreamSynchronize(nullptr));
    return SUO_OK;
}

}  // extern "C"
