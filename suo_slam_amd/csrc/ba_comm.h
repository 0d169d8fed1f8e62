// The communicator of the partitioned bundle adjustment (include/suo_hip.h: suo_ba_comm): one operation, an in-place SUM all-reduce of doubles on a device
// buffer, ordered on a stream.  Two backends behind it (csrc/ba_comm.hip): RCCL, resolved with dlopen at first use, and `world` local ranks on one device.
#pragma once
#include "suo_internal.h"

constexpr int SUO_BA_MAX_LOCAL_RANKS = 16;

struct suo_ba_comm {
    int rank = 0, world = 1;
    int local = 0;                     // the local backend: the driver runs ranks 0 .. world-1 itself, their buffers `stride` doubles apart
    uint64_t calls = 0;
    void* nccl = nullptr;              // ncclComm_t
    int device = -1;                   // RCCL: the device the communicator was created on
};

namespace suo {
// buf: this rank's buffer (local backend: rank 0's).  Stream-ordered; no host synchronisation.
int ba_comm_allreduce(suo_ba_comm* c, double* buf, size_t stride, size_t n, hipStream_t s);
int launch_ba_local_allreduce(double* block, int world, size_t stride, size_t n, hipStream_t s);
}  // namespace suo
