// Calibration probe of the two-term fp16 form (csrc/f16x2.h): the largest magnitude of one site's operand -- max |relu(scale x + shift)| (a BatchNorm
// prologue), or max |x| without one -- over an NHWC tensor the range-safe probe forward has written (csrc/net.hip: Net::calibrate).
// Each workgroup reduces its part to one value, then ONE lane folds it into *out with a vector global atomic max on the float's bits: the values are
// non-negative, so their bits order as the floats do.  The reduction itself runs on those bits as well, so a nan (bits above +inf once the sign is cleared)
// wins the max and reaches the host, which rejects it with inf.
#include "suo_internal.h"

namespace suo {

__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ x, long rows, int C, int ld, const float* __restrict__ scale,
                                                     const float* __restrict__ shift, int relu, unsigned* out) {
    const int c4n = C >> 2;
    const long n4 = rows * c4n;
    unsigned m = 0u;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n4; e += (long)gridDim.x * 256) {
        const long row = e / c4n;
        const int c = (int)(e - row * c4n) * 4;
        const float4 v = *reinterpret_cast<const float4*>(x + row * ld + c);
        float t[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float y = t[j];
            if (scale) y = fmaf(y, scale[c + j], shift[c + j]);
            if (relu) y = fmaxf(y, 0.f);
            const unsigned b = __float_as_uint(y) & 0x7fffffffu;      // |y| (a nan stays above every finite value and +inf)
            m = b > m ? b : m;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned p = (unsigned)__shfl_xor((int)m, o, 64);
        m = p > m ? p : m;
    }
    __shared__ unsigned wm[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wm[w] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned r = wm[0];
        for (int i = 1; i < 4; ++i) r = wm[i] > r ? wm[i] : r;
        atomicMax(out, r);
    }
}

// out: one word in device memory, zeroed by the caller before the first reduction of a site (several tensors may feed one site: conv3 + its skip conv4)
int launch_absmax(const float* x, long rows, int C, int ld, const float* scale, const float* shift, int relu, unsigned* out, hipStream_t s) {
    if (!x || !out || rows <= 0 || C <= 0 || C % 4 || ld % 4 || ld < C || ((scale == nullptr) != (shift == nullptr))) {
        suo_set_error("absmax: bad arguments (rows=%ld C=%d ld=%d)", rows, C, ld);
        return SUO_ERR_ARG;
    }
    const long n4 = rows * (C / 4);
    const long blocks = (n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048;
    hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, rows, C, ld, scale, shift, relu, out);
    SUO_HIP_CHECK(hipGetLastError());
    return SUO_OK;
}

}  // namespace suo
