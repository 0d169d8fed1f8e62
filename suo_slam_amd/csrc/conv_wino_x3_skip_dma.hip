// The LDS-DMA form's fused tail with the up-sampled addend, its skip rows fetched by LDS-DMA one epilogue block ahead (wino3x3_x3_kernel<..., SKD = true, ..., DMA =
// true>: the kernel's comment in csrc/conv_wino_x3_kernel.h), in an object of its own beside csrc/conv_wino_x3_dma.hip, whose tails keep the register loads:
// SUO_WINO_SKIP_DMA selects between the two when a launch is issued (csrc/conv_wino_x3.hip checks the arguments and calls this).  The plain tail and the tail with
// the next block's conv1 have no such form: built and measured, they were no faster / slower (profiles/REJECTED.md).
#include "conv_wino_x3_kernel.h"

namespace suo {

int launch_conv3x3_wino_f16x2_fused_up_skip_dma(const ConvArgs& a, hipStream_t s, int tiles) {
    hipLaunchKernelGGL((wino3x3_x3_kernel<true, true, true, 4, 2, false, true, false, true>), dim3(tiles), dim3(256), 0, s, a);
    SUO_HIP_CHECK(hipGetLastError());
    return SUO_OK;
}

}  // namespace suo
