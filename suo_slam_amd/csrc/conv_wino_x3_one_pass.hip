// The LDS-DMA form's fused tail with the next block's conv1 in ONE pass over the tile (wino3x3_x3_one_pass_kernel: the kernel's comment in
// csrc/conv_wino_x3_kernel.h), in an object of its own beside csrc/conv_wino_x3_dma.hip, whose tails run two passes of 64 pixels.  SUO_WINO_TAIL_ONE_PASS selects
// between the two when a launch is issued (csrc/conv_wino_x3.hip checks the arguments and calls this).  The plain tail has no such form: built and measured, it
// did not gain (profiles/REJECTED.md); nor has the tail with the up-sampled addend, whose skip-row slots (SKD, 16 KB) do not fit beside a 66 KB operand.
#include "conv_wino_x3_kernel.h"

namespace suo {

int launch_conv3x3_wino_f16x2_fused_next_one_pass(const ConvArgs& a, hipStream_t s, int tiles) {
    hipLaunchKernelGGL((wino3x3_x3_one_pass_kernel<true, false, true, 4, 2, true, false, false, true>), dim3(tiles), dim3(256), 0, s, a);
    SUO_HIP_CHECK(hipGetLastError());
    return SUO_OK;
}

}  // namespace suo
