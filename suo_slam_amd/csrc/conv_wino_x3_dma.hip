// The four-wave fp16 Winograd kernels with their halo staged by LDS-DMA (wino3x3_x3_kernel<..., DMA = true>: the kernel's comment in
// csrc/conv_wino_x3_kernel.h) and their launchers, in an object of their own, so that the two staging paths build side by side and
// SUO_WINO_HALO_DMA selects between them when a launch is issued (csrc/conv_wino_x3.hip checks the arguments and calls these).
#include "conv_wino_x3_kernel.h"

namespace suo {

int launch_conv3x3_wino_f16x2_dma(const ConvArgs& a, hipStream_t s, int tiles) {
    if (a.N == 64) hipLaunchKernelGGL((wino3x3_x3_kernel<false, false, false, 2, 2, false, false, false, true>), dim3(tiles), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((wino3x3_x3_kernel<false, false, false, 4, 2, false, false, false, true>), dim3(tiles), dim3(256), 0, s, a);
    SUO_HIP_CHECK(hipGetLastError());
    return SUO_OK;
}
int launch_conv3x3_wino_f16x2_fused_dma(const ConvArgs& a, hipStream_t s, int tiles) {
    if (a.n_W1) hipLaunchKernelGGL((wino3x3_x3_kernel<true, false, true, 4, 2, true, false, false, true>), dim3(tiles), dim3(256), 0, s, a);
    else if (a.up) hipLaunchKernelGGL((wino3x3_x3_kernel<true, true, true, 4, 2, false, false, false, true>), dim3(tiles), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((wino3x3_x3_kernel<true, false, true, 4, 2, false, false, false, true>), dim3(tiles), dim3(256), 0, s, a);
    SUO_HIP_CHECK(hipGetLastError());
    return SUO_OK;
}

}  // namespace suo
