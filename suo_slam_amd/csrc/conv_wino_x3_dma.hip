// The four-wave fp16 Winograd kernels of csrc/conv_wino_x3.hip with their halo staged by LDS-DMA (wino3x3_x3_kernel<..., DMA = true>: the kernel's comment there)
// and their launchers: the same source compiled a second time for these five instantiations alone, so that the two staging paths build side by side and
// SUO_WINO_HALO_DMA selects between them when a launch is issued.
#define SUO_WX3_DMA_TU 1
#include "conv_wino_x3.hip"
