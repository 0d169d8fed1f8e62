// The visibility rule of bop_toolkit's visibility.py:9-42, mode 'bop19', for one pixel: shared by csrc/eval_vsd.hip (row N6) and csrc/gt_info.hip (row N7).
#pragma once
#include "suo_internal.h"

namespace suo {

// d_model, d_test: fp64 distances of the rendered model and of the test image; the difference is taken in float32 on the distances rounded to float32 and
// compared with float32(delta).  A pixel without a measurement (d_test == 0) counts as visible.  NaN in either distance gives false unless d_test == 0.
__device__ __forceinline__ bool visib_bop19(double d_model, double d_test, float delta) {
    return (((float)d_model - (float)d_test) <= delta || d_test == 0.0) && d_model > 0.0;
}

}  // namespace suo
