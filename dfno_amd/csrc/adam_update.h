// The fp32 Adam update of one element, shared by the multi-tensor kernels
// (adam.hip) and the fused spectral grad-W + Adam kernel (spectral.hip), so
// both apply the same expression in the same order.  c1/c2 are the bias
// corrections 1 - beta^step.
#pragma once

#include <hip/hip_runtime.h>

__device__ __forceinline__ void adam_update(float& p, float g, float& m,
                                            float& v, float lr, float b1,
                                            float b2, float eps, float wd,
                                            float c1, float c2) {
  float gg = g + wd * p;
  m = b1 * m + (1.f - b1) * gg;
  v = b2 * v + (1.f - b2) * gg * gg;
  p -= lr * (m / c1) / (sqrtf(v / c2) + eps);
}
