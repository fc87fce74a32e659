// blas_quant.h — the quantisation rule of the device-built BLAS, shared by the builders (bvh_gpu.hip) and the refit
// (blas_refit.hip): a refit of unchanged vertices must reproduce the builder's planes bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace rt {

// dequantisation of one axis from the root box [lo, hi]: 65520 quanta over the extent, quanta 0..3 below every stored plane
__device__ __forceinline__ void blas_quant_axis_params(float lo, float hi, float* q_lo, float* q_scale) {
  const float ext = hi - lo;
  const float scale = ext > 0.f ? ext * 1.00001f / 65520.0f : 1e-30f;
  *q_lo = lo - 4.0f * scale;
  *q_scale = scale;
}

__device__ __forceinline__ uint32_t quant_box_axis(float lo, float hi, float base, float scale) {
  // two quanta of margin on each side cover the float rounding of the division
  float ql = floorf((lo - base) / scale) - 2.0f, qh = ceilf((hi - base) / scale) + 2.0f;
  ql = fminf(fmaxf(ql, 0.0f), 65535.0f); qh = fminf(fmaxf(qh, 0.0f), 65535.0f);
  return (uint32_t)ql | ((uint32_t)qh << 16);
}

}  // namespace rt
