// The [-1, 1] -> [0, 1] mapping of the evaluation kernels (metrics.hip,
// ensemble.hip); the torch form is torch_impl.image_map01.
#pragma once
#include "common.h"

// [-1, 1] -> [0, 1].  quantize: through the 8-bit value a PNG writer stores,
// (uint8) trunc((clamp(x) + 1.0f) * 127.5f) with the fp32 add and multiply
// rounded separately (no FMA), then / 255.
__device__ __forceinline__ double metric_map01(float x, int quantize) {
  float c = fminf(fmaxf(x, -1.0f), 1.0f);
  if (quantize) {
    float s = __fmul_rn(__fadd_rn(c, 1.0f), 127.5f);
    return (double)(int)s / 255.0;
  }
  return ((double)c + 1.0) * 0.5;
}
