// The [-1, 1] -> [0, 1] mapping of the evaluation kernels (metrics.hip,
// ensemble.hip); the torch form is torch_impl.image_map01.
#pragma once
#include "common.h"

// [-1, 1] -> the 8-bit value a PNG writer stores, 0 .. 255 (knn.hip; the torch
// form is torch_impl.image_map_u8): (uint8) trunc((clamp(x) + 1.0f) * 127.5f)
// with the fp32 add and multiply rounded separately (no FMA).
__device__ __forceinline__ int metric_map_u8(float x) {
  float c = fminf(fmaxf(x, -1.0f), 1.0f);
  return (int)__fmul_rn(__fadd_rn(c, 1.0f), 127.5f);
}

// [-1, 1] -> [0, 1].  quantize: through metric_map_u8, then / 255.
__device__ __forceinline__ double metric_map01(float x, int quantize) {
  if (quantize) return (double)metric_map_u8(x) / 255.0;
  float c = fminf(fmaxf(x, -1.0f), 1.0f);
  return ((double)c + 1.0) * 0.5;
}
