// The per-ray device code of the voxel radiance field, shared by field.hip
// (ops.field_render, ops.field_loss_grad) and field_fit.hip
// (ops.field_batch_loss_grad): the slab cut, the trilinear gather, the first
// walk (C of a ray) and the second walk (loss and gradient of a ray into the
// 64-bit fixed-point accumulator), the block's fixed-order loss sum and the
// accumulator's convert-and-clear pass.  field.hip states the rule in full.
// Both translation units are built with the same flags (packed fp32 ops off),
// so a ray gives the same bits through either.
#pragma once
#include "common.h"

#define FIELD_FIX_BITS 36
#define FIELD_T_MAX 3.0e38f

namespace {

__device__ __forceinline__ bool field_slab(float o, float d, float b, float& t0, float& t1) {
  if (d == 0.0f) return fabsf(o) <= b;
  const float ta = (-b - o) / d, tb = (b - o) / d;
  t0 = fmaxf(t0, fminf(ta, tb));
  t1 = fminf(t1, fmaxf(ta, tb));
  return true;
}

struct FieldRay {
  float o[3], d[3], t0, delta;
  bool hit;
};

__device__ __forceinline__ FieldRay field_load_ray(const float* __restrict__ ro, const float* __restrict__ rd, long r,
                                                   int S, float bound) {
  FieldRay q;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    q.o[a] = ro[r * 3 + a];
    q.d[a] = rd[r * 3 + a];
  }
  float t0 = 0.0f, t1 = FIELD_T_MAX;
  bool hit = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) hit = field_slab(q.o[a], q.d[a], bound, t0, t1) && hit;
  q.hit = hit && t1 > t0;
  q.t0 = t0;
  q.delta = q.hit ? (t1 - t0) / (float)S : 0.0f;
  return q;
}

// One sample: the cell, the trilinear weights toward the +1 corners and the
// interpolated raw channels.
struct FieldCell {
  long base;                 // element offset of corner (0, 0, 0)
  float f[3];                // fx, fy, fz
};

__device__ __forceinline__ float field_corner_w(const FieldCell& c, int k) {
  const float wx = (k & 1) ? c.f[0] : 1.0f - c.f[0];
  const float wy = (k & 2) ? c.f[1] : 1.0f - c.f[1];
  const float wz = (k & 4) ? c.f[2] : 1.0f - c.f[2];
  return (wz * wy) * wx;
}
__device__ __forceinline__ long field_corner_off(const FieldCell& c, int k, int G) {
  return c.base + ((long)((k >> 2) * G + ((k >> 1) & 1)) * G + (k & 1)) * 4;
}

__device__ __forceinline__ FieldCell field_locate(const FieldRay& q, int i, int G, float bound, float scale) {
  const float t = q.t0 + ((float)i + 0.5f) * q.delta;
  FieldCell c;
  int idx[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float p = q.o[a] + t * q.d[a];
    const float g = fminf(fmaxf((p + bound) * scale, 0.0f), (float)(G - 1));     // (a NaN clamps to 0)
    const int j = min((int)g, G - 2);
    idx[a] = j;
    c.f[a] = g - (float)j;
  }
  c.base = (((long)idx[2] * G + idx[1]) * G + idx[0]) * 4;
  return c;
}

__device__ __forceinline__ f32x4 field_gather(const float* __restrict__ grid, const FieldCell& c, int G) {
  f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const f32x4 n = *reinterpret_cast<const f32x4*>(grid + field_corner_off(c, k, G));
    const float w = field_corner_w(c, k);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += w * n[e];
  }
  return v;
}

__device__ __forceinline__ float field_softplus(float x) { return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float field_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// The first walk: C of a ray that hits.
__device__ __forceinline__ void field_walk(const float* __restrict__ grid, const FieldRay& q, int S, int G,
                                           float bound, float scale, float (&C)[3]) {
  float T = 1.0f;
  C[0] = C[1] = C[2] = 0.0f;
  for (int i = 0; i < S; ++i) {
    const FieldCell cell = field_locate(q, i, G, bound, scale);
    const f32x4 v = field_gather(grid, cell, G);
    const float alpha = -expm1f(-field_softplus(v[3]) * q.delta);
    const float w = T * alpha;
#pragma unroll
    for (int e = 0; e < 3; ++e) C[e] += w * field_sigmoid(v[e]);
    T *= 1.0f - alpha;
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) C[e] += T;          // the white background
}

// Ray r of (ro, rd, tgt) against grid: adds its squared error to loss and its
// gradient to acc (both walks; acc is the accumulator of that grid).
__device__ __forceinline__ void field_ray_loss_grad(double& loss, const float* __restrict__ grid,
                                                    const float* __restrict__ ro, const float* __restrict__ rd,
                                                    const float* __restrict__ tgt, unsigned long long* __restrict__ acc,
                                                    long r, int S, int G, float bound, float scale) {
  const FieldRay q = field_load_ray(ro, rd, r, S, bound);
  float C[3] = {1.0f, 1.0f, 1.0f};
  if (q.hit) field_walk(grid, q, S, G, bound, scale, C);
  float g[3];
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const double y01 = ((double)tgt[r * 3 + e] + 1.0) * 0.5;
    const double df = (double)C[e] - y01;
    loss += df * df;
    g[e] = (float)(2.0 * df);
  }
  if (q.hit) {
    // the second walk: C<=i runs along; every sample hands its derivatives to its 8 corners
    float T = 1.0f, Cacc[3] = {0.0f, 0.0f, 0.0f};
    for (int i = 0; i < S; ++i) {
      const FieldCell cell = field_locate(q, i, G, bound, scale);
      const f32x4 v = field_gather(grid, cell, G);
      const float alpha = -expm1f(-field_softplus(v[3]) * q.delta);
      const float w = T * alpha;
      const float Tn = T * (1.0f - alpha);
      float draw[4];
      float dsig = 0.0f;
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const float c = field_sigmoid(v[e]);
        Cacc[e] += w * c;
        dsig += g[e] * (q.delta * (Tn * c - (C[e] - Cacc[e])));
        draw[e] = g[e] * w * (c * (1.0f - c));
      }
      draw[3] = dsig * field_sigmoid(v[3]);
      T = Tn;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float wk = field_corner_w(cell, k);
        unsigned long long* a = acc + field_corner_off(cell, k, G);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const long long fx = __float2ll_rn((draw[e] * wk) * (float)(1ll << FIELD_FIX_BITS));
          if (fx != 0) atomicAdd(a + e, (unsigned long long)fx);
        }
      }
    }
  }
}

// The sum of a 256-thread block in a fixed order: the wave's shuffle tree, then
// the 4 waves in ascending order (red: 4 doubles of LDS; thread 0 holds the sum).
__device__ __forceinline__ double field_block_sum(double loss, double* red, int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) loss += __shfl_down(loss, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = loss;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// Fixed point -> fp32, and the accumulator back to zero for the next call.
__global__ __launch_bounds__(256) void field_convert_k(unsigned long long* __restrict__ acc, float* __restrict__ grad,
                                                       long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  grad[i] = (float)((double)(long long)acc[i] * (1.0 / (double)(1ll << FIELD_FIX_BITS)));
  acc[i] = 0ull;
}

// R S M <= 2^23 of the fixed-point range (field.hip): M = 6 max(1, delta_max).
inline bool field_fix_ok(long R, int S, double bound) {
  const double dmax = 2.0 * 1.7320508075688772 * bound / S;
  return (double)R * S * 6.0 * (dmax > 1.0 ? dmax : 1.0) <= 8388608.0;
}
}  // namespace
