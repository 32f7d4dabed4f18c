// Multi-sample evaluation (ops.ensemble_stats; the torch form and the rule's
// oracle is torch_impl.ensemble_stats): the bias of the ensemble mean, the
// spread of the samples and the mean per-sample error of C samples of one
// target view, summed per visibility class.
//
// A group is C samples [C,3,H,W] and one target [3,H,W], fp32 in [-1, 1], and
// optionally a class plane [H,W] int32 (the plane of view_consistency: 0
// background, 1 disoccluded, 2 co-visible, 3 clean; without one every pixel is
// class 0).  With x_c the mapped sample c and y the mapped target (image_map.h,
// [0, 1] in fp64), per pixel p and channel ch:
//   m   = (x_0 + x_1 + ... + x_{C-1}) / C, summed with c ascending;
//   B_p = sum_ch (m - y)^2                      the squared error of the mean;
//   V_p = sum_ch (1 / C) sum_c (x_c - m)^2      the population variance, two-pass
//         from m (sum x^2 - m^2 would cancel on the flat backgrounds);
//   E_p = sum_ch (1 / C) sum_c (x_c - y)^2      the mean per-sample squared error;
// the sums over c ascending, the channel sums 0, 1, 2.  In exact arithmetic
// E_p = B_p + V_p; E is computed directly so that the relation is a check.
// stats [4,4] per group: row k = [n_k, sum B_p, sum V_p, sum E_p] over the
// pixels of class k; a pixel whose class is outside 0..3 enters no row.
// Optional maps: mean [3,H,W] fp32 = 2 m - 1, std [H,W] fp32 = sqrt(V_p / 3).
//
// Numerics: everything after the load is fp64, without contraction (each
// multiply and add rounds on its own, as the torch form's do).
//
// One thread per pixel, grid (ceil(H W / 256), groups), as view_consistency_k.
// Per channel the thread reads the C sample values twice, coalesced along the
// pixel: once for m, once for V and E (the second read hits the cache: the
// same addresses, C loads later).  Every block reduces its 16 doubles in a
// fixed order (wave shuffle tree, LDS, one thread over the 4 waves) into part
// [blocks,16]; ensemble_stats_final_k sums a group's blocks in ascending order.
// No atomics, bitwise reproducible; group i reads row i of every input only.
#include "image_map.h"

#define ES_STATS 16

namespace {

__global__ __launch_bounds__(256) void ensemble_stats_k(const float* __restrict__ smp, const float* __restrict__ tgt,
                                                        const int* __restrict__ cls, int C, long HW, int quantize,
                                                        double* __restrict__ part, float* __restrict__ mean,
                                                        float* __restrict__ sd) {
#pragma clang fp contract(off)
  __shared__ double red[4][ES_STATS];
  const int tid = threadIdx.x;
  const long n = blockIdx.y;
  const long pix = (long)blockIdx.x * 256 + tid;
  double acc[ES_STATS];
#pragma unroll
  for (int j = 0; j < ES_STATS; ++j) acc[j] = 0.0;

  if (pix < HW) {
    const float* x = smp + n * C * 3 * HW + pix;               // sample c, channel ch: x[(c * 3 + ch) * HW]
    const float* y = tgt + n * 3 * HW + pix;
    const double dC = (double)C;
    double B = 0.0, V = 0.0, E = 0.0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float* xc = x + ch * HW;
      const double yv = metric_map01(y[ch * HW], quantize);
      double s = metric_map01(xc[0], quantize);
      for (int c = 1; c < C; ++c) s += metric_map01(xc[(long)c * 3 * HW], quantize);
      const double m = s / dC;
      double v = 0.0, e = 0.0;
      for (int c = 0; c < C; ++c) {
        const double xv = metric_map01(xc[(long)c * 3 * HW], quantize);
        const double dv = xv - m, de = xv - yv;
        v += dv * dv;
        e += de * de;
      }
      const double db = m - yv;
      B += db * db;
      V += v / dC;
      E += e / dC;
      if (mean != nullptr) mean[(n * 3 + ch) * HW + pix] = (float)(2.0 * m - 1.0);
    }
    if (sd != nullptr) sd[n * HW + pix] = (float)sqrt(V / 3.0);
    const int k = cls != nullptr ? cls[n * HW + pix] : 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {                              // (a class outside 0..3 matches no row)
      const bool in = k == r;
      acc[4 * r + 0] = in ? 1.0 : 0.0;
      acc[4 * r + 1] = in ? B : 0.0;
      acc[4 * r + 2] = in ? V : 0.0;
      acc[4 * r + 3] = in ? E : 0.0;
    }
  }

  // block sum in a fixed order: the wave's shuffle tree, then the 4 waves in ascending order
#pragma unroll
  for (int j = 0; j < ES_STATS; ++j) {
    double v = acc[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    acc[j] = v;
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int j = 0; j < ES_STATS; ++j) red[tid >> 6][j] = acc[j];
  }
  __syncthreads();
  if (tid < ES_STATS)
    part[(n * gridDim.x + blockIdx.x) * ES_STATS + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// One thread per (group, column): the group's `blocks` partials in ascending order.
__global__ __launch_bounds__(256) void ensemble_stats_final_k(const double* __restrict__ part, long total, int blocks,
                                                              double* __restrict__ stats) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long n = i / ES_STATS;
  const int j = (int)(i % ES_STATS);
  const double* p = part + n * blocks * ES_STATS + j;
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s += p[(long)b * ES_STATS];
  stats[i] = s;
}
}  // namespace

// smp fp32 [G,C,3,H,W]; tgt fp32 [G,3,H,W]; cls int32 [G,H,W] or null; part
// fp64 [G * ceil(H W / 256), 16] workspace; stats fp64 [G,4,4]; mean fp32
// [G,3,H,W] or null; sd fp32 [G,H,W] or null.
D3D_API int d3d_ensemble_stats(const float* smp, const float* tgt, const int* cls, int G, int C, int H, int W,
                               int quantize, double* part, double* stats, float* mean, float* sd, hipStream_t st) {
  if (G <= 0 || C <= 0 || H <= 0 || W <= 0 || smp == nullptr || tgt == nullptr || part == nullptr ||
      stats == nullptr)
    return (int)hipErrorInvalidValue;
  const long HW = (long)H * W;
  const long gx = (HW + 255) / 256;
  if (gx > 0x7fffffffL) return (int)hipErrorInvalidValue;
  for (long n0 = 0; n0 < G; n0 += 65535) {     // grid.y limit
    const int nb = (int)(G - n0 < 65535 ? G - n0 : 65535);
    hipLaunchKernelGGL(ensemble_stats_k, dim3((unsigned)gx, (unsigned)nb), dim3(256), 0, st, smp + n0 * C * 3 * HW,
                       tgt + n0 * 3 * HW, cls ? cls + n0 * HW : nullptr, C, HW, quantize, part + n0 * gx * ES_STATS,
                       mean ? mean + n0 * 3 * HW : nullptr, sd ? sd + n0 * HW : nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  const long total = (long)G * ES_STATS;
  hipLaunchKernelGGL(ensemble_stats_final_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, part, total,
                     (int)gx, stats);
  return (int)hipGetLastError();
}
