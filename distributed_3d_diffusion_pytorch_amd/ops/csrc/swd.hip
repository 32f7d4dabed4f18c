// Sliced Wasserstein distance between two image sets on Laplacian-pyramid
// patches (ops.sliced_wasserstein; Karras et al. 2018; the torch form and the
// rule's oracle is torch_impl.sliced_wasserstein).  One number per pyramid
// level: fine texture at level 0, coarse shape at level L - 1.
//
// Inputs: a (the generated set), b (the real set), fp32 [N,3,H,W] in [-1, 1];
// levels L >= 1, patches P >= 1 per image and level, seed, quantize; dirs fp64
// [L,D,147].  H, W <= 128, divisible by 2^(L-1), the coarsest level >= 7 x 7.
//  1. Map.  x = metric_map01(., quantize) (image_map.h): fp64 in [0, 1].
//  2. Gaussian pyramid.  G_0 = x, G_{l+1} = down(G_l): the separable 5-tap
//     [1,4,6,4,1] / 16 blur per channel with reflect borders (index -i -> i,
//     S - 1 + i -> S - 1 - i: no edge repeat), along the row and then along
//     the column, taps ascending, then every second row and column from 0.
//  3. Laplacian pyramid.  up(g) puts g at the even rows and columns of a zero
//     plane of twice the size and blurs it the same way with gain 4 (each pass
//     divides by 8).  Level l < L - 1 is G_l - up(G_{l+1}); level L - 1 is
//     G_{L-1}.  Level l has H_l x W_l = (H >> l) x (W >> l) pixels.
//  4. Patches.  Image i takes P patches of 7 x 7 x 3 at level l: with q = (l N
//     + i) P + p the corner is x0 = hash_u32(seed ^ 0x1234567, 2 q) % (W_l - 6),
//     y0 = hash_u32(seed ^ 0x1234567, 2 q + 1) % (H_l - 6), the same for both
//     sets.  Element j = c 49 + dy 7 + dx; n = N P descriptors per set and level.
//  5. Normalise per set, level and channel: mu_c the mean and sigma_c the
//     population standard deviation (two passes: sum, then sum of (v - mu)^2)
//     over the n 49 values of channel c in the patches taken, a pixel counted
//     as often as it is taken; d = (v - mu_c) / sigma_c, and 1 / sigma_c := 0
//     where sigma_c is 0 (the channel then contributes nothing).
//  6. Directions.  dirs[l,k,:] is a unit vector (torch_impl.swd_directions),
//     built on the host for both backends and passed in: the fp32 log / cos of
//     normal01 need not agree bit for bit between host and device.
//  7. Score.  The key of descriptor d under direction k is d . theta_k, summed
//     in fp64 with j ascending and rounded ONCE to fp32.  swd[l] = (1 / D)
//     sum_k (1 / n) sum_i |sort(keys_a)_i - sort(keys_b)_i|, differences and
//     sums in fp64 in a fixed order.  fp64 [L], raw (ProGAN prints it x 1000);
//     exactly 0 for identical sets.
// n <= 16384: both sets' fp32 keys sit in one workgroup's LDS (2 x 64 KB).
//
// Numerics: fp64 after the load, without contraction.  The oracle keeps the
// keys in fp64; sorting is 1-Lipschitz in the sup norm, so the kernel is within
// 2^-23 max|key| of it (half an fp32 ulp per key and set) plus fp64 reordering.
//
// Kernels (no atomics anywhere; every sum has a fixed order: bitwise reproducible):
//  * swd_pyramid_k: one workgroup per (set, image, channel) builds the whole
//    pyramid of its plane in LDS and writes the fp64 Laplacian planes.  Level 0
//    stays in LDS as the fp32 values loaded and is mapped at every read -- the
//    map is a pure function of the fp32 value, so that is exact -- and only the
//    levels from 1 on are fp64: 64 KB + 42.5 KB at 128 x 128, inside the 160 KB,
//    so one launch and one code path serve every size and neither row bands
//    with halos nor a second launch are needed.  down and up are evaluated per
//    output pixel (25 and at most 9 LDS reads) in the separable form's order;
//    no intermediate plane exists.
//  * swd_stats_k: one workgroup per (set, level, channel): thread partials,
//    the wave's shuffle tree, the waves in ascending order; mu from the first
//    pass, sigma from the second.  It writes mu_c and 1 / sigma_c (not mu_c /
//    sigma_c: the projection subtracts mu_c before it scales, which does not
//    cancel when sigma_c is small against mu_c).
//  * swd_project_sort_k, grid (D, L): one workgroup per (direction, level).
//    theta_k / sigma_c of both sets goes to LDS; every thread forms the keys of
//    its descriptors of both sets straight from the Laplacian planes (no
//    descriptor or projection matrix exists), then both key arrays, padded with
//    +inf to a power of two M, are sorted by one bitonic network: a thread owns
//    E = 1, 4 or 16 consecutive keys of each set in registers; strides below E
//    are compare-exchanges in registers, strides below 64 E cross-lane moves
//    inside the wave, and only the strides from 64 E on go through LDS (two
//    barriers each: 20 barriers at M = 16384 where the plain one-barrier-per-
//    stage LDS network has 105 stages).  sum_{i<n} |a_i - b_i| in fp64 (the
//    padding sorts behind the n keys and never enters), one partial to [L,D].
//    d3d_swd_cfg(1) selects the plain network (every stride through LDS) for
//    A/B timing.
//  * swd_final_k: per level the D partials in k order, divided by D.
// Matrix instructions do not fit: the projection is a gathered fp64 dot product
// of 147 terms whose result feeds a sort, not a tile product.
#include "image_map.h"

#define SWD_PATCH 7
#define SWD_DIM 147
#define SWD_MAX_N 16384
#define SWD_MAX_SIDE 128
#define SWD_MAX_LEVELS 5                  // 128 >> 4 = 8 >= 7 > 128 >> 5
#define SWD_K_PATCH 0x1234567ull
#define SWD_SORT_TAIL ((2 * SWD_DIM + 6 + 16) * 8)   // theta of both sets, mu of both sets, the waves' partials

extern __shared__ __attribute__((aligned(16))) unsigned char swd_lds[];

namespace {

int g_swd_plain = 0;

__device__ __forceinline__ int swd_reflect(int i, int S) { return i < 0 ? -i : (i >= S ? 2 * S - 2 - i : i); }

// elements of the Laplacian workspace before level l: levels m < l hold [2,N,3,H_m,W_m]
__host__ __device__ __forceinline__ long swd_level_off(long N, int H, int W, int l) {
  long o = 0;
  for (int m = 0; m < l; ++m) o += 6 * N * (long)(H >> m) * (long)(W >> m);
  return o;
}

// block sum of a double, fixed order: the wave's shuffle tree, then the waves
// ascending; every thread gets the result.  red: 16 doubles of LDS.
__device__ __forceinline__ double swd_block_sum(double v, double* red) {
#pragma clang fp contract(off)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __syncthreads();                                 // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
  const int waves = (int)(blockDim.x >> 6);
  for (int w = 1; w < waves; ++w) s += red[w];
  return s;
}

__global__ __launch_bounds__(256) void swd_pyramid_k(const float* __restrict__ a, const float* __restrict__ b, long N,
                                                     int H, int W, int L, int quantize, double* __restrict__ lap) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  const long plane = blockIdx.x;                   // (set * N + image) * 3 + channel
  const long HW = (long)H * W;
  float* raw = reinterpret_cast<float*>(swd_lds);
  double* gl = reinterpret_cast<double*>(swd_lds + ((HW * 4 + 15) / 16) * 16);     // levels 1 .. L - 1, one after another
  const float* src = (plane < 3 * N ? a + plane * HW : b + (plane - 3 * N) * HW);
  for (int i = tid; i < HW; i += 256) raw[i] = src[i];
  __syncthreads();

  // level l's value: level 0 through the map, the others as stored (g: the level's plane in gl)
  auto rd = [&](int l, const double* g, int Ws, int y, int x) -> double {
    return l == 0 ? metric_map01(raw[y * Ws + x], quantize) : g[y * Ws + x];
  };
  const double w5[5] = {1.0, 4.0, 6.0, 4.0, 1.0};

  auto level = [&](int l) -> double* {             // level l >= 1 in gl (level 0 is raw)
    double* p = gl;
    for (int m = 1; m < l; ++m) p += (H >> m) * (W >> m);
    return p;
  };

  for (int l = 0; l + 1 < L; ++l) {
    const int Hs = H >> l, Ws = W >> l, Hd = Hs >> 1, Wd = Ws >> 1;
    const double* g = level(l);
    double* gn = level(l + 1);
    for (int i = tid; i < Hd * Wd; i += 256) {
      const int y = i / Wd, x = i - y * Wd;
      double s = 0.0;
#pragma unroll
      for (int dy = 0; dy < 5; ++dy) {
        const int ry = swd_reflect(2 * y + dy - 2, Hs);
        double h = 0.0;
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) {
          const double t = w5[dx] * rd(l, g, Ws, ry, swd_reflect(2 * x + dx - 2, Ws));
          h = dx == 0 ? t : h + t;
        }
        const double t = w5[dy] * (h / 16.0);
        s = dy == 0 ? t : s + t;
      }
      gn[i] = s / 16.0;
    }
    __syncthreads();
  }

  for (int l = 0; l < L; ++l) {
    const int Hs = H >> l, Ws = W >> l, Wd = Ws >> 1;
    const double* g = level(l);
    const double* gn = level(l + 1);
    double* out = lap + swd_level_off(N, H, W, l) + plane * (long)Hs * Ws;
    for (int i = tid; i < Hs * Ws; i += 256) {
      const int y = i / Ws, x = i - y * Ws;
      double v = rd(l, g, Ws, y, x);
      if (l + 1 < L) {
        // up(G_{l+1}) at (y, x): the zero plane's odd rows and columns add an exact 0 and are left out
        double s = 0.0;
#pragma unroll
        for (int dy = 0; dy < 5; ++dy) {
          const int ry = swd_reflect(y + dy - 2, Hs);
          if (ry & 1) continue;
          double h = 0.0;
#pragma unroll
          for (int dx = 0; dx < 5; ++dx) {
            const int rx = swd_reflect(x + dx - 2, Ws);
            if (rx & 1) continue;
            h += w5[dx] * gn[(ry >> 1) * Wd + (rx >> 1)];
          }
          s += w5[dy] * (h / 8.0);
        }
        v -= s / 8.0;
      }
      out[i] = v;
    }
  }
}

// the corner of descriptor e (image-major: image e / P) of level l
__device__ __forceinline__ void swd_corner(uint64_t pseed, long q, int Hl, int Wl, int& x0, int& y0) {
  x0 = (int)(hash_u32(pseed, 2ull * (uint64_t)q) % (uint32_t)(Wl - SWD_PATCH + 1));
  y0 = (int)(hash_u32(pseed, 2ull * (uint64_t)q + 1ull) % (uint32_t)(Hl - SWD_PATCH + 1));
}

// grid (3, L, 2) = (channel, level, set); stat [2,L,3,2] = (mu, 1 / sigma)
__global__ __launch_bounds__(1024) void swd_stats_k(const double* __restrict__ lap, long N, int P, int H, int W, int L,
                                                     uint64_t pseed, double* __restrict__ stat) {
#pragma clang fp contract(off)
  __shared__ double red[16];
  const int c = blockIdx.x, l = blockIdx.y, s = blockIdx.z;
  const int Hl = H >> l, Wl = W >> l;
  const long n = N * P, HWl = (long)Hl * Wl;
  const double* base = lap + swd_level_off(N, H, W, l) + ((long)s * N * 3 + c) * HWl;
  const double cnt = (double)(n * SWD_PATCH * SWD_PATCH);
  double mu = 0.0;
  for (int pass = 0; pass < 2; ++pass) {
    double acc = 0.0;
    for (long e = threadIdx.x; e < n; e += 1024) {
      int x0, y0;
      swd_corner(pseed, (long)l * n + e, Hl, Wl, x0, y0);
      const double* p = base + (e / P) * 3 * HWl + (long)y0 * Wl + x0;
      for (int dy = 0; dy < SWD_PATCH; ++dy)
#pragma unroll
        for (int dx = 0; dx < SWD_PATCH; ++dx) {
          const double v = p[dy * Wl + dx];
          if (pass == 0) {
            acc += v;
          } else {
            const double d = v - mu;
            acc += d * d;
          }
        }
    }
    const double tot = swd_block_sum(acc, red);
    if (pass == 0) {
      mu = tot / cnt;
    } else if (threadIdx.x == 0) {
      const double sd = sqrt(tot / cnt);
      double* o = stat + (((long)s * L + l) * 3 + c) * 2;
      o[0] = mu;
      o[1] = sd > 0.0 ? 1.0 / sd : 0.0;
    }
  }
}

template <int E>
__device__ __forceinline__ void swd_put(float* s, const float (&v)[E]) {
  if constexpr (E >= 4) {
#pragma unroll
    for (int r = 0; r < E; r += 4) {
      f32x4 t;
      t[0] = v[r]; t[1] = v[r + 1]; t[2] = v[r + 2]; t[3] = v[r + 3];
      *reinterpret_cast<f32x4*>(s + r) = t;
    }
  } else {
    s[0] = v[0];
  }
}
template <int E>
__device__ __forceinline__ void swd_get(const float* s, float (&v)[E]) {
  if constexpr (E >= 4) {
#pragma unroll
    for (int r = 0; r < E; r += 4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(s + r);
      v[r] = t[0]; v[r + 1] = t[1]; v[r + 2] = t[2]; v[r + 3] = t[3];
    }
  } else {
    v[0] = s[0];
  }
}

// A thread's keys against the partner's (o) at one stride: it keeps the smaller
// ones where its place in the pair and the run's direction agree.
template <int E>
__device__ __forceinline__ void swd_keep(float (&v)[E], const float (&o)[E], bool keep_min) {
#pragma unroll
  for (int r = 0; r < E; ++r) v[r] = keep_min ? fminf(v[r], o[r]) : fmaxf(v[r], o[r]);
}

// M keys per set, blockDim.x = M / E threads, thread t owns keys t E .. t E + E - 1.
// LDS: keys_a [M] fp32, keys_b [M] fp32, theta' [2,147] fp64, mu [2,3] fp64, red [16] fp64.
template <int E, bool PLAIN>
__global__ __launch_bounds__(1024) void swd_project_sort_k(const double* __restrict__ lap,
                                                            const double* __restrict__ stat,
                                                            const double* __restrict__ dirs, long N, int P, int H,
                                                            int W, int L, int D, uint64_t pseed, int M,
                                                            double* __restrict__ part) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, T = blockDim.x;
  const int k = blockIdx.x, l = blockIdx.y;
  const int Hl = H >> l, Wl = W >> l;
  const long HWl = (long)Hl * Wl;
  const int n = (int)(N * P);
  float* sa = reinterpret_cast<float*>(swd_lds);
  float* sb = sa + M;
  double* th = reinterpret_cast<double*>(sb + M);
  double* mus = th + 2 * SWD_DIM;
  double* red = mus + 6;

  // 1. theta_k scaled by each set's 1 / sigma_c; the sets' mu_c
  for (int j = tid; j < 2 * SWD_DIM; j += T) {
    const int s = j / SWD_DIM, jj = j - s * SWD_DIM, c = jj / (SWD_PATCH * SWD_PATCH);
    th[j] = dirs[((long)l * D + k) * SWD_DIM + jj] * stat[(((long)s * L + l) * 3 + c) * 2 + 1];
  }
  if (tid < 6) mus[tid] = stat[(((long)(tid / 3) * L + l) * 3 + tid % 3) * 2];
  __syncthreads();

  // 2. the keys of both sets (fp64 sum with j ascending, one rounding to fp32), +inf beyond n
  const double* la = lap + swd_level_off(N, H, W, l);
  const double* lb = la + N * 3 * HWl;
  for (int e = tid; e < M; e += T) {
    float fa = __builtin_inff(), fb = __builtin_inff();
    if (e < n) {
      int x0, y0;
      swd_corner(pseed, (long)l * n + e, Hl, Wl, x0, y0);
      const long o = (long)(e / P) * 3 * HWl + (long)y0 * Wl + x0;
      double acc_a = 0.0, acc_b = 0.0;
      for (int c = 0; c < 3; ++c) {
        const double ma = mus[c], mb = mus[3 + c];
        const double* pa = la + o + c * HWl;
        const double* pb = lb + o + c * HWl;
        const double* ta = th + c * SWD_PATCH * SWD_PATCH;
        for (int dy = 0; dy < SWD_PATCH; ++dy) {
#pragma unroll
          for (int dx = 0; dx < SWD_PATCH; ++dx) {
            acc_a += ta[dy * SWD_PATCH + dx] * (pa[dy * Wl + dx] - ma);
            acc_b += ta[SWD_DIM + dy * SWD_PATCH + dx] * (pb[dy * Wl + dx] - mb);
          }
        }
      }
      fa = (float)acc_a;
      fb = (float)acc_b;
    }
    sa[e] = fa;
    sb[e] = fb;
  }
  __syncthreads();

  // 3. one bitonic network over both arrays: element g = tid E + r meets g ^ j; runs of k2 ascend where g & k2 is 0
  float ka[E], kb[E], oa[E], ob[E];
  swd_get<E>(sa + tid * E, ka);
  swd_get<E>(sb + tid * E, kb);
  const int lds_from = PLAIN ? 1 : 64 * E;         // the smallest stride that goes through LDS
  for (int k2 = 2; k2 <= M; k2 <<= 1) {
    int j = k2 >> 1;
    for (; j >= lds_from; j >>= 1) {               // through LDS: the partner is in another wave
      swd_put<E>(sa + tid * E, ka);
      swd_put<E>(sb + tid * E, kb);
      __syncthreads();
      if (j >= E) {                                // the partner thread's keys, in order
        const int pt = tid ^ (j / E);
        swd_get<E>(sa + pt * E, oa);
        swd_get<E>(sb + pt * E, ob);
        const bool keep_min = (((tid * E) & j) == 0) == (((tid * E) & k2) == 0);
        swd_keep<E>(ka, oa, keep_min);
        swd_keep<E>(kb, ob, keep_min);
      } else {                                     // (the plain network only)
#pragma unroll
        for (int r = 0; r < E; ++r) {
          const int g = tid * E + r;
          const bool keep_min = ((g & j) == 0) == ((g & k2) == 0);
          const float xa = sa[g ^ j], xb = sb[g ^ j];
          ka[r] = keep_min ? fminf(ka[r], xa) : fmaxf(ka[r], xa);
          kb[r] = keep_min ? fminf(kb[r], xb) : fmaxf(kb[r], xb);
        }
      }
      __syncthreads();
    }
    for (; j >= E; j >>= 1) {                      // across the lanes of the wave
      const int m = j / E;
      const bool keep_min = ((tid & m) == 0) == (((tid * E) & k2) == 0);
#pragma unroll
      for (int r = 0; r < E; ++r) {
        oa[r] = __shfl_xor(ka[r], m, 64);
        ob[r] = __shfl_xor(kb[r], m, 64);
      }
      swd_keep<E>(ka, oa, keep_min);
      swd_keep<E>(kb, ob, keep_min);
    }
#pragma unroll
    for (int jr = E / 2; jr >= 1; jr >>= 1) {      // inside the thread's registers
      if (jr > j) continue;
#pragma unroll
      for (int r = 0; r < E; ++r) {
        if (r & jr) continue;
        const bool asc = ((tid * E + r) & k2) == 0;
        const float alo = fminf(ka[r], ka[r | jr]), ahi = fmaxf(ka[r], ka[r | jr]);
        const float blo = fminf(kb[r], kb[r | jr]), bhi = fmaxf(kb[r], kb[r | jr]);
        ka[r] = asc ? alo : ahi;
        ka[r | jr] = asc ? ahi : alo;
        kb[r] = asc ? blo : bhi;
        kb[r | jr] = asc ? bhi : blo;
      }
    }
  }

  // 4. sum_{i < n} |a_i - b_i|: the thread's keys ascending, the wave's tree, the waves ascending
  double acc = 0.0;
#pragma unroll
  for (int r = 0; r < E; ++r)
    if (tid * E + r < n) acc += fabs((double)ka[r] - (double)kb[r]);
  const double tot = swd_block_sum(acc, red);
  if (tid == 0) part[(long)l * D + k] = tot / (double)n;
}

__global__ __launch_bounds__(64) void swd_final_k(const double* __restrict__ part, int L, int D,
                                                  double* __restrict__ swd) {
#pragma clang fp contract(off)
  const int l = threadIdx.x;
  if (l >= L) return;
  double s = 0.0;
  for (int k = 0; k < D; ++k) s += part[(long)l * D + k];
  swd[l] = s / (double)D;
}

template <typename K>
hipError_t swd_lds_limit(K kernel, int bytes) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

template <int E, bool PLAIN>
hipError_t swd_sort_launch(const double* lap, const double* stat, const double* dirs, long N, int P, int H, int W,
                           int L, int D, uint64_t pseed, int M, double* part, hipStream_t st) {
  static const hipError_t once = swd_lds_limit(swd_project_sort_k<E, PLAIN>, 2 * SWD_MAX_N * 4 + SWD_SORT_TAIL);
  if (once != hipSuccess) return once;
  hipLaunchKernelGGL((swd_project_sort_k<E, PLAIN>), dim3((unsigned)D, (unsigned)L), dim3((unsigned)(M / E)),
                     (size_t)(2 * M * 4 + SWD_SORT_TAIL), st, lap, stat, dirs, N, P, H, W, L, D, pseed, M, part);
  return hipGetLastError();
}

int swd_pyramid_lds(int H, int W, int L) {
  long b = (((long)H * W * 4 + 15) / 16) * 16;
  for (int l = 1; l < L; ++l) b += (long)(H >> l) * (W >> l) * 8;
  return (int)b;
}
}  // namespace

// 1: the plain LDS bitonic network (every stride through LDS) for A/B timing; 0: the fused one.  Returns the old value.
D3D_API int d3d_swd_cfg(int plain) {
  const int old = g_swd_plain;
  if (plain >= 0) g_swd_plain = plain ? 1 : 0;
  return old;
}

// a, b fp32 [N,3,H,W]; dirs fp64 [L,D,147]; pseed = seed ^ 0x1234567 (64 bits);
// workspaces: lap fp64 [sum_l 2 N 3 H_l W_l], stat fp64 [2,L,3,2], part fp64
// [L,D] (all fully written); swd fp64 [L].
D3D_API int d3d_sliced_wasserstein(const float* a, const float* b, const double* dirs, long N, int H, int W, int L,
                                   int P, int D, uint64_t pseed, int quantize, double* lap, double* stat,
                                   double* part, double* swd, hipStream_t st) {
  if (a == nullptr || b == nullptr || dirs == nullptr || lap == nullptr || stat == nullptr || part == nullptr ||
      swd == nullptr || N < 1 || P < 1 || D < 1 || D > 65535 || L < 1 || L > SWD_MAX_LEVELS || H < 1 || W < 1 ||
      H > SWD_MAX_SIDE || W > SWD_MAX_SIDE || N * P > SWD_MAX_N)
    return (int)hipErrorInvalidValue;
  if (H % (1 << (L - 1)) || W % (1 << (L - 1)) || (H >> (L - 1)) < SWD_PATCH || (W >> (L - 1)) < SWD_PATCH)
    return (int)hipErrorInvalidValue;
  const int n = (int)(N * P);
  int M = 64;
  while (M < n) M <<= 1;

  static const hipError_t once = swd_lds_limit(swd_pyramid_k, swd_pyramid_lds(SWD_MAX_SIDE, SWD_MAX_SIDE, SWD_MAX_LEVELS));
  if (once != hipSuccess) return (int)once;
  hipLaunchKernelGGL(swd_pyramid_k, dim3((unsigned)(6 * N)), dim3(256), (size_t)swd_pyramid_lds(H, W, L), st, a, b, N,
                     H, W, L, quantize, lap);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(swd_stats_k, dim3(3, (unsigned)L, 2), dim3(1024), 0, st, (const double*)lap, N, P, H, W, L, pseed,
                     stat);
  e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  const bool plain = g_swd_plain != 0;
  if (M <= 1024)
    e = plain ? swd_sort_launch<1, true>(lap, stat, dirs, N, P, H, W, L, D, pseed, M, part, st)
              : swd_sort_launch<1, false>(lap, stat, dirs, N, P, H, W, L, D, pseed, M, part, st);
  else if (M <= 4096)
    e = plain ? swd_sort_launch<4, true>(lap, stat, dirs, N, P, H, W, L, D, pseed, M, part, st)
              : swd_sort_launch<4, false>(lap, stat, dirs, N, P, H, W, L, D, pseed, M, part, st);
  else
    e = plain ? swd_sort_launch<16, true>(lap, stat, dirs, N, P, H, W, L, D, pseed, M, part, st)
              : swd_sort_launch<16, false>(lap, stat, dirs, N, P, H, W, L, D, pseed, M, part, st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(swd_final_k, dim3(1), dim3(64), 0, st, (const double*)part, L, D, swd);
  return (int)hipGetLastError();
}
