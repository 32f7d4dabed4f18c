// Image metrics of the evaluation path: per-image (MSE, SSIM) of two fp32
// NCHW batches in [-1, 1], scored on the [0, 1] scale.
//
// SSIM is Wang et al. 2004 as tf.image.ssim / scikit-image (gaussian mode)
// compute it: per channel, 11-tap Gaussian (sigma 1.5) applied separably over
// the "valid" (H-10) x (W-10) window positions, L = 1, C1 = 0.01^2, C2 = 0.03^2.
//
// Numerics: SRN renders are mostly flat background, where E[x^2] - mu^2
// cancels to ~1e-7 in fp32 against C2 = 9e-4 (an SSIM error of 4e-4 on a flat
// pair).  Everything after the load is therefore fp64: the [0, 1] mapping, the
// five window sums, the SSIM expression and the reductions; only the final
// (mse, ssim) pair is rounded to fp32.  At [N, 3, 64, 64] the fp64 rate does
// not matter.
//
// Launch 1 (`image_metrics_tile_k`): one 256-thread block per (image, channel,
// 16 x 16 tile of window positions).  The 26 x 26 input patches of both images
// are staged in LDS once (out-of-image entries zero), a horizontal pass writes
// the five row-filtered quantities, a vertical pass forms the SSIM map, and a
// fixed-order tree writes one (squared error, SSIM sum) fp64 pair per block.
// Each pixel's squared error is counted by the one block whose 16 x 16 origin
// cell holds it; the last tile row / column also owns the border beyond it.
// Launch 2 (`image_metrics_final_k`): one wave per image sums that image's
// partials in a fixed order.  No atomics: image i's result does not depend on
// N or on the rest of the batch.
#include "image_map.h"

#define MT_TILE 16
#define MT_TAPS 11
#define MT_PATCH (MT_TILE + MT_TAPS - 1)

struct MetricTaps {
  double g[MT_TAPS];
};

// (the [-1, 1] -> [0, 1] mapping, metric_map01, is image_map.h)

__global__ __launch_bounds__(256) void image_metrics_tile_k(const float* __restrict__ X, const float* __restrict__ Y,
                                                            int H, int W, int TY, int TX, int quantize,
                                                            MetricTaps taps, double* __restrict__ part) {
  __shared__ double xs[MT_PATCH][MT_PATCH];
  __shared__ double ys[MT_PATCH][MT_PATCH];
  __shared__ double hs[5][MT_PATCH][MT_TILE];
  __shared__ double red[2][256];
  const int tid = threadIdx.x;
  const int tiles = TY * TX;
  const int t = blockIdx.x % tiles;
  const long nc = blockIdx.x / tiles;              // image * C + channel
  const int ty = t / TX, tx = t % TX;
  const int r0 = ty * MT_TILE, c0 = tx * MT_TILE;
  const int ph = min(MT_PATCH, H - r0), pw = min(MT_PATCH, W - c0);   // patch rows / cols inside the image
  const int own_h = (ty == TY - 1) ? ph : MT_TILE;                   // pixels whose squared error this block counts
  const int own_w = (tx == TX - 1) ? pw : MT_TILE;
  const float* xp = X + nc * H * W + (long)r0 * W + c0;
  const float* yp = Y + nc * H * W + (long)r0 * W + c0;

  double se = 0.0;
  for (int e = tid; e < MT_PATCH * MT_PATCH; e += 256) {
    const int r = e / MT_PATCH, c = e % MT_PATCH;
    double vx = 0.0, vy = 0.0;
    if (r < ph && c < pw) {
      vx = metric_map01(xp[(long)r * W + c], quantize);
      vy = metric_map01(yp[(long)r * W + c], quantize);
      if (r < own_h && c < own_w) {
        const double d = vx - vy;
        se += d * d;
      }
    }
    xs[r][c] = vx;
    ys[r][c] = vy;
  }
  __syncthreads();

  // horizontal pass: row r, window column j reads patch columns j .. j + 10
  for (int e = tid; e < MT_PATCH * MT_TILE; e += 256) {
    const int r = e / MT_TILE, j = e % MT_TILE;
    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
    for (int k = 0; k < MT_TAPS; ++k) {
      const double g = taps.g[k], a = xs[r][j + k], b = ys[r][j + k];
      sx += g * a;
      sy += g * b;
      sxx += g * (a * a);
      syy += g * (b * b);
      sxy += g * (a * b);
    }
    hs[0][r][j] = sx;
    hs[1][r][j] = sy;
    hs[2][r][j] = sxx;
    hs[3][r][j] = syy;
    hs[4][r][j] = sxy;
  }
  __syncthreads();

  // vertical pass: window (i, j) reads filtered rows i .. i + 10
  const int i = tid / MT_TILE, j = tid % MT_TILE;
  double ssim = 0.0;
  if (r0 + i < H - (MT_TAPS - 1) && c0 + j < W - (MT_TAPS - 1)) {
    double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < MT_TAPS; ++k) {
      const double g = taps.g[k];
#pragma unroll
      for (int q = 0; q < 5; ++q) m[q] += g * hs[q][i + k][j];
    }
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    const double mxx = m[0] * m[0], myy = m[1] * m[1], mxy = m[0] * m[1];
    const double vx = m[2] - mxx, vy = m[3] - myy, cxy = m[4] - mxy;
    ssim = ((2.0 * mxy + C1) * (2.0 * cxy + C2)) / ((mxx + myy + C1) * (vx + vy + C2));
  }

  red[0][tid] = se;
  red[1][tid] = ssim;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] += red[0][tid + s];
      red[1][tid] += red[1][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    part[2 * (long)blockIdx.x] = red[0][0];
    part[2 * (long)blockIdx.x + 1] = red[1][0];
  }
}

// One wave per image: P = C * TY * TX partial pairs, summed lane-strided and
// then through a fixed tree.
__global__ __launch_bounds__(64) void image_metrics_final_k(const double* __restrict__ part, int P, double n_pix,
                                                            double n_win, float* __restrict__ out) {
  __shared__ double red[2][64];
  const int tid = threadIdx.x;
  const double* p = part + 2 * (long)blockIdx.x * P;
  double se = 0.0, ss = 0.0;
  for (int e = tid; e < P; e += 64) {
    se += p[2 * e];
    ss += p[2 * e + 1];
  }
  red[0][tid] = se;
  red[1][tid] = ss;
  __syncthreads();
  for (int s = 32; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] += red[0][tid + s];
      red[1][tid] += red[1][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    out[2 * (long)blockIdx.x] = (float)(red[0][0] / n_pix);
    out[2 * (long)blockIdx.x + 1] = (float)(red[1][0] / n_win);
  }
}

// Blocks of launch 1 (= fp64 pairs the caller provides in `part`;
// hip_impl.image_metrics sizes it by the same rule), or -1 when the shape is
// not covered.
static long image_metrics_blocks(int N, int C, int H, int W) {
  if (N <= 0 || C <= 0 || H < MT_TAPS || W < MT_TAPS) return -1;
  const long tiles = (long)cdiv(H - (MT_TAPS - 1), MT_TILE) * cdiv(W - (MT_TAPS - 1), MT_TILE);
  const long blocks = (long)N * C * tiles;
  if ((long)C * tiles > 0x7fffffffL || blocks > 0x7fffffffL) return -1;
  return blocks;
}

// X, Y: fp32 contiguous [N, C, H, W]; taps: 11 host doubles (the normalised
// Gaussian window); part: fp64 [blocks, 2] scratch; out: fp32 [N, 2] (mse, ssim).
D3D_API int d3d_image_metrics(const float* X, const float* Y, int N, int C, int H, int W, int quantize,
                              const double* taps, double* part, float* out, hipStream_t stream) {
  const long blocks = image_metrics_blocks(N, C, H, W);
  if (blocks < 0 || taps == nullptr) return (int)hipErrorInvalidValue;
  MetricTaps tp;
  for (int k = 0; k < MT_TAPS; ++k) tp.g[k] = taps[k];
  const int TY = cdiv(H - (MT_TAPS - 1), MT_TILE), TX = cdiv(W - (MT_TAPS - 1), MT_TILE);
  hipLaunchKernelGGL(image_metrics_tile_k, dim3((unsigned)blocks), dim3(256), 0, stream, X, Y, H, W, TY, TX, quantize,
                     tp, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(image_metrics_final_k, dim3((unsigned)N), dim3(64), 0, stream, part, C * TY * TX,
                     (double)C * H * W, (double)C * (H - (MT_TAPS - 1)) * (W - (MT_TAPS - 1)), out);
  return (int)hipGetLastError();
}
