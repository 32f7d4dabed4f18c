// Loss by noise level: per-example loss rows of a batch and their
// accumulation into a table of noise-level bins, all on the device (the head
// output, the target and logsnr already sit there; nothing goes to the host).
//
//   diff_loss_rows : rows[b] = (mean_{c,p} l(y - target), mean_{c,p} (y - target)^2)
//                    over the 3 HW valid elements of the padded NHWC head output
//   loss_bins      : table[bin(lambda_b)] += (1, row0, w row0, f_eps row1, f_x row1)
//
// Every reduction runs in a fixed order (no atomics): the rows and the table
// are bitwise reproducible, and a row depends on its own example only.
#include "common.h"

namespace {
// One block per (part, example): the example's pixels are dealt to ROWS_PARTS(HW)
// blocks of 256 threads, so a 16-example batch at 64 x 64 is 256 blocks, not
// 16.  Per pixel: one 16-byte load of y (channels 3..7 are dropped whatever
// they hold) and three target loads coalesced along the pixel.
// mode 0: l2, 1: l1, 2: huber (beta 1), as diff_loss_part_k.
// part[(b * NP + k) * 2 + {0, 1}] = the block's sums of l and of d^2.
__global__ void __launch_bounds__(256) diff_loss_rows_k(const bf16* __restrict__ y, const float* __restrict__ tgt,
                                                        int HW, int mode, float* __restrict__ part) {
  const int bb = blockIdx.y, NP = gridDim.x;
  const bf16* yb = y + (size_t)bb * HW * 8;
  const float* tb = tgt + (size_t)bb * 3 * HW;
  float al = 0.f, aq = 0.f;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += NP * 256) {
    const f32x8 v = ld8(yb + (size_t)p * 8);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float d = v[c] - tb[(size_t)c * HW + p];
      const float ad = fabsf(d);
      al += mode == 0 ? d * d : (mode == 1 ? ad : (ad < 1.f ? 0.5f * d * d : ad - 0.5f));
      aq += d * d;
    }
  }
  __shared__ float red[2][4];
  al = wave_sum(al);
  aq = wave_sum(aq);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = al;
    red[1][threadIdx.x >> 6] = aq;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const float* r = red[threadIdx.x];
    part[((size_t)bb * NP + blockIdx.x) * 2 + threadIdx.x] = (r[0] + r[1]) + (r[2] + r[3]);
  }
}

// rows[b][j] = (sum of the example's NP parts, in order) / (3 HW)
__global__ void diff_loss_rows_final_k(const float* __restrict__ part, int B, int NP, float inv_n,
                                       float* __restrict__ rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;      // (example, column)
  if (i >= 2 * B) return;
  const int bb = i >> 1, j = i & 1;
  float acc = 0.f;
  for (int k = 0; k < NP; ++k) acc += part[((size_t)bb * NP + k) * 2 + j];
  rows[i] = acc * inv_n;
}

// Bins are uniform in t: tau(lambda) = (atan(exp(-lambda / 2)) - b) / a is the
// schedule's inverse, bin = clamp(floor(tau NB), 0, NB - 1), all in fp64 from
// the fp32 lambda = logsnr[2 b + 1].  Columns (sums over the bin's examples):
//   0 count   1 row0   2 w(lambda) row0   3 f_eps row1   4 f_x row1
// w is the weight of diff_loss_part_k's WM (0 none, 1 min-SNR for an eps
// target, 2 for a v target); f_eps / f_x turn the squared error of the
// target (PRED 0: eps, 1: v) into eps / x0 units:
//   eps: f_eps = 1, f_x = e^-lambda      v: f_eps = sigmoid(lambda), f_x = sigmoid(-lambda)
// One block.  The examples are staged 256 at a time in shared memory; the
// thread that owns a bin then adds the bin's examples in example order.
struct BinRow {
  double v[4];
};

__global__ void __launch_bounds__(256) loss_bins_k(double* __restrict__ table, int NB, const float* __restrict__ rows,
                                                   const float* __restrict__ logsnr, int B, int pred, int wm,
                                                   double gamma, double a, double b0) {
  __shared__ BinRow val[256];
  __shared__ int bin[256];
  for (int c0 = 0; c0 < B; c0 += 256) {
    const int e = c0 + threadIdx.x;
    if (e < B) {
      const double lam = (double)logsnr[2 * e + 1];
      const double tau = (atan(exp(-0.5 * lam)) - b0) / a;
      double fb = floor(tau * NB);
      fb = fb < 0.0 ? 0.0 : (fb > (double)(NB - 1) ? (double)(NB - 1) : fb);      // (NaN ends in bin 0)
      bin[threadIdx.x] = fb == fb ? (int)fb : 0;
      const double en = exp(-fabs(lam));                      // sigmoid(+-lambda) without overflow
      const double hi = 1.0 / (1.0 + en), lo = en / (1.0 + en);
      const double sp = lam >= 0.0 ? hi : lo, sn = lam >= 0.0 ? lo : hi;
      double w = 1.0;
      if (wm == 1) w = fmin(1.0, gamma * exp(-lam));
      if (wm == 2) w = fmin(sp, gamma * sn);
      const double fe = pred == 0 ? 1.0 : sp, fx = pred == 0 ? exp(-lam) : sn;
      const double r0 = (double)rows[2 * e], r1 = (double)rows[2 * e + 1];
      BinRow r;
      r.v[0] = r0;
      r.v[1] = w * r0;
      r.v[2] = fe * r1;
      r.v[3] = fx * r1;
      val[threadIdx.x] = r;
    }
    __syncthreads();
    const int m = B - c0 < 256 ? B - c0 : 256;
    for (int j = threadIdx.x; j < NB; j += 256) {
      double* t = table + (size_t)j * 5;
      double cnt = t[0], s0 = t[1], s1 = t[2], s2 = t[3], s3 = t[4];
      for (int i = 0; i < m; ++i) {
        if (bin[i] != j) continue;
        cnt += 1.0;
        s0 += val[i].v[0];
        s1 += val[i].v[1];
        s2 += val[i].v[2];
        s3 += val[i].v[3];
      }
      t[0] = cnt;
      t[1] = s0;
      t[2] = s1;
      t[3] = s2;
      t[4] = s3;
    }
    __syncthreads();
  }
}
}  // namespace

// parts of an example: a function of HW alone (a row must not depend on the batch)
static inline int rows_parts(int HW) {
  int np = (HW + 255) / 256;
  return np < 1 ? 1 : (np > 16 ? 16 : np);
}

D3D_API int d3d_loss_rows_parts(int HW) { return rows_parts(HW); }

// y [B,H,W,8] bf16, target [B,3,H,W] fp32 -> rows [B,2] fp32; part: workspace
// of B * d3d_loss_rows_parts(HW) * 2 floats.
D3D_API int d3d_diff_loss_rows(const void* y, const float* target, int B, int HW, int CP, int mode, float* part,
                               float* rows, hipStream_t st) {
  if (CP != 8 || B < 1 || B > 65535 || HW < 1 || mode < 0 || mode > 2) return -1;
  const int NP = rows_parts(HW);
  hipLaunchKernelGGL(diff_loss_rows_k, dim3(NP, B), dim3(256), 0, st, (const bf16*)y, target, HW, mode, part);
  hipLaunchKernelGGL(diff_loss_rows_final_k, dim3(cdiv(2L * B, 256)), dim3(256), 0, st, part, B, NP,
                     1.f / (3.f * HW), rows);
  return (int)hipGetLastError();
}

// table [NB,5] fp64 += the batch (rows [B,2], logsnr [B,2]); every argument
// is a pointer or a constant of the launch: graph-capturable.
D3D_API int d3d_loss_bins(double* table, int NB, const float* rows, const float* logsnr, int B, int pred, int wmode,
                          double gamma, double a, double b0, hipStream_t st) {
  if (NB < 1 || B < 1 || pred < 0 || pred > 1 || wmode < 0 || wmode > 2 || !(a != 0.0)) return -1;
  hipLaunchKernelGGL(loss_bins_k, dim3(1), dim3(256), 0, st, table, NB, rows, logsnr, B, pred, wmode, gamma, a, b0);
  return (int)hipGetLastError();
}
