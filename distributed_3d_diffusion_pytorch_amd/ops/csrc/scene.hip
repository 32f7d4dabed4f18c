// Procedural multi-view scenes: an analytic ray caster (data/procedural.py;
// the torch form and the rule's oracle is torch_impl.scene_render).
//
// An image is one object of up to SC_SLOTS primitives seen by one pinhole
// camera.  A table row holds 16 fp64 words per slot:
//   [0..8]   A, row-major: world -> the unit primitive (diag(1/axes) R^T)
//   [9..11]  centre          [12..14] albedo
//   [15]     kind: 0 empty, 1 ellipsoid (unit sphere), 2 box ([-1, 1]^3)
// The ray through pixel coordinates (u, v) is  o = t,
//   d = R normalize(Kinv [u, v, 1]),  Kinv = inverse(diag(sx, sy, 1) K)
// (ops.camera_rays with rescale_from: K is the 128^2 matrix, sx = W / 128,
// sy = H / 128).  It hits the nearest primitive with t > 0 (the lowest slot
// on a tie); ellipsoid: the near root, discriminant > 0; box: slabs, tmin <
// tmax, the entry face's normal (the lowest axis on a tie).  Colour =
// albedo (0.35 + 0.65 max(0, n . l)), n = normalize(A^T n_local), l the fixed
// world light normalize(0.3, 0.2, 1); a miss is white.  A pixel is the mean of
// its aa x aa sub-pixel rays (offsets (i + 0.5) / aa, row-major, summed in that
// order), stored as 2 c - 1.  depth / prim come from the pixel-centre ray.
//
// Numerics: everything is fp64 and is rounded once, at the store, so the
// kernel stays within rounding of the fp64 oracle and silhouettes do not flip
// (the same call as metrics.hip; ~50 M ray-primitive tests for 256 images of
// 64 x 64 at aa = 3 are small against the fp64 vector rate).
//
// One thread per pixel, grid (ceil(H W / 256), images).  The image's table,
// with each centre replaced by the camera origin in the primitive's frame
// A (t - c), and its camera (Kinv, R) are staged in LDS once per block; the
// slot loop reads them through wave-uniform (broadcast) LDS addresses and
// branches on the slot's kind, which is uniform over the block.  No atomics;
// image i reads row i of every input only.
#include "common.h"

#define SC_SLOTS 6
#define SC_WORDS 16
#define SC_ROW (SC_SLOTS * SC_WORDS)

namespace {

struct Hit {
  double t;        // ray parameter of the nearest hit (+inf: miss); |d| = 1, so also the distance
  int prim;        // slot of the hit, -1 on a miss
  double c[3];     // colour in [0, 1]
};

__device__ __forceinline__ Hit scene_trace(const double (*S)[SC_WORDS], const double* cam, double u, double v) {
  const double* Ki = cam;
  const double* R = cam + 9;
  double c0 = Ki[0] * u + Ki[1] * v + Ki[2];
  double c1 = Ki[3] * u + Ki[4] * v + Ki[5];
  double c2 = Ki[6] * u + Ki[7] * v + Ki[8];
  const double nrm = sqrt(c0 * c0 + c1 * c1 + c2 * c2);
  c0 /= nrm;
  c1 /= nrm;
  c2 /= nrm;
  const double d0 = R[0] * c0 + R[1] * c1 + R[2] * c2;
  const double d1 = R[3] * c0 + R[4] * c1 + R[5] * c2;
  const double d2 = R[6] * c0 + R[7] * c1 + R[8] * c2;

  Hit h;
  h.t = __builtin_inf();
  h.prim = -1;
  double n0 = 0.0, n1 = 0.0, n2 = 0.0;          // the hit's normal in the primitive's frame
#pragma unroll 1      // (unrolled, both kinds of all six slots are live at once: 260 VGPRs against 112)
  for (int p = 0; p < SC_SLOTS; ++p) {
    const double* s = S[p];
    const int kind = (int)s[15];                // uniform over the block
    if (kind == 0) continue;
    const double q[3] = {s[0] * d0 + s[1] * d1 + s[2] * d2, s[3] * d0 + s[4] * d1 + s[5] * d2,
                         s[6] * d0 + s[7] * d1 + s[8] * d2};
    const double o[3] = {s[9], s[10], s[11]};
    double tt, m0, m1, m2;
    bool hit;
    if (kind == 1) {
      const double a = q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
      const double b = o[0] * q[0] + o[1] * q[1] + o[2] * q[2];
      const double c = o[0] * o[0] + o[1] * o[1] + o[2] * o[2] - 1.0;
      const double disc = b * b - a * c;
      hit = disc > 0.0;
      tt = (-b - sqrt(hit ? disc : 0.0)) / a;
      m0 = o[0] + tt * q[0];
      m1 = o[1] + tt * q[1];
      m2 = o[2] + tt * q[2];
    } else {
      double tmin = -__builtin_inf(), tmax = __builtin_inf();
      int ax = 0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double inv = 1.0 / q[k];
        const double t1 = (-1.0 - o[k]) * inv, t2 = (1.0 - o[k]) * inv;
        const double tn = fmin(t1, t2), tf = fmax(t1, t2);
        if (tn > tmin) {
          tmin = tn;
          ax = k;
        }
        tmax = fmin(tmax, tf);
      }
      hit = tmin < tmax;
      tt = tmin;
      const double sg = q[ax] > 0.0 ? -1.0 : 1.0;
      m0 = ax == 0 ? sg : 0.0;
      m1 = ax == 1 ? sg : 0.0;
      m2 = ax == 2 ? sg : 0.0;
    }
    if (hit && tt > 0.0 && tt < h.t) {
      h.t = tt;
      h.prim = p;
      n0 = m0;
      n1 = m1;
      n2 = m2;
    }
  }
  h.c[0] = h.c[1] = h.c[2] = 1.0;
  if (h.prim >= 0) {
    const double* s = S[h.prim];
    double w0 = s[0] * n0 + s[3] * n1 + s[6] * n2;      // A^T n_local
    double w1 = s[1] * n0 + s[4] * n1 + s[7] * n2;
    double w2 = s[2] * n0 + s[5] * n1 + s[8] * n2;
    const double wn = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
    w0 /= wn;
    w1 /= wn;
    w2 /= wn;
    const double ln = sqrt(0.3 * 0.3 + 0.2 * 0.2 + 1.0 * 1.0);
    const double ndl = w0 * (0.3 / ln) + w1 * (0.2 / ln) + w2 * (1.0 / ln);
    const double shade = 0.35 + 0.65 * fmax(ndl, 0.0);
    h.c[0] = s[12] * shade;
    h.c[1] = s[13] * shade;
    h.c[2] = s[14] * shade;
  }
  return h;
}

__global__ __launch_bounds__(256) void scene_render_k(const double* __restrict__ table, const double* __restrict__ Rm,
                                                      const double* __restrict__ tv, const double* __restrict__ Km,
                                                      int H, int W, int aa, double sx, double sy,
                                                      float* __restrict__ img, float* __restrict__ depth,
                                                      int* __restrict__ prim) {
  __shared__ double S[SC_SLOTS][SC_WORDS];
  __shared__ double cam[18];                   // Kinv [9], R [9]
  const int tid = threadIdx.x;
  const long n = blockIdx.y;
  const double* T = tv + n * 3;
  if (tid < SC_ROW) S[tid / SC_WORDS][tid % SC_WORDS] = table[n * SC_ROW + tid];
  if (tid >= 128 && tid < 137) cam[9 + tid - 128] = Rm[n * 9 + tid - 128];
  if (tid == 192) {                            // inverse of diag(sx, sy, 1) K by the adjugate
    const double* k = Km + n * 9;
    const double a = k[0] * sx, b = k[1] * sx, c = k[2] * sx;
    const double d = k[3] * sy, e = k[4] * sy, f = k[5] * sy;
    const double g = k[6], h = k[7], i = k[8];
    const double A = e * i - f * h, B = f * g - d * i, C = d * h - e * g;
    const double det = a * A + b * B + c * C;
    const double adj[9] = {A, c * h - b * i, b * f - c * e, B, a * i - c * g, c * d - a * f, C, b * g - a * h,
                           a * e - b * d};
#pragma unroll
    for (int j = 0; j < 9; ++j) cam[j] = adj[j] / det;
  }
  __syncthreads();
  if (tid < SC_SLOTS) {                        // centre -> the camera origin in the primitive's frame, A (t - c)
    double* s = S[tid];
    const double x = T[0] - s[9], y = T[1] - s[10], z = T[2] - s[11];
    s[9] = s[0] * x + s[1] * y + s[2] * z;
    s[10] = s[3] * x + s[4] * y + s[5] * z;
    s[11] = s[6] * x + s[7] * y + s[8] * z;
  }
  __syncthreads();

  const long HW = (long)H * W;
  const long pix = (long)blockIdx.x * 256 + tid;
  if (pix >= HW) return;
  const int py = (int)(pix / W), px = (int)(pix % W);

  double acc[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < aa; ++i)
    for (int j = 0; j < aa; ++j) {
      const Hit h = scene_trace(S, cam, px + (j + 0.5) / aa, py + (i + 0.5) / aa);
      acc[0] += h.c[0];
      acc[1] += h.c[1];
      acc[2] += h.c[2];
    }
  const double cnt = (double)(aa * aa);
  float* o = img + n * 3 * HW + pix;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c * HW] = (float)(2.0 * (acc[c] / cnt) - 1.0);
  if (depth != nullptr) {
    const Hit h = scene_trace(S, cam, px + 0.5, py + 0.5);
    depth[n * HW + pix] = (float)h.t;
    prim[n * HW + pix] = h.prim;
  }
}
}  // namespace

// table fp64 [N,6,16]; Rm fp64 [N,3,3] cam-to-world; tv fp64 [N,3]; Km fp64
// [N,3,3], the intrinsics of the ref x ref image (rows 0 / 1 are scaled by
// W / ref, H / ref here); img fp32 [N,3,H,W]; depth fp32 [N,H,W] and prim
// int32 [N,H,W], both null or both set.
D3D_API int d3d_scene_render(const double* table, const double* Rm, const double* tv, const double* Km, int N, int H,
                             int W, int aa, int ref, float* img, float* depth, int* prim, hipStream_t st) {
  if (N <= 0 || H <= 0 || W <= 0 || ref <= 0 || aa < 1 || aa > 4 || (depth == nullptr) != (prim == nullptr))
    return (int)hipErrorInvalidValue;
  const long HW = (long)H * W;
  const long gx = (HW + 255) / 256;
  if (gx > 0x7fffffffL) return (int)hipErrorInvalidValue;
  const double sx = (double)W / ref, sy = (double)H / ref;
  for (long n0 = 0; n0 < N; n0 += 65535) {     // grid.y limit
    const int nb = (int)(N - n0 < 65535 ? N - n0 : 65535);
    hipLaunchKernelGGL(scene_render_k, dim3((unsigned)gx, (unsigned)nb), dim3(256), 0, st, table + n0 * SC_ROW,
                       Rm + n0 * 9, tv + n0 * 3, Km + n0 * 9, H, W, aa, sx, sy, img + n0 * 3 * HW,
                       depth ? depth + n0 * HW : nullptr, prim ? prim + n0 * HW : nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return (int)hipSuccess;
}
