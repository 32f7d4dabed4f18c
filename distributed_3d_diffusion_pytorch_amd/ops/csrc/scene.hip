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
// The tracing rule itself (Hit, scene_trace) lives in scene_trace.h, which
// consistency.hip shares.
#include "scene_trace.h"

namespace {

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
  if (tid == 192) scene_kinv(Km + n * 9, sx, sy, cam, nullptr);     // inverse of diag(sx, sy, 1) K by the adjugate
  __syncthreads();
  if (tid < SC_SLOTS) scene_origin(S[tid], T);   // centre -> the camera origin in the primitive's frame, A (t - c)
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
