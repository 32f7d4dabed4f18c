// Geometry-aware evaluation of the procedural scenes (ops.view_consistency;
// the torch form and the rule's oracle is torch_impl.view_consistency).
//
// A pair is one scene table [6,16] and K (the 128^2 intrinsics, rescaled by
// W / 128, H / 128 as in scene.hip), a source camera (R_s, t_s) with image src
// [3,H,W], a target camera (R_t, t_t) with image tgt [3,H,W] and optionally
// ref [3,H,W], the ground truth of the target view; images are fp32 in [-1, 1].
// The surface id of a ray is 8 prim + face, -1 on a miss; face is 0 for an
// ellipsoid and 1 + 2 ax + (sg > 0) for a box, ax / sg the entry axis and the
// normal's sign of the renderer's slab rule (scene_trace.h).
//
// For target pixel (px, py):
//   * the pixel-centre ray (px + 0.5, py + 0.5) of the target camera gives the
//     hit parameter tau, the surface id s0 and X = t_t + tau d.  A miss is
//     class 0, background.
//   * e = X - t_s, dist = |e|, c = R_s^T e, (u, v) = ((Ks c)_0, (Ks c)_1) /
//     (Ks c)_2 with Ks = diag(W / 128, H / 128, 1) K; the ray from t_s along
//     e / dist gives (tau1, s1).
//   * the pixel is co-visible iff c_z > 0, the bilinear footprint x0 =
//     floor(u - 0.5), y0 = floor(v - 0.5) has 0 <= x0, x0 + 1 <= W - 1 (and
//     likewise y0), |tau1 - dist| < 1e-9 and s1 == s0.  A hit pixel that is not
//     co-visible is class 1, disoccluded; a co-visible one is class 2.
//   * a co-visible pixel is clean, class 3, iff the four corner rays of the
//     target pixel (px + {0, 1}, py + {0, 1}) and the nine source rays through
//     the corner lattice (x0 + {0, 1, 2}, y0 + {0, 1, 2}) of the footprint all
//     have surface id s0: silhouettes, occlusion edges and box creases stay out
//     of the interpolation.
//   * warp = the bilinear interpolation of src at (u - 0.5, v - 0.5): weights
//     (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy, fx fy on (x0, y0), (x0 + 1,
//     y0), (x0, y0 + 1), (x0 + 1, y0 + 1), summed in that order in fp64.
// stats [8] per pair: [0..2] pixel counts of background, disoccluded,
// co-visible (class 3 counted in 2); [3] count of clean pixels; [4..6] the sum
// over the class's pixels and 3 channels of ((tgt - ref) / 2)^2 (0 without
// ref); [7] the sum over clean pixels and 3 channels of ((tgt - warp) / 2)^2.
//
// Numerics: everything is fp64 (the classes are decisions on fp64 rays, as the
// renderer's silhouettes are).
//
// One thread per target pixel, grid (ceil(H W / 256), pairs), as
// scene_render_k.  The table is staged in LDS twice, its centres replaced by
// the target and by the source origin in the primitive's frame -- the only
// part that differs between the cameras -- next to Kinv, R_t, Ks, R_s, t_t,
// t_s.  Up to 15 traces per thread, with early exits (background 1,
// disoccluded 2).  Every block reduces its 8 doubles in a fixed order (wave
// shuffle tree, LDS, one thread over the 4 waves) into part [blocks,8];
// view_consistency_final_k sums a pair's blocks in ascending order.  No
// atomics, bitwise reproducible; pair i reads row i of every input only.
#include "scene_trace.h"

#define VC_STATS 8

namespace {

__global__ __launch_bounds__(256) void view_consistency_k(
    const double* __restrict__ table, const double* __restrict__ Km, const double* __restrict__ Rs,
    const double* __restrict__ ts, const float* __restrict__ src, const double* __restrict__ Rt,
    const double* __restrict__ tt, const float* __restrict__ tgt, const float* __restrict__ ref, int H, int W,
    double sx, double sy, double* __restrict__ part, int* __restrict__ cls) {
  __shared__ double St[SC_SLOTS][SC_WORDS];    // origins: the target camera's
  __shared__ double Ss[SC_SLOTS][SC_WORDS];    // ... the source camera's
  __shared__ double cam[48];                   // Kinv [9], R_t [9], R_s [9], Ks [9], t_t [3], t_s [3]
  __shared__ double red[4][VC_STATS];
  const int tid = threadIdx.x;
  const long n = blockIdx.y;
  const double* Ki = cam;
  const double* RT = cam + 9;
  const double* RS = cam + 18;
  const double* KS = cam + 27;
  const double* TT = cam + 36;
  const double* TS = cam + 39;
  if (tid < SC_ROW) {
    const double w = table[n * SC_ROW + tid];
    St[tid / SC_WORDS][tid % SC_WORDS] = w;
    Ss[tid / SC_WORDS][tid % SC_WORDS] = w;
  }
  if (tid >= 128 && tid < 137) cam[9 + tid - 128] = Rt[n * 9 + tid - 128];
  if (tid >= 137 && tid < 146) cam[18 + tid - 137] = Rs[n * 9 + tid - 137];
  if (tid >= 146 && tid < 149) cam[36 + tid - 146] = tt[n * 3 + tid - 146];
  if (tid >= 149 && tid < 152) cam[39 + tid - 149] = ts[n * 3 + tid - 149];
  if (tid == 192) scene_kinv(Km + n * 9, sx, sy, cam, cam + 27);
  __syncthreads();
  if (tid < SC_SLOTS) scene_origin(St[tid], TT);
  if (tid >= 64 && tid < 64 + SC_SLOTS) scene_origin(Ss[tid - 64], TS);
  __syncthreads();

  const long HW = (long)H * W;
  const long pix = (long)blockIdx.x * 256 + tid;
  double acc[VC_STATS];
#pragma unroll
  for (int j = 0; j < VC_STATS; ++j) acc[j] = 0.0;

  if (pix < HW) {
    const int py = (int)(pix / W), px = (int)(pix % W);
    double d[3], nrm[3];
    scene_dir(Ki, RT, px + 0.5, py + 0.5, d);
    const Hit h0 = scene_nearest(St, d, nrm);
    const int s0 = scene_surface(h0);
    int klass = 0;
    int ix = 0, iy = 0;
    double fx = 0.0, fy = 0.0;
    if (s0 >= 0) {
      klass = 1;
      const double e0 = TT[0] + h0.t * d[0] - TS[0];
      const double e1 = TT[1] + h0.t * d[1] - TS[1];
      const double e2 = TT[2] + h0.t * d[2] - TS[2];
      const double dist = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
      const double c0 = RS[0] * e0 + RS[3] * e1 + RS[6] * e2;        // R_s^T e
      const double c1 = RS[1] * e0 + RS[4] * e1 + RS[7] * e2;
      const double c2 = RS[2] * e0 + RS[5] * e1 + RS[8] * e2;
      const double k0 = KS[0] * c0 + KS[1] * c1 + KS[2] * c2;
      const double k1 = KS[3] * c0 + KS[4] * c1 + KS[5] * c2;
      const double k2 = KS[6] * c0 + KS[7] * c1 + KS[8] * c2;
      const double u = k0 / k2, v = k1 / k2;
      const double x0 = floor(u - 0.5), y0 = floor(v - 0.5);
      const double ds[3] = {e0 / dist, e1 / dist, e2 / dist};
      const Hit h1 = scene_nearest(Ss, ds, nrm);
      const bool inside = x0 >= 0.0 && x0 + 1.0 <= (double)(W - 1) && y0 >= 0.0 && y0 + 1.0 <= (double)(H - 1);
      if (c2 > 0.0 && inside && fabs(h1.t - dist) < 1e-9 && scene_surface(h1) == s0) {
        klass = 2;
        ix = (int)x0;                          // inside: 0 <= ix <= W - 2, 0 <= iy <= H - 2
        iy = (int)y0;
        fx = (u - 0.5) - x0;
        fy = (v - 0.5) - y0;
        bool clean = true;
#pragma unroll 1
        for (int k = 0; k < 4 && clean; ++k) {           // the target pixel's corners
          scene_dir(Ki, RT, (double)(px + (k & 1)), (double)(py + (k >> 1)), d);
          clean = scene_surface(scene_nearest(St, d, nrm)) == s0;
        }
#pragma unroll 1
        for (int k = 0; k < 9 && clean; ++k) {           // the corner lattice of the source footprint
          scene_dir(Ki, RS, x0 + (double)(k % 3), y0 + (double)(k / 3), d);
          clean = scene_surface(scene_nearest(Ss, d, nrm)) == s0;
        }
        if (clean) klass = 3;
      }
    }
    if (cls != nullptr) cls[n * HW + pix] = klass;
    const int col = klass < 2 ? klass : 2;
    acc[col] = 1.0;
    if (klass == 3) acc[3] = 1.0;
    const float* g = tgt + n * 3 * HW + pix;
    if (ref != nullptr) {
      const float* r = ref + n * 3 * HW + pix;
      double se = 0.0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double q = ((double)g[c * HW] - (double)r[c * HW]) * 0.5;
        se += q * q;
      }
      acc[4 + col] = se;
    }
    if (klass == 3) {
      const float* s = src + n * 3 * HW + (long)iy * W + ix;
      const double w00 = (1.0 - fx) * (1.0 - fy), w01 = fx * (1.0 - fy), w10 = (1.0 - fx) * fy, w11 = fx * fy;
      double se = 0.0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float* sc = s + c * HW;
        const double warp = w00 * (double)sc[0] + w01 * (double)sc[1] + w10 * (double)sc[W] + w11 * (double)sc[W + 1];
        const double q = ((double)g[c * HW] - warp) * 0.5;
        se += q * q;
      }
      acc[7] = se;
    }
  }

  // block sum in a fixed order: the wave's shuffle tree, then the 4 waves in ascending order
#pragma unroll
  for (int j = 0; j < VC_STATS; ++j) {
    double v = acc[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    acc[j] = v;
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int j = 0; j < VC_STATS; ++j) red[tid >> 6][j] = acc[j];
  }
  __syncthreads();
  if (tid < VC_STATS)
    part[(n * gridDim.x + blockIdx.x) * VC_STATS + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// One thread per (pair, column): the pair's `blocks` partials in ascending order.
__global__ __launch_bounds__(256) void view_consistency_final_k(const double* __restrict__ part, long total,
                                                                int blocks, double* __restrict__ stats) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long n = i / VC_STATS;
  const int j = (int)(i % VC_STATS);
  const double* p = part + n * blocks * VC_STATS + j;
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s += p[(long)b * VC_STATS];
  stats[i] = s;
}
}  // namespace

// table fp64 [N,6,16]; Km fp64 [N,3,3], the intrinsics of the refsize x refsize
// image; Rs / Rt fp64 [N,3,3] cam-to-world, ts / tt fp64 [N,3]; src, tgt and
// ref (may be null) fp32 [N,3,H,W]; part fp64 [N * ceil(H W / 256), 8]
// workspace; stats fp64 [N,8]; cls int32 [N,H,W] or null.
D3D_API int d3d_view_consistency(const double* table, const double* Km, const double* Rs, const double* ts,
                                 const float* src, const double* Rt, const double* tt, const float* tgt,
                                 const float* ref, int N, int H, int W, int refsize, double* part, double* stats,
                                 int* cls, hipStream_t st) {
  if (N <= 0 || H <= 0 || W <= 0 || refsize <= 0 || part == nullptr || stats == nullptr)
    return (int)hipErrorInvalidValue;
  const long HW = (long)H * W;
  const long gx = (HW + 255) / 256;
  if (gx > 0x7fffffffL) return (int)hipErrorInvalidValue;
  const double sx = (double)W / refsize, sy = (double)H / refsize;
  for (long n0 = 0; n0 < N; n0 += 65535) {     // grid.y limit
    const int nb = (int)(N - n0 < 65535 ? N - n0 : 65535);
    hipLaunchKernelGGL(view_consistency_k, dim3((unsigned)gx, (unsigned)nb), dim3(256), 0, st, table + n0 * SC_ROW,
                       Km + n0 * 9, Rs + n0 * 9, ts + n0 * 3, src + n0 * 3 * HW, Rt + n0 * 9, tt + n0 * 3,
                       tgt + n0 * 3 * HW, ref ? ref + n0 * 3 * HW : nullptr, H, W, sx, sy,
                       part + n0 * gx * VC_STATS, cls ? cls + n0 * HW : nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  const long total = (long)N * VC_STATS;
  hipLaunchKernelGGL(view_consistency_final_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, part, total,
                     (int)gx, stats);
  return (int)hipGetLastError();
}
