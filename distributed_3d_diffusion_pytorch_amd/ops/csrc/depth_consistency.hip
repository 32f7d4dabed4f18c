// Depth reprojection consistency between the V views of an object
// (ops.depth_consistency; the torch form and the rule's oracle is
// torch_impl.depth_consistency).  Every view carries a depth plane -- the
// depth of a fitted field (plane 1 of field_geom.hip's maps) or of the
// renderer (scene.hip's depth aux) -- so a target pixel can be lifted to a
// point, projected into every other view and compared with what that view
// shows there: the geometry comes from the depths, the appearance from the
// images themselves.  No scene table is needed.
//
// Inputs, per field f < F: depth fp32 [F,V,H,W], a distance along the unit
// pixel-centre ray, +inf where the view sees no surface; img fp32 [F,V,3,H,W]
// in [-1, 1]; K fp64 [F,3,3]; R fp64 [F,V,3,3] cam-to-world; t fp64 [F,V,3];
// tol > 0.  Cameras are scene.hip's: Ks = diag(W / ref, H / ref, 1) K (ref = 0:
// K itself), Kinv its inverse by the adjugate, and the ray of pixel (px, py) is
// d = R_a normalize(Kinv [px + 1/2, py + 1/2, 1]).  Per source view b the
// projection is formed once: P_b = Ks R_b^T, P_b[i][j] = sum_k Ks[i][k]
// R_b[j][k] with k ascending, and z_b = the third column of R_b.
//
// For target pixel (px, py) of view a, D = depth[a, py, px]:
//   * D not finite: class 0, background, for every b.
//   * otherwise X = t_a + D d, and for each source b != a:
//       e = X - t_b, dist = |e|, c_z = z_b . e (the z of R_b^T e), k = P_b e,
//       (u, v) = (k_0, k_1) / k_2,
//       x0 = floor(u - 1/2), y0 = floor(v - 1/2), fx = u - 1/2 - x0, fy = v -
//       1/2 - y0; inside: 0 <= x0, x0 + 1 <= W - 1, 0 <= y0, y0 + 1 <= H - 1;
//       the four source depths q_k = depth[b, y0 + {0, 1}, x0 + {0, 1}] and
//       q_n, the tap nearest to (u - 1/2, v - 1/2): x0 + (fx >= 1/2), y0 +
//       (fy >= 1/2).
//   * co-visible, class 2, iff c_z > 0, inside, q_n finite and |dist - q_n| <=
//     tol dist.  A hit pixel that is not co-visible is class 1, hidden:
//     occluded, outside the source image or on the source's background.
//   * clean, class 3, iff co-visible, all four q_k are finite with |dist - q_k|
//     <= tol dist, and every 4-neighbour of (px, py) inside the target image
//     has a finite depth D' with |D' - D| <= tol D: silhouettes and depth edges
//     stay out of the interpolation on both sides.
//   * warp = the bilinear sample of img[b] at (u - 1/2, v - 1/2) with
//     consistency.hip's weights and order: (1 - fx)(1 - fy), fx (1 - fy),
//     (1 - fx) fy, fx fy on (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1,
//     y0 + 1), summed in that order; qbar = the same sample of the four q_k,
//     formed for clean pixels only.
// stats [F,V,V,7], index [f,a,b]: [0..2] the pixel counts of background,
// hidden, co-visible (class 3 counted in 2); [3] clean pixels; [4] the sum over
// co-visible pixels and 3 channels of ((tgt - warp) / 2)^2; [5] the same over
// clean pixels; [6] the sum over clean pixels of |dist - qbar|.  Rows [f,a,a]
// are zero and their class plane is -1.
//
// Numerics: fp64 throughout, the depth and image words upcast once, nothing
// contracted into fmas.
//
// Work split: a wave owns an 8 x 8 target tile, so the footprints of its lanes
// fall into a compact patch of a source's planes; a 256-thread block owns four
// consecutive tiles (row order) of one (field, target view); launch grid
// (ceil(tiles / 4), V, F), the fields chunked to the grid limit.  Staged in LDS
// once per block: Kinv, R_a, t_a and, for all V views, P_b, z_b and t_b (15
// doubles a view), which the source loop reads through wave-uniform addresses.
// A lane does the target side once -- ray, D, X, its three colours and the
// neighbour test -- and keeps it in registers over the source loop, b
// ascending.  The source depths and colours are gathered through L2: a block
// touches a few hundred words of a plane, far fewer than staging the plane
// would move (profiles/field/README.md has both timings).  Per source the four
// counts are the population counts of the wave's ballots (sums of ones are
// exact in any order) and the three fp64 sums go through the wave's shuffle
// tree; lane 0 parks them in LDS.  After one barrier the block adds its four
// waves in ascending order into part [F,V,V,blocks,7], and
// depth_consistency_final_k adds a row's blocks in ascending order.  No
// atomics: bitwise reproducible; a field's rows read only that field's inputs,
// so a batched call equals the single calls bit for bit.  The launcher takes
// pointers and constants and never synchronises: it can be captured.
#pragma clang fp contract(off)
#include "scene_trace.h"

#define DC_STATS 7
#define DC_MAXV 64
#define DC_SRC 15        // per source view: P [9], z [3], t [3]

namespace {

template <bool CLS>
__global__ __launch_bounds__(256) void depth_consistency_k(const float* __restrict__ depth,
                                                           const float* __restrict__ img,
                                                           const double* __restrict__ Km,
                                                           const double* __restrict__ Rm,
                                                           const double* __restrict__ tv, double* __restrict__ part,
                                                           int* __restrict__ cls, int V, int H, int W, double tol,
                                                           double sx, double sy, int f0) {
  __shared__ double cam[21];                   // Kinv [9], R_a [9], t_a [3]
  __shared__ double src[DC_MAXV][DC_SRC];
  __shared__ double red[DC_MAXV][4][3];        // per source and wave: stats 4..6
  __shared__ int cnt[DC_MAXV][4][4];           // ... stats 0..3
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int a = blockIdx.y;
  const long f = f0 + (long)blockIdx.z, fa = f * V + a;
  if (tid < V) {
    const double* k = Km + f * 9;
    const double* R = Rm + (f * V + tid) * 9;
    const double ks[9] = {k[0] * sx, k[1] * sx, k[2] * sx, k[3] * sy, k[4] * sy, k[5] * sy, k[6], k[7], k[8]};
    double* s = src[tid];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        s[3 * i + j] = ks[3 * i] * R[3 * j] + ks[3 * i + 1] * R[3 * j + 1] + ks[3 * i + 2] * R[3 * j + 2];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      s[9 + j] = R[3 * j + 2];
      s[12 + j] = tv[(f * V + tid) * 3 + j];
    }
  }
  if (tid >= 128 && tid < 137) cam[9 + tid - 128] = Rm[fa * 9 + tid - 128];
  if (tid >= 137 && tid < 140) cam[18 + tid - 137] = tv[fa * 3 + tid - 137];
  if (tid == 192) scene_kinv(Km + f * 9, sx, sy, cam, nullptr);
  __syncthreads();

  const int tiles_x = (W + 7) >> 3, tiles_y = (H + 7) >> 3;
  const long tile = (long)blockIdx.x * 4 + wave;
  const int ty = (int)(tile / tiles_x), tx = (int)(tile - (long)ty * tiles_x);
  const int py = ty * 8 + (lane >> 3), px = tx * 8 + (lane & 7);
  const bool live = ty < tiles_y && px < W && py < H;
  const long HW = (long)H * W, pix = (long)py * W + px;

  // the target side, once: X, the pixel's colours, the neighbour test
  bool hit = false, smooth = true;
  double X[3] = {0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
  if (live) {
    const float* dp = depth + fa * HW;
    const float Df = dp[pix];
    hit = __builtin_isfinite(Df);
    if (hit) {
      const double D = (double)Df, lim = tol * D;
      double d[3];
      scene_dir(cam, cam + 9, px + 0.5, py + 0.5, d);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        X[k] = cam[18 + k] + D * d[k];
        g[k] = (double)img[(fa * 3 + k) * HW + pix];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int nx = px + (k == 0 ? -1 : k == 1 ? 1 : 0), ny = py + (k == 2 ? -1 : k == 3 ? 1 : 0);
        if (nx < 0 || nx >= W || ny < 0 || ny >= H) continue;
        const float Dn = dp[(long)ny * W + nx];
        smooth = smooth && __builtin_isfinite(Dn) && fabs((double)Dn - D) <= lim;
      }
    }
  }

#pragma unroll 1
  for (int b = 0; b < V; ++b) {
    int klass = b == a ? -1 : 0;
    double s4 = 0.0, s5 = 0.0, s6 = 0.0;
    if (b != a && hit) {
      klass = 1;
      const double* s = src[b];
      const double e0 = X[0] - s[12], e1 = X[1] - s[13], e2 = X[2] - s[14];
      const double dist = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
      const double cz = s[9] * e0 + s[10] * e1 + s[11] * e2;
      const double k0 = s[0] * e0 + s[1] * e1 + s[2] * e2;
      const double k1 = s[3] * e0 + s[4] * e1 + s[5] * e2;
      const double k2 = s[6] * e0 + s[7] * e1 + s[8] * e2;
      const double u = k0 / k2, v = k1 / k2;
      const double x0 = floor(u - 0.5), y0 = floor(v - 0.5);
      const bool inside = x0 >= 0.0 && x0 + 1.0 <= (double)(W - 1) && y0 >= 0.0 && y0 + 1.0 <= (double)(H - 1);
      if (cz > 0.0 && inside) {
        const int ix = (int)x0, iy = (int)y0;            // inside: 0 <= ix <= W - 2, 0 <= iy <= H - 2
        const double fx = (u - 0.5) - x0, fy = (v - 0.5) - y0;
        const long o = (long)iy * W + ix;
        const float* sp = depth + (f * V + b) * HW + o;
        const double q00 = (double)sp[0], q01 = (double)sp[1], q10 = (double)sp[W], q11 = (double)sp[W + 1];
        const double qn = fy >= 0.5 ? (fx >= 0.5 ? q11 : q10) : (fx >= 0.5 ? q01 : q00);
        const double lim = tol * dist;
        if (__builtin_isfinite(qn) && fabs(dist - qn) <= lim) {
          klass = 2;
          const double w00 = (1.0 - fx) * (1.0 - fy), w01 = fx * (1.0 - fy), w10 = (1.0 - fx) * fy, w11 = fx * fy;
          const float* sc = img + (f * V + b) * 3 * HW + o;
#pragma unroll
          for (int c = 0; c < 3; ++c, sc += HW) {
            const double warp =
                w00 * (double)sc[0] + w01 * (double)sc[1] + w10 * (double)sc[W] + w11 * (double)sc[W + 1];
            const double r = (g[c] - warp) * 0.5;
            s4 += r * r;
          }
          const bool flat = __builtin_isfinite(q00) && fabs(dist - q00) <= lim && __builtin_isfinite(q01) &&
                            fabs(dist - q01) <= lim && __builtin_isfinite(q10) && fabs(dist - q10) <= lim &&
                            __builtin_isfinite(q11) && fabs(dist - q11) <= lim;
          if (flat && smooth) {
            klass = 3;
            s5 = s4;
            s6 = fabs(dist - (w00 * q00 + w01 * q01 + w10 * q10 + w11 * q11));
          }
        }
      }
    }
    if (CLS && live) cls[(fa * V + b) * HW + pix] = klass;
    // the wave's row: ballots for the counts, the shuffle tree for the sums
    const unsigned long long m0 = __ballot(live && klass == 0), m1 = __ballot(live && klass == 1),
                             m2 = __ballot(live && klass >= 2), m3 = __ballot(live && klass == 3);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      s4 += __shfl_down(s4, o, 64);
      s5 += __shfl_down(s5, o, 64);
      s6 += __shfl_down(s6, o, 64);
    }
    if (lane == 0) {
      cnt[b][wave][0] = __popcll(m0);
      cnt[b][wave][1] = __popcll(m1);
      cnt[b][wave][2] = __popcll(m2);
      cnt[b][wave][3] = __popcll(m3);
      red[b][wave][0] = s4;
      red[b][wave][1] = s5;
      red[b][wave][2] = s6;
    }
  }
  __syncthreads();
  // the block's rows: the 4 waves in ascending order
  for (int i = tid; i < V * DC_STATS; i += 256) {
    const int b = i / DC_STATS, k = i - b * DC_STATS;
    double x;
    if (k < 4)
      x = (double)(((cnt[b][0][k] + cnt[b][1][k]) + cnt[b][2][k]) + cnt[b][3][k]);
    else
      x = ((red[b][0][k - 4] + red[b][1][k - 4]) + red[b][2][k - 4]) + red[b][3][k - 4];
    part[((fa * V + b) * gridDim.x + blockIdx.x) * DC_STATS + k] = x;
  }
}

// One thread per (field, target, source, k): the blocks' partial rows in ascending order.
__global__ __launch_bounds__(256) void depth_consistency_final_k(const double* __restrict__ part, int blocks, long n,
                                                                 double* __restrict__ stats) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long row = i / DC_STATS;
  const int k = (int)(i - row * DC_STATS);
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s += part[(row * blocks + b) * DC_STATS + k];
  stats[i] = s;
}

// Blocks per (field, target view): four 8 x 8 tiles each (0: beyond the launch grid).
long depth_consistency_blocks(int H, int W) {
  if (H <= 0 || W <= 0 || (long)H * W > 0x7fffffffL) return 0;
  const long nb = ((((long)W + 7) / 8) * (((long)H + 7) / 8) + 3) / 4;
  return nb <= 0x7fffffffL ? nb : 0;
}
}  // namespace

// The blocks of a (field, target view) of d3d_depth_consistency: `part` holds
// F V V times that many rows of 7 (-1: bad arguments).
D3D_API int d3d_depth_consistency_blocks(int H, int W) {
  const long nb = depth_consistency_blocks(H, W);
  return nb > 0 ? (int)nb : -1;
}

// depth fp32 [F,V,H,W]; img fp32 [F,V,3,H,W]; Km fp64 [F,3,3], the intrinsics
// of the ref x ref image (ref = 0: of the H x W image); Rm fp64 [F,V,3,3]
// cam-to-world; tv fp64 [F,V,3]; 1 <= V <= 64; tol > 0; part fp64
// [F,V,V,d3d_depth_consistency_blocks(H, W),7] workspace; stats fp64 [F,V,V,7];
// cls int32 [F,V,V,H,W] or null.
D3D_API int d3d_depth_consistency(const float* depth, const float* img, const double* Km, const double* Rm,
                                  const double* tv, int F, int V, int H, int W, double tol, int ref, double* part,
                                  double* stats, int* cls, hipStream_t st) {
  const long nb = depth_consistency_blocks(H, W);
  if (F <= 0 || V < 1 || V > DC_MAXV || nb <= 0 || !(tol > 0.0) || !(tol < 1e300) || ref < 0 || depth == nullptr ||
      img == nullptr || Km == nullptr || Rm == nullptr || tv == nullptr || part == nullptr || stats == nullptr)
    return (int)hipErrorInvalidValue;
  const double sx = ref > 0 ? (double)W / ref : 1.0, sy = ref > 0 ? (double)H / ref : 1.0;
  for (int f0 = 0; f0 < F; f0 += 65535) {      // grid.z limit
    const dim3 gd((unsigned)nb, (unsigned)V, (unsigned)(F - f0 < 65535 ? F - f0 : 65535));
    if (cls != nullptr)
      hipLaunchKernelGGL(depth_consistency_k<true>, gd, dim3(256), 0, st, depth, img, Km, Rm, tv, part, cls, V, H, W,
                         tol, sx, sy, f0);
    else
      hipLaunchKernelGGL(depth_consistency_k<false>, gd, dim3(256), 0, st, depth, img, Km, Rm, tv, part, cls, V, H, W,
                         tol, sx, sy, f0);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  const long n = (long)F * V * V * DC_STATS;
  hipLaunchKernelGGL(depth_consistency_final_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, (int)nb, n,
                     stats);
  return (int)hipGetLastError();
}
