// Field geometry (ops.field_geometry; the torch form and the rule's oracle is
// torch_impl.field_geometry): what surface a fitted voxel radiance field
// implies -- opacity, depth and normal along every pixel's ray -- and, for a
// procedural object, its score against the true surface of the scene table.
//
// Inputs, per field f < F and view v < V: grid fp32 [F,G,G,G,4] (field.hip's
// layout; only the raw_sigma channel is read), K fp64 [F,3,3], R fp64
// [F,V,3,3] cam-to-world, t fp64 [F,V,3], table fp64 [F,6,16] (scene.hip's
// layout) or none.
//
// The ray of pixel (px, py) goes through the pixel centre (px + 1/2, py + 1/2)
// by scene.hip's rule in fp64: o = t, d = R normalize(Kinv [u, v, 1]), Kinv
// the inverse of diag(W / ref, H / ref, 1) K (ref = 0: of K itself).  The truth
// is traced along the fp64 d; the field is walked along o and d rounded once
// to fp32.
//
// The walk is field.hip's, unchanged: the slab cut of the cube
// [-bound, bound]^3, S equal steps at t_i = t0 + (i + 1/2) delta, the cell and
// the trilinear weights of field_locate, and
//   raw_i = sum_k w_k s_k over the cell's corners k = (dz, dy, dx) ascending,
//           w_k = (wz wy) wx, s_k the corner's raw_sigma
//   alpha_i = -expm1(-softplus(raw_i) delta), T_0 = 1, T_{i+1} = T_i (1 - alpha_i),
//   w_i = T_i alpha_i.
// The same eight corner values give the analytic gradient of the trilinear
// interpolant in world units, scale = (G - 1) / (2 bound):
//   grad_i = scale (sum_k +-(wz wy) s_k, sum_k +-(wz wx) s_k, sum_k +-(wy wx) s_k),
// the sign + for the corners on the +1 side of that axis.
//
// The field's values at a pixel:
//   opacity  A = sum_i w_i                      (0 for a ray that misses the cube)
//   the field "hits" where A > 1/2: the mask P
//   depth    D = (sum_i w_i t_i) / A on P, +inf elsewhere; |d| = 1, so D is a
//            distance along the ray, comparable with Hit.t
//   normal   g = sum_i w_i grad_i;  n = -g / |g| on P where |g| > 0, else 0.
// maps fp32 [F,V,5,H,W]: the planes A, D, n_x, n_y, n_z.
//
// The truth, with a table: scene_nearest on the same pixel-centre ray gives t*
// and the hit mask M (prim >= 0); n* = normalize(A^T n_local) as scene_shade
// forms it.  The score row of a (field, view), sums over its H W pixels in
// fp64 of the fp32 field values:
//   0: sum M        1: sum P        2: sum M&P
//   3: sum_{M&P} |D - t*|           4: sum_{M&P} (D - t*)^2
//   5: sum_{M&P} (1 - n . n*)       6: sum_all (A - M)^2, a silhouette error
//                                      that has no threshold.
//
// Work split: a wave owns an 8 x 8 pixel tile, so that its lanes' gathers fall
// into neighbouring cells; a 256-thread block owns four consecutive tiles (row
// order) of one (field, view); launch grid (ceil(tiles / 4), V, F), the last
// two chunked to the grid limits.  The view's camera (Kinv, R) and the field's
// table, each centre moved into its primitive's frame by scene_origin, are
// staged in LDS once per block; the slot loop of scene_nearest reads them
// through wave-uniform addresses.  A lane walks its ray in registers (fp32;
// the eight raw_sigma loads of a sample serve the opacity and the gradient),
// then traces the truth (fp64) and forms its seven terms.  They are summed in
// a fixed order, as field_block_sum does: the wave's shuffle tree, the 4 waves
// ascending; the block's partial row goes to part [F,V,blocks,7], and
// field_geom_final_k adds the blocks of a row in ascending order.  No atomics;
// a (field, view) row reads only its own inputs, so a batched call equals the
// single calls bit for bit and the op is bitwise reproducible.  The launcher
// takes pointers and constants and never synchronises: it can be captured.
//
// Built with field.hip's flags (packed fp32 ops off).  The ray cut, the sample
// positions, the cells and the weights are field_ray.h's own functions; the
// gather below reads only the raw_sigma word of each corner (4 bytes of the
// 16) and forms raw_i by field_gather's expression.
#include "field_ray.h"
#include "scene_trace.h"

#define FG_ROWS 7
#define FG_PLANES 5

namespace {

// One sample's raw_sigma and the gradient of the cell's trilinear interpolant
// in grid units (x, y, z) from its eight corner values.
__device__ __forceinline__ float field_geom_gather(const float* __restrict__ grid, const FieldCell& c, int G,
                                                   float (&gr)[3]) {
  float raw = 0.0f;
  gr[0] = gr[1] = gr[2] = 0.0f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float s = grid[field_corner_off(c, k, G) + 3];
    const float wx = (k & 1) ? c.f[0] : 1.0f - c.f[0];
    const float wy = (k & 2) ? c.f[1] : 1.0f - c.f[1];
    const float wz = (k & 4) ? c.f[2] : 1.0f - c.f[2];
    raw += ((wz * wy) * wx) * s;
    gr[0] += (wz * wy) * ((k & 1) ? s : -s);
    gr[1] += (wz * wx) * ((k & 2) ? s : -s);
    gr[2] += (wy * wx) * ((k & 4) ? s : -s);
  }
  return raw;
}

// TRUTH: score against the table (S, part); otherwise maps only.
template <bool TRUTH>
__global__ __launch_bounds__(256) void field_geom_k(const float* __restrict__ grid, const double* __restrict__ Km,
                                                    const double* __restrict__ Rm, const double* __restrict__ tv,
                                                    const double* __restrict__ table, float* __restrict__ maps,
                                                    double* __restrict__ part, int V, int H, int W, int S, int G,
                                                    float bound, float scale, double sx, double sy, int f0, int v0) {
  __shared__ double Sc[SC_SLOTS][SC_WORDS];
  __shared__ double cam[18];                   // Kinv [9], R [9]
  __shared__ double red[4][FG_ROWS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long f = f0 + (long)blockIdx.z, fv = f * V + v0 + blockIdx.y;
  const double* T = tv + fv * 3;
  if (TRUTH && tid < SC_ROW) Sc[tid / SC_WORDS][tid % SC_WORDS] = table[f * SC_ROW + tid];
  if (tid >= 128 && tid < 137) cam[9 + tid - 128] = Rm[fv * 9 + tid - 128];
  if (tid == 192) scene_kinv(Km + f * 9, sx, sy, cam, nullptr);
  __syncthreads();
  if (TRUTH && tid < SC_SLOTS) scene_origin(Sc[tid], T);      // centre -> the origin in the primitive's frame
  __syncthreads();

  const int tiles_x = (W + 7) >> 3, tiles_y = (H + 7) >> 3;
  const long tile = (long)blockIdx.x * 4 + wave;
  const int ty = (int)(tile / tiles_x), tx = (int)(tile - (long)ty * tiles_x);
  const int py = ty * 8 + (lane >> 3), px = tx * 8 + (lane & 7);
  const bool live = ty < tiles_y && px < W && py < H;
  const long HW = (long)H * W;

  double row[FG_ROWS];
#pragma unroll
  for (int k = 0; k < FG_ROWS; ++k) row[k] = 0.0;
  if (live) {
    double d[3];
    scene_dir(cam, cam + 9, px + 0.5, py + 0.5, d);
    const float o32[3] = {(float)T[0], (float)T[1], (float)T[2]};
    const float d32[3] = {(float)d[0], (float)d[1], (float)d[2]};
    const FieldRay q = field_load_ray(o32, d32, 0, S, bound);
    float A = 0.0f, Dn = 0.0f, g[3] = {0.0f, 0.0f, 0.0f};
    if (q.hit) {
      const float* gf = grid + f * ((long)G * G * G * 4);
      float Tr = 1.0f;
      for (int i = 0; i < S; ++i) {
        const FieldCell cell = field_locate(q, i, G, bound, scale);
        float gr[3];
        const float raw = field_geom_gather(gf, cell, G, gr);
        const float alpha = -expm1f(-field_softplus(raw) * q.delta);
        const float w = Tr * alpha;
        A += w;
        Dn += w * (q.t0 + ((float)i + 0.5f) * q.delta);
#pragma unroll
        for (int a = 0; a < 3; ++a) g[a] += w * (gr[a] * scale);
        Tr *= 1.0f - alpha;
      }
    }
    const bool P = q.hit && A > 0.5f;
    const float D = P ? Dn / A : __builtin_inff();
    const float gn = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
    float n[3] = {0.0f, 0.0f, 0.0f};
    if (P && gn > 0.0f) {
#pragma unroll
      for (int a = 0; a < 3; ++a) n[a] = -g[a] / gn;
    }
    if (maps != nullptr) {
      float* m = maps + fv * FG_PLANES * HW + (long)py * W + px;
      m[0] = A;
      m[HW] = D;
      m[2 * HW] = n[0];
      m[3 * HW] = n[1];
      m[4 * HW] = n[2];
    }
    if (TRUTH) {
      double nl[3];
      const Hit h = scene_nearest(Sc, d, nl);
      const bool M = h.prim >= 0;
      row[0] = M ? 1.0 : 0.0;
      row[1] = P ? 1.0 : 0.0;
      if (M && P) {
        const double* s = Sc[h.prim];
        double w0 = s[0] * nl[0] + s[3] * nl[1] + s[6] * nl[2];      // A^T n_local
        double w1 = s[1] * nl[0] + s[4] * nl[1] + s[7] * nl[2];
        double w2 = s[2] * nl[0] + s[5] * nl[1] + s[8] * nl[2];
        const double wn = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
        w0 /= wn;
        w1 /= wn;
        w2 /= wn;
        const double df = (double)D - h.t;
        row[2] = 1.0;
        row[3] = fabs(df);
        row[4] = df * df;
        row[5] = 1.0 - (((double)n[0] * w0 + (double)n[1] * w1) + (double)n[2] * w2);
      }
      const double sil = (double)A - row[0];
      row[6] = sil * sil;
    }
  }
  if (TRUTH) {
    // the wave's shuffle tree, then the 4 waves in ascending order
#pragma unroll
    for (int k = 0; k < FG_ROWS; ++k) {
      double x = row[k];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
      if (lane == 0) red[wave][k] = x;
    }
    __syncthreads();
    if (tid < FG_ROWS)
      part[(fv * gridDim.x + blockIdx.x) * FG_ROWS + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  }
}

// One thread per (field, view, k): the blocks' partial rows in ascending order.
__global__ __launch_bounds__(256) void field_geom_final_k(const double* __restrict__ part, int blocks, long n,
                                                          double* __restrict__ scores) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long fv = i / FG_ROWS;
  const int k = (int)(i - fv * FG_ROWS);
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s += part[(fv * blocks + b) * FG_ROWS + k];
  scores[i] = s;
}

// Blocks per (field, view): four 8 x 8 tiles each (0: beyond the launch grid).
long field_geom_blocks(int H, int W) {
  if (H <= 0 || W <= 0) return 0;
  const long nb = ((((long)W + 7) / 8) * (((long)H + 7) / 8) + 3) / 4;
  return nb <= 0x7fffffffL ? nb : 0;
}
}  // namespace

// The blocks of a (field, view) of d3d_field_geometry: `part` holds F V times that many rows of 7 (-1: bad arguments).
D3D_API int d3d_field_geometry_blocks(int H, int W) {
  const long nb = field_geom_blocks(H, W);
  return nb > 0 ? (int)nb : -1;
}

// grid fp32 [F,G,G,G,4]; Km fp64 [F,3,3], the intrinsics of the ref x ref image
// (ref = 0: of the H x W image); Rm fp64 [F,V,3,3] cam-to-world; tv fp64
// [F,V,3]; table fp64 [F,6,16] or null; maps fp32 [F,V,5,H,W] or null (not both
// null); with a table, part fp64 [F,V,d3d_field_geometry_blocks(H, W),7]
// workspace and scores fp64 [F,V,7].
D3D_API int d3d_field_geometry(const float* grid, const double* Km, const double* Rm, const double* tv,
                               const double* table, int F, int V, int H, int W, int S, int G, double bound, int ref,
                               float* maps, double* part, double* scores, hipStream_t st) {
  const long nb = field_geom_blocks(H, W);
  if (F <= 0 || V <= 0 || nb <= 0 || S < 1 || G < 2 || G > 4096 || !(bound > 0.0) || !(bound < 1e30) || ref < 0 ||
      grid == nullptr || Km == nullptr || Rm == nullptr || tv == nullptr || (table == nullptr && maps == nullptr) ||
      (table != nullptr && (part == nullptr || scores == nullptr)))
    return (int)hipErrorInvalidValue;
  const double sx = ref > 0 ? (double)W / ref : 1.0, sy = ref > 0 ? (double)H / ref : 1.0;
  const float scale = (float)((G - 1) / (2.0 * bound));
  for (int f0 = 0; f0 < F; f0 += 65535)        // grid.z and grid.y limits
    for (int v0 = 0; v0 < V; v0 += 65535) {
      const dim3 gd((unsigned)nb, (unsigned)(V - v0 < 65535 ? V - v0 : 65535), (unsigned)(F - f0 < 65535 ? F - f0 : 65535));
      if (table != nullptr)
        hipLaunchKernelGGL(field_geom_k<true>, gd, dim3(256), 0, st, grid, Km, Rm, tv, table, maps, part, V, H, W, S,
                           G, (float)bound, scale, sx, sy, f0, v0);
      else
        hipLaunchKernelGGL(field_geom_k<false>, gd, dim3(256), 0, st, grid, Km, Rm, tv, table, maps, part, V, H, W, S,
                           G, (float)bound, scale, sx, sy, f0, v0);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return (int)e;
    }
  if (table == nullptr) return (int)hipSuccess;
  const long n = (long)F * V * FG_ROWS;
  hipLaunchKernelGGL(field_geom_final_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, (int)nb, n, scores);
  return (int)hipGetLastError();
}
