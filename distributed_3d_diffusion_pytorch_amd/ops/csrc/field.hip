// Radiance-field consistency (ops.field_render, ops.field_loss_grad; the torch
// form and the rule's oracle are torch_impl.field_render / field_loss_grad): a
// dense voxel radiance field rendered by fixed-step quadrature, its squared
// error against target colours, and the gradient of that error on the grid --
// the fused forward and backward of one iteration of a field fit.  The per-ray
// device code lives in field_ray.h, which field_fit.hip (the batched fit)
// includes as well.
//
// The field: grid fp32 [G,G,G,4], contiguous, indexed [iz,iy,ix,c], channels
// (raw_r, raw_g, raw_b, raw_sigma); node j of an axis lies at
// -bound + 2 bound j / (G - 1); G >= 2, bound > 0.
//
// A ray (o, d), fp32 [3] each, d of unit length, is cut with the cube
// [-bound, bound]^3 by slabs, starting from t0 = 0 and a finite far end: per
// axis, a direction component of exactly 0 takes a branch of its own -- the
// ray is inside that slab for all t iff |o| <= bound, else it misses -- and any
// other component narrows [t0, t1] to [min, max] of (-+bound - o) / d.  A ray
// misses when t1 <= t0; then C = bg.  Otherwise delta = (t1 - t0) / S and the
// samples lie at t_i = t0 + (i + 1/2) delta, i < S: no jitter, no early exit.
//
// A sample: the point o + t_i d in continuous grid coordinates
// (p + bound) (G - 1) / (2 bound), clamped to [0, G - 1]; the cell is
// min(floor, G - 2) per axis, and all 4 channels are interpolated trilinearly,
// sum_k w_k v_k over the corners k = (dz, dy, dx) ascending, w_k = (wz wy) wx.
//   sigma_i = max(raw, 0) + log1p(exp(-|raw|))     softplus, overflow-safe
//   c_i     = 1 / (1 + exp(-raw_rgb))              sigmoid
//   alpha_i = -expm1(-sigma_i delta)
//   T_0 = 1, T_{i+1} = T_i (1 - alpha_i), w_i = T_i alpha_i
//   C = sum_i w_i c_i + T_S bg, bg = 1 (white), on the [0, 1] scale.
// The loss against targets y fp32 [R,3] in [-1, 1], scored as y01 = (y + 1) / 2:
// L = sum_rays sum_ch (C - y01)^2 -- a sum; the caller divides.
//
// The gradient needs no stored per-sample state and no reverse walk.  With
// C<=i = sum_{j<=i} w_j c_j:
//   dC/dsigma_i = delta (T_{i+1} c_i - (C - C<=i)),   dC/dc_i = w_i,
// so a ray is two forward walks: the first gives C, the second recomputes each
// sample, forms g = 2 (C - y01) and the sample's four raw-channel derivatives
// (through softplus' = sigmoid(raw_sigma) and sigmoid' = c (1 - c)) and hands
// them to the sample's eight corners by the trilinear weights.
//
// One thread per ray, 256 per block; both walks live in registers, every
// corner is one 16-byte load of the four channels (no LDS but the 32 bytes of
// the loss sum, no scratch).  With width = W > 0 the rays are the pixels of
// images of width W in row order (R = rows W), and a wave takes an 8 x 8 pixel
// tile, so that its lanes' gathers fall into neighbouring cells; with W = 0
// lane l of wave w takes ray 64 w + l.  Ray r reads row r of o, d and y only.
//
// The gradient is bitwise reproducible: contributions are added to a 64-bit
// fixed-point accumulator acc [G^3 4] (scale 2^36, round to nearest) with
// integer atomics -- integer addition is associative, so the arrival order
// does not matter -- and field_convert_k turns it into fp32 and clears it for
// the next call (the accumulator is zero between calls).  Range: one
// contribution is at most M = 6 max(1, delta_max) in magnitude (|g| <= 2 on 3
// channels, |dC/dsigma| <= delta, the other factors <= 1; delta_max =
// 2 sqrt(3) bound / S, the cube's diagonal) and a node receives at most 8 R S
// of them, so |acc| <= 8 R S M 2^36; the launcher refuses R S M > 2^23, which
// keeps that below 2^62 (at bound = 1 and S >= 4: R S <= 1398101).  The loss is
// summed in a fixed order: fp64 per thread, the wave's shuffle tree, the
// block's 4 waves ascending into part [blocks], then field_loss_final_k over
// the blocks ascending, as in ensemble.hip.
//
// Numerics: fp32 with the accurate expf / log1pf / expm1f (the fast forms'
// error grows with |raw|), the squared error and its sums in fp64.
#include "field_ray.h"

namespace {

// The ray of thread slot s: linear, or the 8 x 8 pixel tiles of rows x W images.
__device__ __forceinline__ long field_ray(long s, long R, int W, long rows) {
  if (W <= 0) return s < R ? s : -1;
  const long tiles_x = (W + 7) >> 3;
  const long tile = s >> 6;
  const int lane = (int)(s & 63);
  const long ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const long y = ty * 8 + (lane >> 3), x = tx * 8 + (lane & 7);
  return (x < W && y < rows) ? y * W + x : -1;
}

__global__ __launch_bounds__(256) void field_render_k(const float* __restrict__ grid, const float* __restrict__ ro,
                                                      const float* __restrict__ rd, float* __restrict__ out, long R,
                                                      int S, int G, float bound, float scale, int W, long rows) {
  const long r = field_ray((long)blockIdx.x * 256 + threadIdx.x, R, W, rows);
  if (r < 0) return;
  const FieldRay q = field_load_ray(ro, rd, r, S, bound);
  float C[3] = {1.0f, 1.0f, 1.0f};
  if (q.hit) field_walk(grid, q, S, G, bound, scale, C);
#pragma unroll
  for (int e = 0; e < 3; ++e) out[r * 3 + e] = C[e];
}

__global__ __launch_bounds__(256) void field_loss_grad_k(const float* __restrict__ grid, const float* __restrict__ ro,
                                                         const float* __restrict__ rd, const float* __restrict__ tgt,
                                                         unsigned long long* __restrict__ acc,
                                                         double* __restrict__ part, long R, int S, int G, float bound,
                                                         float scale, int W, long rows) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const long r = field_ray((long)blockIdx.x * 256 + tid, R, W, rows);
  double loss = 0.0;
  if (r >= 0) field_ray_loss_grad(loss, grid,ro, rd, tgt, acc, r, S, G, bound, scale);
  loss = field_block_sum(loss, red, tid);
  if (tid == 0) part[blockIdx.x] = loss;
}

// One thread: the blocks' partial sums in ascending order.
__global__ void field_loss_final_k(const double* __restrict__ part, int blocks, double* __restrict__ loss) {
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s += part[b];
  *loss = s;
}

// Thread slots of R rays (whole 8 x 8 tiles with a width), or -1 for bad arguments.
long field_slots(long R, int W) {
  if (R <= 0 || W < 0 || (W > 0 && R % W != 0)) return -1;
  if (W == 0) return R;
  return (((long)W + 7) / 8) * ((R / W + 7) / 8) * 64;
}

bool field_args_ok(int S, int G, double bound, long slots) {
  return S >= 1 && G >= 2 && G <= 4096 && bound > 0.0 && bound < 1e30 && slots > 0 &&
         (slots + 255) / 256 <= 0x7fffffffL;
}
}  // namespace

// The blocks of a d3d_field_loss_grad launch = the length of its `part` workspace (-1: bad arguments).
D3D_API int d3d_field_blocks(int R, int W) {
  const long slots = field_slots(R, W);
  return slots <= 0 ? -1 : (int)((slots + 255) / 256);
}

// grid fp32 [G,G,G,4]; ro, rd fp32 [R,3]; out fp32 [R,3].
D3D_API int d3d_field_render(const float* grid, const float* ro, const float* rd, float* out, int R, int S, int G,
                             double bound, int W, hipStream_t st) {
  const long slots = field_slots(R, W);
  if (!field_args_ok(S, G, bound, slots) || grid == nullptr || ro == nullptr || rd == nullptr || out == nullptr)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(field_render_k, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, grid, ro, rd, out,
                     (long)R, S, G, (float)bound, (float)((G - 1) / (2.0 * bound)), W, W > 0 ? (long)R / W : 0L);
  return (int)hipGetLastError();
}

// tgt fp32 [R,3]; acc int64 [G^3 4], zero on entry and on return; part fp64
// [d3d_field_blocks(R, W)] workspace; loss fp64 [1]; grad fp32 [G,G,G,4].
D3D_API int d3d_field_loss_grad(const float* grid, const float* ro, const float* rd, const float* tgt, void* acc,
                                double* part, double* loss, float* grad, int R, int S, int G, double bound, int W,
                                hipStream_t st) {
  const long slots = field_slots(R, W);
  if (!field_args_ok(S, G, bound, slots) || grid == nullptr || ro == nullptr || rd == nullptr || tgt == nullptr ||
      acc == nullptr || part == nullptr || loss == nullptr || grad == nullptr)
    return (int)hipErrorInvalidValue;
  if (!field_fix_ok(R, S, bound))                                        // beyond the fixed-point range
    return (int)hipErrorInvalidValue;
  const int blocks = (int)((slots + 255) / 256);
  unsigned long long* a = reinterpret_cast<unsigned long long*>(acc);
  hipLaunchKernelGGL(field_loss_grad_k, dim3((unsigned)blocks), dim3(256), 0, st, grid, ro, rd, tgt, a, part, (long)R,
                     S, G, (float)bound, (float)((G - 1) / (2.0 * bound)), W, W > 0 ? (long)R / W : 0L);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(field_loss_final_k, dim3(1), dim3(1), 0, st, part, blocks, loss);
  e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  const long n = (long)G * G * G * 4;
  hipLaunchKernelGGL(field_convert_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, grad, n);
  return (int)hipGetLastError();
}
