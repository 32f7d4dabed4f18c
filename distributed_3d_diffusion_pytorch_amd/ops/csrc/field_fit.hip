// Batched radiance-field fits (ops.field_batch_loss_grad, ops.field_adam_tv;
// the torch forms and the rule's oracle are torch_impl.field_batch_loss_grad /
// field_adam_tv): one iteration of F independent field fits is two ops -- the
// data term's loss and gradient over rays the kernel draws itself, and Adam
// with a smoothness term on the grid.  engine.fit_fields is the loop.
//
// The draw.  Field f has N stored rays, rays_o, rays_d and target fp32
// [F,N,3].  Iteration `it` of a fit with n rays per iteration gives thread
// slot s < n the ray j = hash_u32(seed, s + it n) % N (common.h's counter
// hash, 64-bit index): with replacement, unsorted, and the same j for every
// field -- the fields are different objects, and a batched fit is F single
// fits.  The draw is integer arithmetic, so the kernel and the torch form read
// identical rows.
//
// The data term is field.hip's rule unchanged, per field: the summed squared
// error of the n drawn rays and its gradient on that field's grid, through the
// per-ray device code of field_ray.h into slice f of the 64-bit fixed-point
// accumulator [F, G^3 4] (bitwise reproducible; the same range check per
// field, n S M <= 2^23).  Field f reads row f of every input only.  The loss
// is summed per field in a fixed order: fp64 per thread, the wave's shuffle
// tree, the block's 4 waves ascending into part [F, blocks], then one thread
// per field over the blocks ascending into loss [F].  The convert-and-clear
// pass of field.hip runs over F G^3 4 elements.
//
// The smoothness term acts on the raw grid values, per field:
//   L_tv = (1 / G^3) sum_c lambda_c sum_edges (v_a,c - v_b,c)^2
// over the axis-aligned neighbour pairs inside the grid -- no wrap, no ghost
// nodes: a face node has 5 neighbours, an edge node 4, a corner node 3.
// lambda_c is tv_rgb for c < 3 and tv_sigma for c = 3.  Its gradient at a node
// is (2 lambda_c / G^3) sum_neighbours (v - v_n), the neighbours taken in the
// order x-1, x+1, y-1, y+1, z-1, z+1.
//
// The update is Adam in torch's arithmetic order (as adam.hip) on
// g = grad_scale grad + grad L_tv:
//   m <- m + (1 - b1) (g - m),  v <- v b2 + (1 - b2) g g,
//   p <- p - (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps)),
// bc1 = 1 - b1^step, bc2 = 1 - b2^step, step counted from 1.  m and v are
// updated in place; the new grid goes to a second buffer: a tile's neighbours
// belong to other workgroups that may already have stepped, so an in-place
// grid would make the result depend on scheduling.  The caller ping-pongs.
//
// field_fit_grad_k: launch grid (ceil(n / 256), F), one thread per drawn ray.
// field_adam_tv_k: a workgroup of 256 threads owns a tile of TX x TY x TZ =
// 8 x 8 x 8 nodes of one field (launch grid (tiles, F)).  It stages the tile
// and a one-node halo, 10^3 nodes of 16 bytes = 16000 bytes, in LDS with one
// 16-byte load per node; a halo node outside the grid is absent: its slot is
// zeroed and the node that would read it skips the term (the test is on the
// node's coordinates, never on the slot's value).  Thread t takes the nodes
// (x, y, z) and (x, y, z + 4) of the tile, x = t % 8, y = t / 8 % 8,
// z = t / 64: a wave is one 8 x 8 plane of the tile, its 16-byte global
// accesses are 8 runs of 128 bytes, and its LDS reads step 16 bytes along x.
// The six neighbour reads of a node are 16-byte LDS reads; grad, exp_avg and
// exp_avg_sq are one 16-byte global load each.  No atomics, no scratch.
#include "field_ray.h"

#ifndef FIELD_TV_TX
#define FIELD_TV_TX 8
#define FIELD_TV_TY 8
#define FIELD_TV_TZ 8
#endif

namespace {
constexpr int TX = FIELD_TV_TX, TY = FIELD_TV_TY, TZ = FIELD_TV_TZ;
constexpr int HX = TX + 2, HY = TY + 2, HZ = TZ + 2;
constexpr int TILE_NODES = TX * TY * TZ, HALO_NODES = HX * HY * HZ;
static_assert(TILE_NODES % 256 == 0, "a thread takes a whole number of nodes");

__global__ __launch_bounds__(256) void field_fit_grad_k(const float* __restrict__ grid, const float* __restrict__ ro,
                                                        const float* __restrict__ rd, const float* __restrict__ tgt,
                                                        unsigned long long* __restrict__ acc,
                                                        double* __restrict__ part, long N, int n, unsigned long long it,
                                                        unsigned long long seed, int S, int G, float bound,
                                                        float scale) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const long f = blockIdx.y, s = (long)blockIdx.x * 256 + tid;
  const long gsz = (long)G * G * G * 4, rsz = N * 3;
  double loss = 0.0;
  if (s < n) {
    const long j = (long)(hash_u32(seed, (unsigned long long)s + it * (unsigned long long)n) % (unsigned long long)N);
    field_ray_loss_grad(loss, grid + f * gsz, ro + f * rsz, rd + f * rsz, tgt + f * rsz, acc + f * gsz, j, S, G,
                        bound, scale);
  }
  loss = field_block_sum(loss, red, tid);
  if (tid == 0) part[f * gridDim.x + blockIdx.x] = loss;
}

// One thread per field: its blocks' partial sums in ascending order.
__global__ __launch_bounds__(64) void field_fit_loss_k(const double* __restrict__ part, int blocks, int F,
                                                       double* __restrict__ loss) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= F) return;
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s += part[(long)f * blocks + b];
  loss[f] = s;
}

struct FieldAdam {
  float omb1, b2, omb2, eps, step_size, inv_bc2, grad_scale, tv_rgb, tv_sigma;     // om*: 1 - beta; tv_*: 2 lambda / G^3
};

__global__ __launch_bounds__(256) void field_adam_tv_k(const float* __restrict__ grid, float* __restrict__ out,
                                                       float* __restrict__ m, float* __restrict__ v,
                                                       const float* __restrict__ grad, int G, int ntx, int nty,
                                                       FieldAdam a) {
  __shared__ f32x4 halo[HALO_NODES];
  const int tid = threadIdx.x;
  const int tile = blockIdx.x;
  const int tx = tile % ntx, ty = (tile / ntx) % nty, tz = tile / (ntx * nty);
  const int x0 = tx * TX, y0 = ty * TY, z0 = tz * TZ;
  const long fbase = (long)blockIdx.y * G * G * G;               // in nodes
  for (int k = tid; k < HALO_NODES; k += 256) {
    const int hx = k % HX, hy = (k / HX) % HY, hz = k / (HX * HY);
    const int gx = x0 + hx - 1, gy = y0 + hy - 1, gz = z0 + hz - 1;
    f32x4 n = {0.0f, 0.0f, 0.0f, 0.0f};                            // absent: never used, see below
    if (gx >= 0 && gx < G && gy >= 0 && gy < G && gz >= 0 && gz < G)
      n = *reinterpret_cast<const f32x4*>(grid + (fbase + ((long)gz * G + gy) * G + gx) * 4);
    halo[k] = n;
  }
  __syncthreads();
  const f32x4 coef = {a.tv_rgb, a.tv_rgb, a.tv_rgb, a.tv_sigma};
#pragma unroll
  for (int q = 0; q < TILE_NODES / 256; ++q) {
    const int l = tid + q * 256;
    const int lx = l % TX, ly = (l / TX) % TY, lz = l / (TX * TY);
    const int gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
    if (gx >= G || gy >= G || gz >= G) continue;
    const int h = ((lz + 1) * HY + (ly + 1)) * HX + (lx + 1);
    const f32x4 c = halo[h];
    f32x4 tv = {0.0f, 0.0f, 0.0f, 0.0f};
    if (gx > 0) tv += c - halo[h - 1];
    if (gx < G - 1) tv += c - halo[h + 1];
    if (gy > 0) tv += c - halo[h - HX];
    if (gy < G - 1) tv += c - halo[h + HX];
    if (gz > 0) tv += c - halo[h - HX * HY];
    if (gz < G - 1) tv += c - halo[h + HX * HY];
    const long i = (fbase + ((long)gz * G + gy) * G + gx) * 4;
    const f32x4 gg = *reinterpret_cast<const f32x4*>(grad + i);
    f32x4 mm = *reinterpret_cast<const f32x4*>(m + i), vv = *reinterpret_cast<const f32x4*>(v + i), pp;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gj = gg[e] * a.grad_scale + coef[e] * tv[e];
      mm[e] = mm[e] + a.omb1 * (gj - mm[e]);
      vv[e] = vv[e] * a.b2 + a.omb2 * gj * gj;
      const float denom = sqrtf(vv[e]) * a.inv_bc2 + a.eps;
      pp[e] = c[e] - a.step_size * (mm[e] / denom);
    }
    *reinterpret_cast<f32x4*>(out + i) = pp;
    *reinterpret_cast<f32x4*>(m + i) = mm;
    *reinterpret_cast<f32x4*>(v + i) = vv;
  }
}

bool fit_dims_ok(int F, int G) { return F >= 1 && F <= 65535 && G >= 2 && G <= 4096; }
}  // namespace

// The blocks per field of a d3d_field_fit_loss_grad launch: `part` holds F times that many doubles.
D3D_API int d3d_field_fit_blocks(int n) { return n <= 0 ? -1 : (n + 255) / 256; }

// grid fp32 [F,G,G,G,4]; ro, rd, tgt fp32 [F,N,3]; acc int64 [F, G^3 4], zero
// on entry and on return; part fp64 [F, d3d_field_fit_blocks(n)] workspace;
// loss fp64 [F]; grad fp32 [F,G,G,G,4].
D3D_API int d3d_field_fit_loss_grad(const float* grid, const float* ro, const float* rd, const float* tgt, void* acc,
                                    double* part, double* loss, float* grad, int F, long N, int n, long it,
                                    unsigned long long seed, int S, int G, double bound, hipStream_t st) {
  if (!fit_dims_ok(F, G) || N < 1 || N > 0x7fffffffL || n < 1 || it < 0 || S < 1 || !(bound > 0.0 && bound < 1e30) ||
      grid == nullptr || ro == nullptr || rd == nullptr || tgt == nullptr || acc == nullptr || part == nullptr ||
      loss == nullptr || grad == nullptr)
    return (int)hipErrorInvalidValue;
  if (!field_fix_ok(n, S, bound))                                        // beyond the fixed-point range, per field
    return (int)hipErrorInvalidValue;
  const int blocks = (n + 255) / 256;
  unsigned long long* a = reinterpret_cast<unsigned long long*>(acc);
  hipLaunchKernelGGL(field_fit_grad_k, dim3((unsigned)blocks, (unsigned)F), dim3(256), 0, st, grid, ro, rd, tgt, a,
                     part, N, n, (unsigned long long)it, seed, S, G, (float)bound, (float)((G - 1) / (2.0 * bound)));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(field_fit_loss_k, dim3((unsigned)((F + 63) / 64)), dim3(64), 0, st, part, blocks, F, loss);
  e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  const long total = (long)F * G * G * G * 4;
  if ((total + 255) / 256 > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(field_convert_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a, grad, total);
  return (int)hipGetLastError();
}

// grid, out, m, v, grad fp32 [F,G,G,G,4]; out must not overlap grid.  step >= 1.
D3D_API int d3d_field_adam_tv(const float* grid, float* out, float* m, float* v, const float* grad, int F, int G,
                              int step, double lr, double b1, double b2, double eps, double grad_scale, double tv_rgb,
                              double tv_sigma, hipStream_t st) {
  if (!fit_dims_ok(F, G) || step < 1 || grid == nullptr || out == nullptr || m == nullptr || v == nullptr ||
      grad == nullptr || out == grid)
    return (int)hipErrorInvalidValue;
  const int ntx = (G + TX - 1) / TX, nty = (G + TY - 1) / TY, ntz = (G + TZ - 1) / TZ;
  const long tiles = (long)ntx * nty * ntz;
  if (tiles > 0x7fffffffL) return (int)hipErrorInvalidValue;
  const double bc1 = 1.0 - pow(b1, (double)step), bc2 = 1.0 - pow(b2, (double)step);
  const double g3 = (double)G * G * G;
  FieldAdam a;
  a.omb1 = (float)(1.0 - b1);
  a.b2 = (float)b2;
  a.omb2 = (float)(1.0 - b2);
  a.eps = (float)eps;
  a.step_size = (float)(lr / bc1);
  a.inv_bc2 = 1.0f / (float)sqrt(bc2);
  a.grad_scale = (float)grad_scale;
  a.tv_rgb = (float)(2.0 * tv_rgb / g3);
  a.tv_sigma = (float)(2.0 * tv_sigma / g3);
  hipLaunchKernelGGL(field_adam_tv_k, dim3((unsigned)tiles, (unsigned)F), dim3(256), 0, st, grid, out, m, v, grad, G,
                     ntx, nty, a);
  return (int)hipGetLastError();
}
