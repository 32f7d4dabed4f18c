// Procedural batches in one launch: scene table, pose and render fused
// (ops.procedural_render / ops.procedural_batch; the torch form and the rule's
// oracle is torch_impl.procedural_scene / procedural_pose / scene_render).
//
// A procedural image is a pure function of (seed, object o, view v).  The
// rule, everything fp64 (u01 is common.h's fp32 uniform01, widened):
//   * o has 3 + hash_u32(seed ^ 0x5bd1e995, o) % 4 primitives in SC_SLOTS
//     slots; slot p reads u_k = u01(seed, (6 o + p) 64 + k), k < 14 (the index
//     in 64 bits: o reaches 2^31 - 1): centre (u0..2 - 0.5) (0.7, 0.5, 0.4),
//     semi-axes 0.08 + 0.22 u3..5, the quaternion (w, x, y, z) = normalize(2
//     u6..9 - 1 + 1e-3), its rotation R, A = diag(1 / axes) R^T row-major,
//     albedo 0.1 + 0.8 u10..12, kind 1 (ellipsoid) if u13 < 0.5, else 2 (box);
//     a dead slot is all zeros;
//   * v reads u = u01(seed ^ 0x7f4a7c15, 2 (4096 o + v) + {0, 1}): azimuth 2 pi
//     u0, elevation 0.05 + 0.95 u1, position t = radius (cos el cos az, cos el
//     sin az, sin el), fwd = -t / |t|, right = normalize(fwd x up), down = fwd
//     x right, R = columns [right, down, fwd] (orbit_look_at), up = (0, 0, 1);
//   * the image of scene.hip's rule under Kinv = inverse(diag(sx, sy, 1) K), K
//     the 128 x 128 SRN pinhole.
// The ids of image n come from two int64 arrays (LIST) or from the batch key
// (DRAW, ProceduralBatches.draw): example g = example_offset + n / 2, frame n
// % 2, rank = hash_u32(s, 4 g) % n_objects, o = 10 rank + 9 (val) or rank +
// rank / 9 (train), v0 = hash_u32(s, 4 g + 1) % views, v1 = (v0 + 1 +
// hash_u32(s, 4 g + 2) % (views - 1)) % views.
//
// Layout: scene_render_k's split of the image -- one thread per pixel, grid
// (ceil(H W / 256), images) -- and its LDS picture (table with each centre
// replaced by the origin in the primitive's frame; Kinv, R), but built by a
// block prologue instead of loaded: lanes 0-5 of wave 0 each build one slot in
// registers, move its centre with scene_origin and store it to LDS; lane 0 of
// wave 1 builds the pose, lane 0 of wave 2 Kinv; one barrier; then the
// unchanged aa x aa trace loop of scene_trace.h and the stores.  The slot
// lanes form the camera position themselves (two hashes, four sin / cos) so
// that the origin needs no second barrier.  The prologue is redundant across
// the blocks of an image: 16 blocks at 64 x 64 each repeat about a hundred fp64
// operations per active lane, against aa^2 6 ray-primitive tests per pixel; a
// second launch to avoid it would cost more than it saves.
// Block blockIdx.x == 0 of an image also writes the image's global outputs
// from the registers of the lanes that built them: the table row [6,16] in
// the public layout (true centres), R [3,3], t [3], and in DRAW mode obj and
// view.  Every output word is written by exactly one thread; no atomics;
// image n depends on entry n of its inputs only.  The ids only enter hashes,
// never an address.
//
// Numerics: fp64, the prologue without contraction (the oracle's operations
// one by one), rounded once at the store: scene.hip's stance.
// Resources (gfx950, -O3): procedural_k<0> and <1> 112 VGPRs (scene_render_k's
// count: the prologue's registers are dead before the trace), 912 B LDS, no
// scratch.
#include "scene_trace.h"

namespace {

#define PR_K_COUNT 0x5BD1E995ull
#define PR_K_POSE 0x7F4A7C15ull
#define PR_VIEWS 4096

struct ProcArgs {
  unsigned long long seed;       // LIST and DRAW: the scene / pose key
  const long long* obj_in;       // LIST [N]
  const long long* view_in;      // LIST [N]
  unsigned long long s;          // DRAW: the batch key
  unsigned n_objects, views;     // DRAW
  int val;                       // DRAW: 1 the held-out split
  long long example_offset;      // DRAW
  long n0;                       // first image of this launch (grid.y chunk)
  int H, W, aa;
  double sx, sy, radius;
  double K[9];
  float* img;                    // [N,3,H,W]
  double* R;                     // [N,3,3]
  double* t;                     // [N,3]
  double* table;                 // [N,6,16] or null
  long long* obj_out;            // DRAW [N / 2]
  long long* view_out;           // DRAW [N]
  float* depth;                  // [N,H,W] or null
  int* prim;                     // with depth
};

__device__ __forceinline__ double pr_u01(unsigned long long seed, unsigned long long idx) {
  return (double)uniform01(seed, idx);
}

// Camera position of view v of object o.
__device__ __forceinline__ void pr_position(unsigned long long seed, unsigned long long o, unsigned long long v,
                                            double radius, double pos[3]) {
#pragma clang fp contract(off)
  const unsigned long long c = 2ull * (o * PR_VIEWS + v);
  const double az = 6.283185307179586 * pr_u01(seed ^ PR_K_POSE, c);
  const double el = 0.05 + 0.95 * pr_u01(seed ^ PR_K_POSE, c + 1);
  const double ce = cos(el);
  pos[0] = radius * (ce * cos(az));
  pos[1] = radius * (ce * sin(az));
  pos[2] = radius * sin(el);
}

// orbit_look_at: R row-major, columns [right, down, fwd].
__device__ __forceinline__ void pr_look_at(const double pos[3], double R[9]) {
#pragma clang fp contract(off)
  const double pn = sqrt(pos[0] * pos[0] + pos[1] * pos[1] + pos[2] * pos[2]);
  const double f[3] = {-pos[0] / pn, -pos[1] / pn, -pos[2] / pn};
  const double up[3] = {0.0, 0.0, 1.0};
  double r[3] = {f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0]};
  const double rn = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  r[0] /= rn;
  r[1] /= rn;
  r[2] /= rn;
  const double d[3] = {f[1] * r[2] - f[2] * r[1], f[2] * r[0] - f[0] * r[2], f[0] * r[1] - f[1] * r[0]};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    R[3 * i] = r[i];
    R[3 * i + 1] = d[i];
    R[3 * i + 2] = f[i];
  }
}

// Slot p of object o in the public layout (true centre); all zeros when dead.
__device__ __forceinline__ void pr_slot(unsigned long long seed, unsigned long long o, int p, double s[SC_WORDS]) {
#pragma clang fp contract(off)
  const int count = 3 + (int)(hash_u32(seed ^ PR_K_COUNT, o) % 4u);
  if (p >= count) {
#pragma unroll
    for (int k = 0; k < SC_WORDS; ++k) s[k] = 0.0;
    return;
  }
  const unsigned long long base = (o * SC_SLOTS + (unsigned long long)p) * 64ull;
  double u[14];
#pragma unroll
  for (int k = 0; k < 14; ++k) u[k] = pr_u01(seed, base + k);
  const double ax[3] = {0.08 + 0.22 * u[3], 0.08 + 0.22 * u[4], 0.08 + 0.22 * u[5]};
  double qw = 2.0 * u[6] - 1.0 + 1e-3, qx = 2.0 * u[7] - 1.0 + 1e-3;
  double qy = 2.0 * u[8] - 1.0 + 1e-3, qz = 2.0 * u[9] - 1.0 + 1e-3;
  const double qn = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
  qw /= qn;
  qx /= qn;
  qy /= qn;
  qz /= qn;
  const double Rm[9] = {1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz),     2 * (qx * qz + qw * qy),
                        2 * (qx * qy + qw * qz),     1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx),
                        2 * (qx * qz - qw * qy),     2 * (qy * qz + qw * qx),     1 - 2 * (qx * qx + qy * qy)};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) s[3 * i + j] = Rm[3 * j + i] / ax[i];      // diag(1 / axes) R^T
  s[9] = (u[0] - 0.5) * 0.7;
  s[10] = (u[1] - 0.5) * 0.5;
  s[11] = (u[2] - 0.5) * 0.4;
  s[12] = 0.1 + 0.8 * u[10];
  s[13] = 0.1 + 0.8 * u[11];
  s[14] = 0.1 + 0.8 * u[12];
  s[15] = u[13] < 0.5 ? 1.0 : 2.0;
}

// DRAW = 0: ids from obj_in / view_in (LIST); 1: from the batch key.
template <int DRAW>
__global__ __launch_bounds__(256) void procedural_k(const ProcArgs a) {
  __shared__ double S[SC_SLOTS][SC_WORDS];
  __shared__ double cam[18];                   // Kinv [9], R [9]
  const int tid = threadIdx.x;
  const long n = a.n0 + blockIdx.y;
  const bool first = blockIdx.x == 0;

  unsigned long long o, v;                     // uniform over the block
  if (DRAW) {
    const unsigned long long g = (unsigned long long)(a.example_offset + n / 2);
    const unsigned long long rank = hash_u32(a.s, 4 * g) % a.n_objects;
    o = a.val ? 10 * rank + 9 : rank + rank / 9;
    const unsigned v0 = hash_u32(a.s, 4 * g + 1) % a.views;
    v = (n & 1) ? (v0 + 1 + hash_u32(a.s, 4 * g + 2) % (a.views - 1)) % a.views : v0;
  } else {
    o = (unsigned long long)a.obj_in[n];
    v = (unsigned long long)a.view_in[n];
  }

  if (tid < SC_SLOTS) {
    double s[SC_WORDS], pos[3];
    pr_slot(a.seed, o, tid, s);
    if (first && a.table != nullptr) {
      double* row = a.table + (n * SC_SLOTS + tid) * SC_WORDS;
#pragma unroll
      for (int k = 0; k < SC_WORDS; ++k) row[k] = s[k];
    }
    pr_position(a.seed, o, v, a.radius, pos);
    scene_origin(s, pos);                      // centre -> the camera origin in the primitive's frame, A (t - c)
#pragma unroll
    for (int k = 0; k < SC_WORDS; ++k) S[tid][k] = s[k];
  } else if (tid == 64) {
    double pos[3], R[9];
    pr_position(a.seed, o, v, a.radius, pos);
    pr_look_at(pos, R);
#pragma unroll
    for (int k = 0; k < 9; ++k) cam[9 + k] = R[k];
    if (first) {
#pragma unroll
      for (int k = 0; k < 9; ++k) a.R[n * 9 + k] = R[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) a.t[n * 3 + k] = pos[k];
      if (DRAW) {
        a.view_out[n] = (long long)v;
        if ((n & 1) == 0) a.obj_out[n / 2] = (long long)o;
      }
    }
  } else if (tid == 128) {
    scene_kinv(a.K, a.sx, a.sy, cam, nullptr);   // inverse of diag(sx, sy, 1) K by the adjugate
  }
  __syncthreads();

  const long HW = (long)a.H * a.W;
  const long pix = (long)blockIdx.x * 256 + tid;
  if (pix >= HW) return;
  const int py = (int)(pix / a.W), px = (int)(pix % a.W);
  const int aa = a.aa;

  double acc[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < aa; ++i)
    for (int j = 0; j < aa; ++j) {
      const Hit h = scene_trace(S, cam, px + (j + 0.5) / aa, py + (i + 0.5) / aa);
      acc[0] += h.c[0];
      acc[1] += h.c[1];
      acc[2] += h.c[2];
    }
  const double cnt = (double)(aa * aa);
  float* out = a.img + n * 3 * HW + pix;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c * HW] = (float)(2.0 * (acc[c] / cnt) - 1.0);
  if (a.depth != nullptr) {
    const Hit h = scene_trace(S, cam, px + 0.5, py + 0.5);
    a.depth[n * HW + pix] = (float)h.t;
    a.prim[n * HW + pix] = h.prim;
  }
}

template <int DRAW>
int procedural_launch(ProcArgs a, long N, hipStream_t st) {
  const long gx = ((long)a.H * a.W + 255) / 256;
  if (gx > 0x7fffffffL) return (int)hipErrorInvalidValue;
  for (long n0 = 0; n0 < N; n0 += 65535) {     // grid.y limit
    const int nb = (int)(N - n0 < 65535 ? N - n0 : 65535);
    a.n0 = n0;
    hipLaunchKernelGGL(procedural_k<DRAW>, dim3((unsigned)gx, (unsigned)nb), dim3(256), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return (int)hipSuccess;
}

bool procedural_common(ProcArgs& a, int H, int W, int aa, int ref, double radius, const double* K, float* img,
                       double* R, double* t, double* table, float* depth, int* prim) {
  if (H <= 0 || W <= 0 || ref <= 0 || aa < 1 || aa > 4 || !(radius > 0.0) || K == nullptr || img == nullptr ||
      R == nullptr || t == nullptr || (depth == nullptr) != (prim == nullptr))
    return false;
  a.H = H;
  a.W = W;
  a.aa = aa;
  a.sx = (double)W / ref;
  a.sy = (double)H / ref;
  a.radius = radius;
  for (int k = 0; k < 9; ++k) a.K[k] = K[k];
  a.img = img;
  a.R = R;
  a.t = t;
  a.table = table;
  a.depth = depth;
  a.prim = prim;
  return true;
}
}  // namespace

// LIST: obj / view int64 [N] on the device (object ids in [0, 2^31), view ids
// in [0, 4096): the caller's check); K: 9 HOST doubles, the intrinsics of the
// ref x ref image; img fp32 [N,3,H,W]; R fp64 [N,3,3]; t fp64 [N,3]; table
// fp64 [N,6,16] or null; depth fp32 [N,H,W] and prim int32 [N,H,W], both null
// or both set.
D3D_API int d3d_procedural_render(unsigned long long seed, const long long* obj, const long long* view, long N, int H,
                                  int W, int aa, int ref, double radius, const double* K, float* img, double* R,
                                  double* t, double* table, float* depth, int* prim, hipStream_t st) {
  ProcArgs a = {};
  if (N <= 0 || obj == nullptr || view == nullptr ||
      !procedural_common(a, H, W, aa, ref, radius, K, img, R, t, table, depth, prim))
    return (int)hipErrorInvalidValue;
  a.seed = seed;
  a.obj_in = obj;
  a.view_in = view;
  return procedural_launch<0>(a, N, st);
}

// DRAW: examples example_offset .. + B of the batch whose key is s (the host
// folds (seed, batch index) into it); n_objects in [1, 2^31], views in [2,
// 4096], val 1 for the held-out split.  obj int64 [B], view int64 [B,2], img
// fp32 [B,2,3,H,W], R fp64 [B,2,3,3], t fp64 [B,2,3]; table fp64 [2 B,6,16] or
// null.
D3D_API int d3d_procedural_batch(unsigned long long seed, unsigned long long s, long n_objects, int views, int val,
                                 long example_offset, long B, int H, int W, int aa, int ref, double radius,
                                 const double* K, long long* obj, long long* view, float* img, double* R, double* t,
                                 double* table, hipStream_t st) {
  ProcArgs a = {};
  if (B <= 0 || B > (1L << 40) || n_objects < 1 || n_objects > (1L << 31) || views < 2 || views > PR_VIEWS ||
      example_offset < 0 || example_offset > (1L << 60) || obj == nullptr || view == nullptr ||
      !procedural_common(a, H, W, aa, ref, radius, K, img, R, t, table, nullptr, nullptr))
    return (int)hipErrorInvalidValue;
  a.seed = seed;
  a.s = s;
  a.n_objects = (unsigned)n_objects;
  a.views = (unsigned)views;
  a.val = val != 0;
  a.example_offset = example_offset;
  a.obj_out = obj;
  a.view_out = view;
  return procedural_launch<1>(a, 2 * B, st);
}
