// Fused multi-head self / cross-view attention at head dims 32 and 256.
//
// attention.hip serves D = C / heads in {64, 128}; this file serves the two
// neighbouring values the model's `attn_heads` knob reaches (8 heads -> D = 32
// at the 16x16 level, 2 heads -> D = 256 at the 8x8 level) with work splits
// of their own.  Same conventions: qkv [N, L, 3C] bf16 packed q | k | v with
// head h at columns h*D..h*D+D-1, out [N, L, C] bf16, lse [N, heads, L] fp32
// (natural log), key / value image n (self) or n ^ 1 (cross), any L >= 1
// (keys past L score -inf, query rows past L are neither stored nor allowed
// to contribute), online softmax in base 2 with scale * log2(e) folded in,
// mfma_f32_16x16x32_bf16 throughout, no atomics and every reduction in a
// fixed order (dQ bitwise reproducible).  The MFMA operand layouts (keys on
// the forward's MFMA rows, keys on the backward's lanes, the permuted key
// order inside a 32-key step) are those described in attention.hip.
//
// D = 32, the head-pair kernels.  A head's row is 64 bytes, half a cache
// line, and there is one MFMA per 16-key score tile, so a workgroup serves
// TWO adjacent heads of one image: every staged K / V / Q / dO row is the 128
// contiguous bytes of both heads, in the D = 64 tile geometry ([rows][64
// columns], 16-byte-chunk XOR swizzle for K, V padded to 80 columns for the
// transpose reads), and a wave's head selects the 32-column half.
//   forward : 8 waves, waves 0-3 head 2p, waves 4-7 head 2p+1, 16 queries of
//             a 64-query block each; K / V of a 64-key block staged once for
//             both heads, the next block's fetch in flight in registers.
//   backward: one workgroup per (image, head pair, key block); the 32-query
//             Q / dO tile is staged once for both heads, each wave owns 16-key
//             groups of one head (kf, vf one chunk, dk, dv two tiles per
//             group).  L <= 64: one 64-key workgroup (8 waves); 64 < L <= 256:
//             one 256-key workgroup (8 waves x 4 key groups, 84 KB of dynamic
//             LDS; 16 waves x 2 groups spilled at the 128-register budget)
//             owns every key, so dQ leaves as bf16 directly; L > 256:
//             64-key workgroups write fp32 dQ slabs that dq_sum_k adds in
//             key-block order.
//   An odd head count leaves the last pair with one head: the missing half
//   is never loaded (zeros are staged) and never stored, and its waves run
//   the same barriers on zeros.
//
// D = 256, the split-D kernels.
//   forward : 4 waves, one per 16 queries (o = 16 tiles = 64 accumulator
//             registers, q = 8 fragments).  Key block = 32 keys: the block in
//             flight is 4 + 4 16-byte chunks per thread (32 registers); a
//             64-key block would hold 64, and with o (64), q (32) and the
//             transpose reads in flight the kernel sits at 220 registers,
//             under the 256 that two waves per SIMD allow (launch bound),
//             only with the short block.  The kernel is bound by its 16
//             transpose reads per 32-key step, and the second resident wave
//             is what hides them.  K (16 KB) and padded V (17 KB) stay a
//             static 33 KB block (64 keys: 66 KB, dynamic LDS).  The price
//             is one accumulator rescale per 32 keys, not 64.
//   backward: 64 keys per workgroup, 8 waves: a PAIR of waves shares a
//             16-key group, wave A holds columns 0-127 of dK / dV (8 + 8
//             tiles) and of the K / V fragments, wave B columns 128-255.
//             Variant (a) of the two ways to form S and dP: each wave
//             contracts over its own 128 columns (4 + 4 MFMAs per 16 x 16
//             tile where the full-S form (b) needs 8 + 8 in both waves, from
//             LDS), and the pair exchanges the partial sums through a 32 KB
//             fp32 LDS buffer, summed as A + B in both waves.  The resource
//             report (profiles/attn_headdim/README.md): 252 VGPRs, 0 bytes of
//             scratch, 2 waves per SIMD -- the split form fits the 8-wave
//             register budget, so the MFMA-doubling form (b) was not built.
//             dQ = dS K is split the same way over its 16 column tiles.
//             105 KB of dynamic LDS.  L <= 64 writes bf16 dQ directly, longer
//             sequences go through the slabs.
//
// The C entry points take pointers and launch constants only: no allocation,
// no synchronisation (they are captured into graphs).  The dynamic-LDS limit
// of a kernel is raised once per process.
#include "common.h"

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

namespace {

constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ s16x4 ds_tr(const bf16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
}
__device__ __forceinline__ bf16x8 tr8(const bf16* base, int stride, int r1, int r2, int col) {
  s16x4 lo = ds_tr(base + r1 * stride + col);
  s16x4 hi = ds_tr(base + r2 * stride + col);
  s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}
__device__ __forceinline__ bf16x8 pack8(f32x4 a, f32x4 b) {
  bf16x8 r;
  r[0] = (bf16)a[0]; r[1] = (bf16)a[1]; r[2] = (bf16)a[2]; r[3] = (bf16)a[3];
  r[4] = (bf16)b[0]; r[5] = (bf16)b[1]; r[6] = (bf16)b[2]; r[7] = (bf16)b[3];
  return r;
}
// swizzled [row][W] tile of 16-byte chunks for ds_read_b128 row reads
template <int W>
__device__ __forceinline__ int swz(int row, int chunk) {
  return row * W + ((chunk ^ (row & 7)) << 3);
}
__device__ __forceinline__ bf16x8 ldg8(const bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }

// online-softmax step shared by both forwards: s holds NK 16-key score tiles
// of query column (lane & 15), keys kb + 16 kt + 4 g + i; returns alpha
template <int NK>
__device__ __forceinline__ float softmax_step(f32x4 (&s)[NK], int kb, int g, int L, float sl2, float& m, float& l) {
  float mb = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < NK; ++kt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s[kt][i] = kb + 16 * kt + 4 * g + i < L ? s[kt][i] * sl2 : -INFINITY;   // keys past L
      mb = fmaxf(mb, s[kt][i]);
    }
  mb = fmaxf(mb, __shfl_xor(mb, 16, 64));
  mb = fmaxf(mb, __shfl_xor(mb, 32, 64));
  const float mn = fmaxf(m, mb);               // finite: key kb < L is in every block
  const float alpha = exp2f(m - mn);
  float ls = 0.f;
#pragma unroll
  for (int kt = 0; kt < NK; ++kt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s[kt][i] = exp2f(s[kt][i] - mn);
      ls += s[kt][i];
    }
  ls += __shfl_xor(ls, 16, 64);
  ls += __shfl_xor(ls, 32, 64);
  l = l * alpha + ls;
  m = mn;
  return alpha;
}

// ------------------------------------------------- D = 32: head pairs ----
__global__ void __launch_bounds__(512) attn32_fwd_k(const bf16* __restrict__ qkv, bf16* __restrict__ out,
                                                    float* __restrict__ lse, int L, int C, int heads, int cross,
                                                    float scale) {
  constexpr int VS = 64 + 16;                // padded V row (tr reads)
  __shared__ __attribute__((aligned(16))) bf16 Ks[64 * 64];
  __shared__ __attribute__((aligned(16))) bf16 Vs[64 * VS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int hh = w >> 2, wq = w & 3;         // head of the pair, 16-query group
  const int qblk = blockIdx.x, hp = blockIdx.y, n = blockIdx.z;
  const int nkv = cross ? (n ^ 1) : n;
  const int g = lane >> 4, fr = lane & 15, qq = (lane & 15) >> 2, pc = lane & 3;
  const long C3 = 3L * C;
  const int h = 2 * hp + hh;
  const int q = qblk * 64 + wq * 16 + fr;
  const bool qok = h < heads && q < L;       // missing head of an odd count, ragged last block
  const bf16x8 qf = qok ? ldg8(qkv + ((long)n * L + q) * C3 + h * 32 + 8 * g) : bf16x8{};

  f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  float m = -INFINITY, l = 0.f;
  const float sl2 = scale * LOG2E;

  // one 16-byte chunk of K and of V per thread and key block, one block ahead
  const int sr = tid >> 3, sc = tid & 7;
  const bool hok = 2 * hp + (sc >> 2) < heads;
  bf16x8 kr, vr;
  auto fetch = [&](int kb) {
    const bool ok = hok && kb + sr < L;
    const bf16* src = qkv + ((long)nkv * L + (ok ? kb + sr : 0)) * C3 + (ok ? hp * 64 + sc * 8 : 0);
    kr = ok ? ldg8(src + C) : bf16x8{};
    vr = ok ? ldg8(src + 2 * C) : bf16x8{};
  };
  fetch(0);
  for (int kb = 0; kb < L; kb += 64) {
    *reinterpret_cast<bf16x8*>(Ks + swz<64>(sr, sc)) = kr;
    *reinterpret_cast<bf16x8*>(Vs + sr * VS + sc * 8) = vr;
    if (kb + 64 < L) fetch(kb + 64);
    __syncthreads();
    f32x4 s[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      bf16x8 a = *reinterpret_cast<const bf16x8*>(Ks + swz<64>(16 * kt + fr, 4 * hh + g));
      s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, qf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    }
    const float alpha = softmax_step<4>(s, kb, g, L, sl2, m, l);
    o[0] *= alpha;
    o[1] *= alpha;
    // O^T += V^T P^T, two 32-key steps
#pragma unroll
    for (int kc2 = 0; kc2 < 2; ++kc2) {
      bf16x8 pb = pack8(s[2 * kc2], s[2 * kc2 + 1]);
      const int r1 = 32 * kc2 + 4 * g + qq, r2 = r1 + 16;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        bf16x8 va = tr8(Vs, VS, r1, r2, 32 * hh + 16 * t + 4 * pc);
        o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pb, o[t], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  if (!qok) return;
  const float inv = 1.f / l;
  bf16* orow = out + ((long)n * L + q) * C + h * 32;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    bf16x4 v4;
#pragma unroll
    for (int i = 0; i < 4; ++i) v4[i] = (bf16)(o[t][i] * inv);
    *reinterpret_cast<bf16x4*>(orow + 16 * t + 4 * g) = v4;
  }
  if (g == 0) lse[((long)n * heads + h) * L + q] = (m + log2f(l)) / LOG2E;
}

extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];

// KW keys per workgroup, 8 waves: 64 (one 16-key group per wave; L <= 64, or
// the slab form above 256 keys) or 256 (four groups per wave, all keys of an
// L <= 256 sequence).  Waves 0-3 serve head 2p, waves 4-7 head 2p+1.
template <int KW>
constexpr int attn32_bwd_lds() {
  return (2 * 32 * 80 + KW * 80 + 2 * 32 * (KW + 8)) * 2 + 128 * 4;
}
template <int KW>
__global__ void __launch_bounds__(512) attn32_bwd_k(
    const bf16* __restrict__ qkv, const bf16* __restrict__ dout, const float* __restrict__ lse,
    const bf16* __restrict__ out, float* __restrict__ dq_acc, bf16* __restrict__ dqkv, int L, int C, int heads,
    int cross, float scale) {
  constexpr int NWH = 4, NT = 512, KG = KW / (16 * NWH);
  constexpr int TS = 64 + 16;     // padded rows: row reads + tr reads
  constexpr int SS = KW + 8;      // dS tile row stride (bf16)
  bf16* Qs = reinterpret_cast<bf16*>(dyn_lds);          // [32][TS]
  bf16* dOs = Qs + 32 * TS;                             // [32][TS]
  bf16* Kt = dOs + 32 * TS;                             // [KW][TS]
  bf16* dSs = Kt + KW * TS;                             // [2 heads][32][SS]
  float* lse_s = reinterpret_cast<float*>(dSs + 2 * 32 * SS);   // [2][32]
  float* D_s = lse_s + 64;                              // [2][32]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int hh = w / NWH, wk = w % NWH;
  const int kblk = blockIdx.x, hp = blockIdx.y, n = blockIdx.z;
  const int nkv = cross ? (n ^ 1) : n;
  const int g = lane >> 4, fr = lane & 15, qq = (lane & 15) >> 2, pc = lane & 3;
  const long C3 = 3L * C;
  const int k0 = kblk * KW;
  const int h = 2 * hp + hh;
  const bool hvalid = h < heads;
  const float sl2 = scale * LOG2E;
  const int sr = tid >> 3, sc = tid & 7;                // staged row / 16-byte chunk of the 64-column tile
  const bool sc_ok = 2 * hp + (sc >> 2) < heads;        // the chunk's head exists

  // K tile of the block (both heads, for dQ) and this wave's K / V fragments
#pragma unroll
  for (int i = 0; i < KW * 8 / NT; ++i) {
    const int r = sr + i * (NT / 8);
    const bool ok = sc_ok && k0 + r < L;
    *reinterpret_cast<bf16x8*>(Kt + r * TS + sc * 8) =
        ok ? ldg8(qkv + ((long)nkv * L + k0 + r) * C3 + C + hp * 64 + sc * 8) : bf16x8{};
  }
  bool kok[KG];
  bf16x8 kf[KG], vf[KG];
  f32x4 dk[KG][2], dv[KG][2];
#pragma unroll
  for (int kg = 0; kg < KG; ++kg) {
    const int key = k0 + 16 * (wk + NWH * kg) + fr;
    kok[kg] = hvalid && key < L;
    const bf16* krow = qkv + ((long)nkv * L + (kok[kg] ? key : 0)) * C3 + (kok[kg] ? h * 32 + 8 * g : 0);
    kf[kg] = kok[kg] ? ldg8(krow + C) : bf16x8{};
    vf[kg] = kok[kg] ? ldg8(krow + 2 * C) : bf16x8{};
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      dk[kg][t] = f32x4{0.f, 0.f, 0.f, 0.f};
      dv[kg][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  const bool direct_dq = L <= KW;                       // one key block: dQ is complete here
  const int nkc = min(KW, L - k0 + 31) / 32;            // 32-key steps of dQ = dS K that hold a key < L

  // tile q0 + 32 is loaded into registers while tile q0 computes.  Waves
  // 0-3: one chunk of Q and of dO (32 rows x 8 chunks), and one chunk of the
  // D-term operands: 4 adjacent lanes per (row, head), 8 columns each.
  bf16x8 qr, dr, orr, drr;
  float lse_r = 0.f;
  bool lse_ok = false;
  const int dpair = tid >> 2, drow = dpair >> 1, dhd = dpair & 1, dpart = tid & 3;
  auto fetch = [&](int qb) {
    {
      const bool ok = tid < 256 && sc_ok && qb + sr < L;
      const long row = (long)n * L + (ok ? qb + sr : 0);
      const int col = ok ? hp * 64 + sc * 8 : 0;
      qr = ok ? ldg8(qkv + row * C3 + col) : bf16x8{};
      dr = ok ? ldg8(dout + row * C + col) : bf16x8{};
    }
    {
      const bool ok = tid < 256 && 2 * hp + dhd < heads && qb + drow < L;
      const long off = ok ? ((long)n * L + qb + drow) * C + (2 * hp + dhd) * 32 + dpart * 8 : 0;
      orr = ok ? ldg8(out + off) : bf16x8{};
      drr = ok ? ldg8(dout + off) : bf16x8{};
    }
    // threads 0-63: lse of (head tid >> 5, row tid & 31); unconditional load
    const int lh = 2 * hp + ((tid >> 5) & 1), li = qb + (tid & 31);
    lse_ok = tid < 64 && lh < heads && li < L;
    lse_r = lse[lse_ok ? ((long)n * heads + lh) * L + li : 0];
  };
  fetch(0);

  for (int q0 = 0; q0 < L; q0 += 32) {
    __syncthreads();
    if (tid < 256) {
      *reinterpret_cast<bf16x8*>(Qs + sr * TS + sc * 8) = qr;
      *reinterpret_cast<bf16x8*>(dOs + sr * TS + sc * 8) = dr;
      // D[head][q] = sum over the head's own 32 columns of dO * O
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc += (float)orr[j] * (float)drr[j];
      acc += __shfl_xor(acc, 1, 64);
      acc += __shfl_xor(acc, 2, 64);
      if (dpart == 0) D_s[dhd * 32 + drow] = acc;
    }
    // query rows past L (and a missing head): lse = +inf makes the probabilities exactly 0
    if (tid < 64) lse_s[tid] = lse_ok ? lse_r * LOG2E : INFINITY;
    if (q0 + 32 < L) fetch(q0 + 32);                    // in flight during this tile's compute
    __syncthreads();
#pragma unroll
    for (int kg = 0; kg < KG; ++kg) {
      f32x4 p[2], ds[2];
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        bf16x8 a = *reinterpret_cast<const bf16x8*>(Qs + (16 * qt + fr) * TS + 32 * hh + 8 * g);
        f32x4 s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, kf[kg], z, 0, 0, 0);
        bf16x8 b = *reinterpret_cast<const bf16x8*>(dOs + (16 * qt + fr) * TS + 32 * hh + 8 * g);
        f32x4 dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, vf[kg], z, 0, 0, 0);
        // rows: q = 16qt + 4g + i ; column (lane): key
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int qi = 32 * hh + 16 * qt + 4 * g + i;
          const float pv = kok[kg] ? exp2f(s[i] * sl2 - lse_s[qi]) : 0.f;
          p[qt][i] = pv;
          ds[qt][i] = pv * (dp[i] - D_s[qi]);
        }
      }
      // dV += P^T dO ; dK += dS^T Q  (k-slots permuted: q = {4g+j, 16+4g+j})
      bf16x8 pa = pack8(p[0], p[1]);
      bf16x8 dsa = pack8(ds[0], ds[1]);
      const int r1 = 4 * g + qq, r2 = 16 + 4 * g + qq;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        bf16x8 bo = tr8(dOs, TS, r1, r2, 32 * hh + 16 * t + 4 * pc);
        dv[kg][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, bo, dv[kg][t], 0, 0, 0);
        bf16x8 bq = tr8(Qs, TS, r1, r2, 32 * hh + 16 * t + 4 * pc);
        dk[kg][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsa, bq, dk[kg][t], 0, 0, 0);
      }
      // dS -> LDS [head][32 q][KW keys], columns in the permuted k-slot order
      // of the tr-read K operand: key u of a 32-key chunk -> slot
      // 8*(u/4)+u%4 (u<16), 8*((u-16)/4)+4+u%4
      {
        const int kl = 16 * (wk + NWH * kg) + fr, u = kl & 31;
        const int col = (kl & ~31) + (u < 16 ? 8 * (u >> 2) + (u & 3) : 8 * ((u - 16) >> 2) + 4 + (u & 3));
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
#pragma unroll
          for (int i = 0; i < 4; ++i) dSs[(32 * hh + 16 * qt + 4 * g + i) * SS + col] = (bf16)ds[qt][i];
      }
    }
    __syncthreads();
    // dQ tiles: 2 heads x 2 (q) x 2 (d), one per wave
    {
      const int hd = w >> 2, qt = (w >> 1) & 1, t = w & 1;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int kc = 0; kc < nkc; ++kc) {
        bf16x8 a = *reinterpret_cast<const bf16x8*>(dSs + (32 * hd + 16 * qt + fr) * SS + 32 * kc + 8 * g);
        bf16x8 b = tr8(Kt, TS, 32 * kc + 4 * g + qq, 32 * kc + 16 + 4 * g + qq, 32 * hd + 16 * t + 4 * pc);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
      }
      // acc rows: q = 16qt + 4g + i, column d = 16t + fr of head 2p + hd
      if (2 * hp + hd < heads) {
        const int col = (2 * hp + hd) * 32 + 16 * t + fr;
        float* slab = direct_dq ? nullptr : dq_acc + (long)kblk * gridDim.z * L * C;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int qi = q0 + 16 * qt + 4 * g + i;
          if (qi >= L) continue;
          const long row = (long)n * L + qi;
          if (direct_dq)
            dqkv[row * C3 + col] = (bf16)(acc[i] * scale);
          else
            slab[row * C + col] = acc[i] * scale;
        }
      }
    }
  }
  // dk[kg][t][i] = dK[key 16 (wk + NWH kg) + 4g + i][d = 16t + fr]
  if (!hvalid) return;
#pragma unroll
  for (int kg = 0; kg < KG; ++kg)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int kk = k0 + 16 * (wk + NWH * kg) + 4 * g + i;
        if (kk >= L) continue;
        const long row = (long)nkv * L + kk;
        dqkv[row * C3 + C + h * 32 + 16 * t + fr] = (bf16)(dk[kg][t][i] * scale);
        dqkv[row * C3 + 2 * C + h * 32 + 16 * t + fr] = (bf16)dv[kg][t][i];
      }
}

// --------------------------------------------------- D = 256: split D ----
__global__ void __launch_bounds__(256, 2) attn256_fwd_k(const bf16* __restrict__ qkv, bf16* __restrict__ out,
                                                     float* __restrict__ lse, int L, int C, int heads, int cross,
                                                     float scale) {
  constexpr int D = 256, VS = D + 16, KB = 32;          // key block (see the header)
  __shared__ __attribute__((aligned(16))) bf16 Ks[KB * D];
  __shared__ __attribute__((aligned(16))) bf16 Vs[KB * VS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int qblk = blockIdx.x, h = blockIdx.y, n = blockIdx.z;
  const int nkv = cross ? (n ^ 1) : n;
  const int g = lane >> 4, fr = lane & 15, qq = (lane & 15) >> 2, pc = lane & 3;
  const long C3 = 3L * C;
  const int q = qblk * 64 + w * 16 + fr;
  const bool qok = q < L;
  const bf16* qrow = qkv + ((long)n * L + (qok ? q : 0)) * C3 + h * D;
  bf16x8 qf[8];
#pragma unroll
  for (int kc = 0; kc < 8; ++kc) qf[kc] = qok ? ldg8(qrow + 32 * kc + 8 * g) : bf16x8{};
  f32x4 o[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;
  const float sl2 = scale * LOG2E;

  // 32 rows x 32 chunks of each of K / V: 4 chunks per thread, one block ahead
  bf16x8 kr[4], vr[4];
  auto fetch = [&](int kb) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + i * 256, r = idx >> 5, c = idx & 31;
      const bool ok = kb + r < L;
      const bf16* src = qkv + ((long)nkv * L + (ok ? kb + r : 0)) * C3 + h * D + c * 8;
      kr[i] = ok ? ldg8(src + C) : bf16x8{};
      vr[i] = ok ? ldg8(src + 2 * C) : bf16x8{};
    }
  };
  fetch(0);
  for (int kb = 0; kb < L; kb += KB) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + i * 256, r = idx >> 5, c = idx & 31;
      *reinterpret_cast<bf16x8*>(Ks + swz<D>(r, c)) = kr[i];
      *reinterpret_cast<bf16x8*>(Vs + r * VS + c * 8) = vr[i];
    }
    if (kb + KB < L) fetch(kb + KB);
    __syncthreads();
    f32x4 s[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kc = 0; kc < 8; ++kc) {
        bf16x8 a = *reinterpret_cast<const bf16x8*>(Ks + swz<D>(16 * kt + fr, 4 * kc + g));
        s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, qf[kc], s[kt], 0, 0, 0);
      }
    }
    const float alpha = softmax_step<2>(s, kb, g, L, sl2, m, l);
#pragma unroll
    for (int t = 0; t < 16; ++t) o[t] *= alpha;
    // O^T += V^T P^T, one 32-key step, 16 transpose-read tiles
    bf16x8 pb = pack8(s[0], s[1]);
    const int r1 = 4 * g + qq, r2 = r1 + 16;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      bf16x8 va = tr8(Vs, VS, r1, r2, 16 * t + 4 * pc);
      o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pb, o[t], 0, 0, 0);
    }
    __syncthreads();
  }
  if (!qok) return;
  const float inv = 1.f / l;
  bf16* orow = out + ((long)n * L + q) * C + h * D;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    bf16x4 v4;
#pragma unroll
    for (int i = 0; i < 4; ++i) v4[i] = (bf16)(o[t][i] * inv);
    *reinterpret_cast<bf16x4*>(orow + 16 * t + 4 * g) = v4;
  }
  if (g == 0) lse[((long)n * heads + h) * L + q] = (m + log2f(l)) / LOG2E;
}

// 64 keys per workgroup; wave w: 16-key group w >> 1, column half w & 1.
constexpr int ATTN256_BWD_LDS = (2 * 32 * 272 + 64 * 272 + 32 * 72) * 2 + (8 * 16 * 64 + 64) * 4;
__global__ void __launch_bounds__(512) attn256_bwd_k(const bf16* __restrict__ qkv, const bf16* __restrict__ dout,
                                                     const float* __restrict__ lse, const bf16* __restrict__ out,
                                                     float* __restrict__ dq_acc, bf16* __restrict__ dqkv, int L,
                                                     int C, int heads, int cross, float scale) {
  constexpr int D = 256, KW = 64, NT = 512;
  constexpr int TS = D + 16;      // padded rows: row reads + tr reads
  constexpr int SS = KW + 8;      // dS tile row stride (bf16)
  bf16* Qs = reinterpret_cast<bf16*>(dyn_lds);          // [32][TS]
  bf16* dOs = Qs + 32 * TS;                             // [32][TS]
  bf16* Kt = dOs + 32 * TS;                             // [KW][TS]
  bf16* dSs = Kt + KW * TS;                             // [32][SS]
  float* xs = reinterpret_cast<float*>(dSs + 32 * SS);  // [8 waves][16 values][64 lanes] partial S / dP
  float* lse_s = xs + 8 * 16 * 64;                      // [32]
  float* D_s = lse_s + 32;                              // [32]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int kgp = w >> 1, half = w & 1;
  const int kblk = blockIdx.x, h = blockIdx.y, n = blockIdx.z;
  const int nkv = cross ? (n ^ 1) : n;
  const int g = lane >> 4, fr = lane & 15, qq = (lane & 15) >> 2, pc = lane & 3;
  const long C3 = 3L * C;
  const int k0 = kblk * KW;
  const float sl2 = scale * LOG2E;

  // K tile of the block (for dQ): 64 rows x 32 chunks, 4 per thread
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = tid + i * NT, r = idx >> 5, c = idx & 31;
    *reinterpret_cast<bf16x8*>(Kt + r * TS + c * 8) =
        k0 + r < L ? ldg8(qkv + ((long)nkv * L + k0 + r) * C3 + C + h * D + c * 8) : bf16x8{};
  }
  // this wave's half of its keys' K / V rows (B operands) and of dK / dV
  const int key = k0 + 16 * kgp + fr;
  const bool kok = key < L;
  bf16x8 kf[4], vf[4];
  f32x4 dk[8], dv[8];
  {
    const bf16* krow = qkv + ((long)nkv * L + (kok ? key : 0)) * C3 + h * D + 128 * half + 8 * g;
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      kf[kc] = kok ? ldg8(krow + C + 32 * kc) : bf16x8{};
      vf[kc] = kok ? ldg8(krow + 2 * C + 32 * kc) : bf16x8{};
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      dk[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      dv[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  const float* lse_nh = lse + ((long)n * heads + h) * L;
  const bool direct_dq = L <= KW;
  const int nkc = min(KW, L - k0 + 31) / 32;            // 32-key steps of dQ = dS K that hold a key < L

  // next tile in registers: 32 rows x 32 chunks of Q and dO (2 per thread),
  // D-term operands (16 lanes per row, 16 columns each)
  bf16x8 qr[2], dr[2], orr[2], drr[2];
  float lse_r = 0.f;
  bool lse_ok = false;
  const int drow = tid >> 4, dpart = tid & 15;
  auto fetch = [&](int qb) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + i * NT, r = idx >> 5, c = idx & 31;
      const bool ok = qb + r < L;
      const long row = (long)n * L + (ok ? qb + r : 0);
      qr[i] = ok ? ldg8(qkv + row * C3 + h * D + c * 8) : bf16x8{};
      dr[i] = ok ? ldg8(dout + row * C + h * D + c * 8) : bf16x8{};
    }
    {
      const bool ok = qb + drow < L;
      const long off = ((long)n * L + (ok ? qb + drow : 0)) * C + h * D + dpart * 16;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        orr[k] = ok ? ldg8(out + off + 8 * k) : bf16x8{};
        drr[k] = ok ? ldg8(dout + off + 8 * k) : bf16x8{};
      }
    }
    const int li = qb + (tid & 31);
    lse_ok = tid < 32 && li < L;
    lse_r = lse_nh[li < L ? li : 0];
  };
  fetch(0);

  for (int q0 = 0; q0 < L; q0 += 32) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + i * NT, r = idx >> 5, c = idx & 31;
      *reinterpret_cast<bf16x8*>(Qs + r * TS + c * 8) = qr[i];
      *reinterpret_cast<bf16x8*>(dOs + r * TS + c * 8) = dr[i];
    }
    if (tid < 32) lse_s[tid] = lse_ok ? lse_r * LOG2E : INFINITY;   // rows past L: p = 0
    {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += (float)orr[k][j] * (float)drr[k][j];
      acc += __shfl_xor(acc, 1, 64);
      acc += __shfl_xor(acc, 2, 64);
      acc += __shfl_xor(acc, 4, 64);
      acc += __shfl_xor(acc, 8, 64);
      if (dpart == 0) D_s[drow] = acc;
    }
    if (q0 + 32 < L) fetch(q0 + 32);
    __syncthreads();
    // partial S and dP over this wave's 128 columns, exchanged with the
    // partner wave (w ^ 1) through xs
    f32x4 s[2], dp[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      s[qt] = f32x4{0.f, 0.f, 0.f, 0.f};
      dp[qt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) {
        const int off = (16 * qt + fr) * TS + 128 * half + 32 * kc + 8 * g;
        bf16x8 a = *reinterpret_cast<const bf16x8*>(Qs + off);
        s[qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, kf[kc], s[qt], 0, 0, 0);
        bf16x8 b = *reinterpret_cast<const bf16x8*>(dOs + off);
        dp[qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, vf[kc], dp[qt], 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        xs[(w * 16 + qt * 8 + i) * 64 + lane] = s[qt][i];
        xs[(w * 16 + qt * 8 + 4 + i) * 64 + lane] = dp[qt][i];
      }
    }
    __syncthreads();
    f32x4 p[2], ds[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        // fixed order: columns 0-127 (wave A) + columns 128-255 (wave B)
        const float so = xs[((w ^ 1) * 16 + qt * 8 + i) * 64 + lane];
        const float dpo = xs[((w ^ 1) * 16 + qt * 8 + 4 + i) * 64 + lane];
        const float sf = half ? so + s[qt][i] : s[qt][i] + so;
        const float dpf = half ? dpo + dp[qt][i] : dp[qt][i] + dpo;
        const int qi = 16 * qt + 4 * g + i;
        const float pv = kok ? exp2f(sf * sl2 - lse_s[qi]) : 0.f;
        p[qt][i] = pv;
        ds[qt][i] = pv * (dpf - D_s[qi]);
      }
    // dV += P^T dO ; dK += dS^T Q over this wave's 8 column tiles
    bf16x8 pa = pack8(p[0], p[1]);
    bf16x8 dsa = pack8(ds[0], ds[1]);
    const int r1 = 4 * g + qq, r2 = 16 + 4 * g + qq;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      bf16x8 bo = tr8(dOs, TS, r1, r2, 128 * half + 16 * t + 4 * pc);
      dv[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, bo, dv[t], 0, 0, 0);
      bf16x8 bq = tr8(Qs, TS, r1, r2, 128 * half + 16 * t + 4 * pc);
      dk[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsa, bq, dk[t], 0, 0, 0);
    }
    // dS -> LDS [32 q][64 keys] (both waves of a pair hold the same values:
    // wave A stores), columns in the permuted k-slot order of the tr-read K
    if (half == 0) {
      const int kl = 16 * kgp + fr, u = kl & 31;
      const int col = (kl & ~31) + (u < 16 ? 8 * (u >> 2) + (u & 3) : 8 * ((u - 16) >> 2) + 4 + (u & 3));
#pragma unroll
      for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int i = 0; i < 4; ++i) dSs[(16 * qt + 4 * g + i) * SS + col] = (bf16)ds[qt][i];
    }
    __syncthreads();
    // dQ = dS K: 2 (q) x 16 (d) tiles; a wave takes 4 tiles of its column half
    float* slab = direct_dq ? nullptr : dq_acc + (long)kblk * gridDim.z * L * C;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ti = kgp * 4 + j, qt = ti >> 3, t = half * 8 + (ti & 7);
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int kc = 0; kc < nkc; ++kc) {
        bf16x8 a = *reinterpret_cast<const bf16x8*>(dSs + (16 * qt + fr) * SS + 32 * kc + 8 * g);
        bf16x8 b = tr8(Kt, TS, 32 * kc + 4 * g + qq, 32 * kc + 16 + 4 * g + qq, 16 * t + 4 * pc);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int qi = q0 + 16 * qt + 4 * g + i;
        if (qi >= L) continue;
        const long row = (long)n * L + qi;
        if (direct_dq)
          dqkv[row * C3 + h * D + 16 * t + fr] = (bf16)(acc[i] * scale);
        else
          slab[row * C + h * D + 16 * t + fr] = acc[i] * scale;
      }
    }
  }
  // dk[t][i] = dK[key 16 kgp + 4g + i][d = 128 half + 16t + fr]
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int kk = k0 + 16 * kgp + 4 * g + i;
      if (kk >= L) continue;
      const long row = (long)nkv * L + kk;
      const int col = h * D + 128 * half + 16 * t + fr;
      dqkv[row * C3 + C + col] = (bf16)(dk[t][i] * scale);
      dqkv[row * C3 + 2 * C + col] = (bf16)dv[t][i];
    }
}

// dQ = sum over the kb key-block slabs (fixed order) -> bf16 q-columns of dqkv
__global__ void dq_sum_k(const float* __restrict__ dq, bf16* __restrict__ dqkv, long rows, int C, int kb) {
  const long total = rows * C / 8, slab = rows * C;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    long r = (i * 8) / C;
    int c = (int)((i * 8) % C);
    f32x8 s = ld8f(dq + i * 8);
    for (int k = 1; k < kb; ++k) s += ld8f(dq + k * slab + i * 8);
    st8(dqkv + r * 3L * C + c, s);
  }
}

// head dim of a shape this file serves, else 0
int hd_dim(int C, int heads) {
  if (heads < 1 || C < 1 || C % heads) return 0;
  const int D = C / heads;
  return D == 32 || D == 256 ? D : 0;
}

// a kernel's dynamic-LDS limit, raised once per process
template <typename K>
hipError_t lds_limit(K kernel, int bytes) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

}  // namespace

// qkv: [N, L, 3C] bf16; out: [N, L, C] bf16; lse: [N, heads, L] fp32.
// D = C/heads in {32, 256}; any L >= 1 (ragged blocks are masked).
D3D_API int d3d_attn_hd_fwd(const void* qkv, void* out, float* lse, int N, int L, int C, int heads, int cross,
                            float scale, hipStream_t st) {
  const int D = hd_dim(C, heads);
  if (D == 0 || L < 1 || N < 1) return (int)hipErrorInvalidValue;
  if (D == 32)
    hipLaunchKernelGGL(attn32_fwd_k, dim3((L + 63) / 64, (heads + 1) / 2, N), dim3(512), 0, st, (const bf16*)qkv,
                       (bf16*)out, lse, L, C, heads, cross, scale);
  else
    hipLaunchKernelGGL(attn256_fwd_k, dim3((L + 63) / 64, heads, N), dim3(256), 0, st, (const bf16*)qkv, (bf16*)out,
                       lse, L, C, heads, cross, scale);
  return (int)hipGetLastError();
}

// fp32 dQ slabs d3d_attn_hd_bwd needs for this shape (0: dQ is written
// directly: L <= 256 at head dim 32, L <= 64 at head dim 256)
D3D_API int d3d_attn_hd_bwd_slabs(int N, int L, int C, int heads) {
  const int D = hd_dim(C, heads);
  if (D == 0 || L <= 64 || (D == 32 && L <= 256)) return 0;
  return (L + 63) / 64;
}

// dq_acc: [d3d_attn_hd_bwd_slabs(...), N, L, C] fp32 workspace (one slab per
// 64-key block, fully written; may be null when no slab is needed); dqkv:
// [N, L, 3C] bf16 output (every element written).
D3D_API int d3d_attn_hd_bwd(const void* qkv, const void* out, const void* dout, const float* lse, float* dq_acc,
                            void* dqkv, int N, int L, int C, int heads, int cross, float scale, hipStream_t st) {
  const int D = hd_dim(C, heads);
  const int slabs = d3d_attn_hd_bwd_slabs(N, L, C, heads);
  if (D == 0 || L < 1 || N < 1 || (slabs > 0 && dq_acc == nullptr)) return (int)hipErrorInvalidValue;
  const int kblocks = (L + 63) / 64;
  if (D == 32 && L > 64 && L <= 256) {
    static const hipError_t once = lds_limit(attn32_bwd_k<256>, attn32_bwd_lds<256>());
    if (once != hipSuccess) return (int)once;
    hipLaunchKernelGGL(attn32_bwd_k<256>, dim3(1, (heads + 1) / 2, N), dim3(512), attn32_bwd_lds<256>(), st,
                       (const bf16*)qkv, (const bf16*)dout, lse, (const bf16*)out, dq_acc, (bf16*)dqkv, L, C, heads,
                       cross, scale);
    return (int)hipGetLastError();
  }
  if (D == 32) {
    hipLaunchKernelGGL(attn32_bwd_k<64>, dim3(kblocks, (heads + 1) / 2, N), dim3(512), attn32_bwd_lds<64>(), st,
                       (const bf16*)qkv, (const bf16*)dout, lse, (const bf16*)out, dq_acc, (bf16*)dqkv, L, C, heads,
                       cross, scale);
  } else {
    static const hipError_t once = lds_limit(attn256_bwd_k, ATTN256_BWD_LDS);
    if (once != hipSuccess) return (int)once;
    hipLaunchKernelGGL(attn256_bwd_k, dim3(kblocks, heads, N), dim3(512), ATTN256_BWD_LDS, st, (const bf16*)qkv,
                       (const bf16*)dout, lse, (const bf16*)out, dq_acc, (bf16*)dqkv, L, C, heads, cross, scale);
  }
  if (slabs == 0) return (int)hipGetLastError();
  const long rows = (long)N * L;
  long g = (rows * C / 8 + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(dq_sum_k, dim3((int)g), dim3(256), 0, st, dq_acc, (bf16*)dqkv, rows, C, kblocks);
  return (int)hipGetLastError();
}
