// Exact k-nearest-neighbour search between two image sets in 8-bit pixel space
// on the int8 matrix units (ops.image_knn; the torch form and the rule's oracle
// is torch_impl.image_knn).  The primitive under improved precision / recall,
// density / coverage and the nearest-training-image (memorisation) check; the
// N x M distance matrix never exists.
//
// Inputs: a [N,3,H,W] (queries), b [M,3,H,W] (candidates), each fp32 in [-1, 1]
// or uint8; k in 1 .. 8; exclude_self; radius int64 [M] or none.  D = 3 H W.
//  1. Map.  fp32 goes through u = metric_map_u8(x) (image_map.h), the byte a PNG
//     writer stores; uint8 is taken as it is.
//  2. Distance.  d2(i, j) = sum_p (u_a[i,p] - u_b[j,p])^2, an integer in units
//     of (1/255)^2.  With s = u - 128 (a translation: distances do not change)
//     the values are int8 and d2 = |s_a|^2 + |s_b|^2 - 2 s_a . s_b exactly:
//     |s_a . s_b| <= D 2^14 and |s|^2 <= D 2^14, so D <= 131071 keeps the int32
//     accumulators and the int32 norms below 2^31; d2 itself needs 64 bits
//     (3 128 128 255^2 = 3.2e9) and is formed in int64.
//  3. Order.  Candidates are ranked by the total order on (d2, j): equal
//     distances go to the lower index.  Kernels carry a candidate as ONE
//     unsigned 64-bit key (d2 << 31) | j -- d2 <= 131071 255^2 < 2^33 and
//     j < 2^31, so the key fits (a shift of 32 would not) and is below the
//     all-ones sentinel of an empty slot.  The order is total, so the k
//     smallest keys do not depend on how the candidates were split or merged.
//  4. Output.  d2 [N,k] and idx [N,k] int64, ascending in that order.
//     exclude_self skips j == i.  With radius: inside[i] = #{j : d2(i, j) <=
//     radius[j]} over ALL M candidates (exclude_self honoured); radius -1 is
//     never inside because d2 >= 0.
//
// Kernels (no atomics; integer arithmetic only: exact and bitwise reproducible):
//  * knn_pack_k: one workgroup per panel row.  Maps a set to the int8 panel
//    [rows_p, Dp] (for uint8 input that is a flip of the top bit) and writes the
//    row's int32 squared norm.  Dp is D rounded up to the 128-byte LDS stage
//    (two 64-byte MFMA K steps), rows_p is rows rounded up to whole tiles
//    (d3d_knn_rows); the padding is 0, which adds nothing to a dot product or a
//    norm, so the distance kernel loads whole tiles without a bounds check.
//  * knn_dist_k<NW, KK, RADIUS>, grid (query tiles, splits of M), NW waves.
//    A workgroup holds 32 NW queries (256 with 8 waves: in the evaluation use,
//    a few hundred queries against up to 1e5 candidates, one workgroup covers
//    all or most queries, so b, the HBM stream, is read once or twice; the
//    split over M is what fills the chip) and sweeps its range of candidates in
//    column tiles of 64.  Per stage 128 K-bytes of both tiles go global ->
//    registers -> LDS (the next stage's loads are in flight under the MFMAs;
//    rows are 144 bytes apart in LDS so that a fragment read of 16 rows x 16
//    bytes touches every bank once).  v_mfma_i32_16x16x64_i8 with the
//    CANDIDATES as the A operand and the QUERIES as the B operand: the
//    accumulator of lane l then holds candidates 4 (l / 16) + r, r = 0 .. 3, of
//    ONE query l % 16 (the accumulator layout of mfma_gemm.h: rows on the
//    registers, columns on the lanes).  Integer addition is associative and
//    both operands are read with the same lane -> K-byte assignment, so which
//    16 of the 64 K-bytes a lane group holds does not matter.  A wave owns 2 x
//    16 queries against all 4 x 16 candidates of the tile: 32 accumulator
//    registers, and per lane TWO running top-KK lists (KK = 1 for k = 1, else
//    8) of keys in registers over the whole sweep.  Epilogue per column tile in
//    int64: d2 = n_a + n_b - 2 dot; columns past M and the diagonal are masked
//    by the global indices to the sentinel; a candidate fails one unsigned
//    compare against the list's last key or is inserted by a register shift;
//    `inside` is a per-lane count.  At the end of the sweep the four lanes that
//    hold a query merge their lists by two cross-lane exchanges (lane ^ 16,
//    lane ^ 32; no wave shares a query with another, so LDS is not needed) and
//    one of them writes keys [split, N, k] and counts [split, N].
//  * knn_merge_k: one thread per query merges the splits' lists in the same
//    order and adds the counts.
// Every launch takes pointers and constants only: graph-capturable.
#include "image_map.h"

#define KNN_QW 2          // 16-query subtiles per wave
#define KNN_CT 64         // candidates per column tile (4 subtiles of 16)
#define KNN_KC 128        // K bytes per LDS stage
#define KNN_LD 144        // LDS row stride in bytes
#define KNN_KMAX 8
#define KNN_SHIFT 31
#define KNN_MAX_D 131071

typedef int knn_i4 __attribute__((ext_vector_type(4)));
typedef unsigned long long knn_u64;

namespace {

constexpr knn_u64 KNN_EMPTY = ~0ull;

// keep the KK smallest keys, ascending: almost every key fails the first compare
template <int KK>
__device__ __forceinline__ void knn_insert(knn_u64 (&t)[KK], knn_u64 key) {
  if (key < t[KK - 1]) {
#pragma unroll
    for (int i = KK - 1; i > 0; --i) t[i] = key < t[i - 1] ? t[i - 1] : (key < t[i] ? key : t[i]);
    t[0] = key < t[0] ? key : t[0];
  }
}

// x: fp32 or uint8 [rows, D]; panel int8 [rows_p, Dp]; norm int32 [rows_p].  grid rows_p, 256 threads.
__global__ __launch_bounds__(256) void knn_pack_k(const void* __restrict__ x, int is_u8, int rows, int D, int Dp,
                                                  unsigned* __restrict__ panel, int* __restrict__ norm) {
  __shared__ int red[4];
  const int r = blockIdx.x, tid = threadIdx.x;
  const bool live = r < rows;
  const float* xf = reinterpret_cast<const float*>(x) + (size_t)r * D;
  const unsigned char* xu = reinterpret_cast<const unsigned char*>(x) + (size_t)r * D;
  unsigned* out = panel + (size_t)r * (Dp / 4);
  int acc = 0;
  for (int w = tid; w < Dp / 4; w += 256) {
    unsigned word = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int p = 4 * w + e;
      int s = 0;
      if (live && p < D) s = (is_u8 ? (int)xu[p] : metric_map_u8(xf[p])) - 128;
      acc += s * s;
      word |= (unsigned)(s & 0xff) << (8 * e);
    }
    out[w] = word;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) norm[r] = red[0] + red[1] + red[2] + red[3];
}

// the 16-byte chunks of one stage that this thread moves: chunk c = tid + i T is row c / 8, bytes 16 (c % 8) ..
template <int T, int CQ, int CC>
__device__ __forceinline__ void knn_fetch(const int8_t* __restrict__ pa, const int8_t* __restrict__ pb, size_t Dp,
                                          int q0, int tile, int kc, int tid, knn_i4 (&rq)[CQ], knn_i4 (&rc)[CC]) {
#pragma unroll
  for (int i = 0; i < CQ; ++i) {
    const int c = tid + i * T;
    rq[i] = *reinterpret_cast<const knn_i4*>(pa + (size_t)(q0 + (c >> 3)) * Dp + (size_t)kc * KNN_KC + (c & 7) * 16);
  }
#pragma unroll
  for (int i = 0; i < CC; ++i) {
    const int c = tid + i * T;
    rc[i] = *reinterpret_cast<const knn_i4*>(pb + (size_t)(tile * KNN_CT + (c >> 3)) * Dp + (size_t)kc * KNN_KC +
                                             (c & 7) * 16);
  }
}

// pa int8 [rows_p(N), Dp], na int32 [rows_p(N)], pb / nb the same for M; radius int64 [M] (RADIUS);
// keys [S, N, k], cnt [S, N] (RADIUS).  Split s sweeps column tiles s tps .. min((s + 1) tps, tiles) - 1.
template <int NW, int KK, bool RADIUS>
__global__ __launch_bounds__(64 * NW) void knn_dist_k(const int8_t* __restrict__ pa, const int* __restrict__ na,
                                                      const int8_t* __restrict__ pb, const int* __restrict__ nb,
                                                      const long long* __restrict__ radius, int N, int M, int Dp,
                                                      int tps, int excl, int k, knn_u64* __restrict__ keys,
                                                      long long* __restrict__ cnt) {
  constexpr int T = 64 * NW, QT = KNN_QW * 16 * NW, CQ = QT * 8 / T, CC = KNN_CT * 8 / T;
  static_assert(CQ * T == QT * 8 && CC * T == KNN_CT * 8, "a stage is a whole number of chunks per thread");
  __shared__ __attribute__((aligned(16))) int8_t lds[(QT + KNN_CT) * KNN_LD];
  int8_t* sq = lds;
  int8_t* sc = lds + QT * KNN_LD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * QT, split = blockIdx.y;
  const int ntiles = (M + KNN_CT - 1) / KNN_CT;
  const int t0 = split * tps, t1 = min(ntiles, t0 + tps);
  const int nK = Dp / KNN_KC;

  knn_u64 best[KNN_QW][KK];
  long long inside[KNN_QW];
  int qi[KNN_QW], naq[KNN_QW];
  knn_i4 acc[KNN_QW][4];
#pragma unroll
  for (int q = 0; q < KNN_QW; ++q) {
    qi[q] = q0 + (wave * KNN_QW + q) * 16 + fr;
    naq[q] = na[qi[q]];
    inside[q] = 0;
#pragma unroll
    for (int i = 0; i < KK; ++i) best[q][i] = KNN_EMPTY;
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[q][c] = knn_i4{0, 0, 0, 0};
  }

  knn_i4 rq[CQ], rc[CC];
  int tile = t0, kc = 0;
  if (tile < t1) knn_fetch<T, CQ, CC>(pa, pb, (size_t)Dp, q0, tile, kc, tid, rq, rc);
  while (tile < t1) {
    __syncthreads();                               // the previous stage's fragments have been read
#pragma unroll
    for (int i = 0; i < CQ; ++i) {
      const int c = tid + i * T;
      *reinterpret_cast<knn_i4*>(sq + (c >> 3) * KNN_LD + (c & 7) * 16) = rq[i];
    }
#pragma unroll
    for (int i = 0; i < CC; ++i) {
      const int c = tid + i * T;
      *reinterpret_cast<knn_i4*>(sc + (c >> 3) * KNN_LD + (c & 7) * 16) = rc[i];
    }
    __syncthreads();
    int ntile = tile, nkc = kc + 1;
    if (nkc == nK) {
      nkc = 0;
      ++ntile;
    }
    if (ntile < t1) knn_fetch<T, CQ, CC>(pa, pb, (size_t)Dp, q0, ntile, nkc, tid, rq, rc);

#pragma unroll
    for (int ks = 0; ks < KNN_KC / 64; ++ks) {
      knn_i4 fq[KNN_QW], fc[4];
#pragma unroll
      for (int q = 0; q < KNN_QW; ++q)
        fq[q] = *reinterpret_cast<const knn_i4*>(sq + ((wave * KNN_QW + q) * 16 + fr) * KNN_LD + ks * 64 + g * 16);
#pragma unroll
      for (int c = 0; c < 4; ++c)
        fc[c] = *reinterpret_cast<const knn_i4*>(sc + (c * 16 + fr) * KNN_LD + ks * 64 + g * 16);
#pragma unroll
      for (int q = 0; q < KNN_QW; ++q)
#pragma unroll
        for (int c = 0; c < 4; ++c)
          acc[q][c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fc[c], fq[q], acc[q][c], 0, 0, 0);
    }

    if (kc == nK - 1) {                            // the tile's dot products are complete
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int jb = tile * KNN_CT + c * 16 + 4 * g;
        const knn_i4 nbv = *reinterpret_cast<const knn_i4*>(nb + jb);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = jb + r;
          long long rad = -1;
          if (RADIUS && j < M) rad = radius[j];
#pragma unroll
          for (int q = 0; q < KNN_QW; ++q) {
            const long long d2 = (long long)naq[q] + (long long)nbv[r] - 2ll * (long long)acc[q][c][r];
            const bool ok = j < M && !(excl && j == qi[q]);
            if (RADIUS) inside[q] += (ok && d2 <= rad) ? 1 : 0;
            knn_insert<KK>(best[q], ok ? (((knn_u64)d2 << KNN_SHIFT) | (knn_u64)j) : KNN_EMPTY);
          }
        }
#pragma unroll
        for (int q = 0; q < KNN_QW; ++q) acc[q][c] = knn_i4{0, 0, 0, 0};
      }
    }
    tile = ntile;
    kc = nkc;
  }

  // the four lanes of a query (g = 0 .. 3) merge; afterwards all four hold the same list and count
#pragma unroll
  for (int q = 0; q < KNN_QW; ++q) {
#pragma unroll
    for (int m = 16; m <= 32; m <<= 1) {
      knn_u64 other[KK];
#pragma unroll
      for (int i = 0; i < KK; ++i) other[i] = __shfl_xor(best[q][i], m, 64);
#pragma unroll
      for (int i = 0; i < KK; ++i) knn_insert<KK>(best[q], other[i]);
      if (RADIUS) inside[q] += __shfl_xor(inside[q], m, 64);
    }
    if (g == 0 && qi[q] < N) {
      const size_t row = (size_t)split * N + qi[q];
#pragma unroll
      for (int i = 0; i < KK; ++i)
        if (i < k) keys[row * k + i] = best[q][i];
      if (RADIUS) cnt[row] = inside[q];
    }
  }
}

// keys [S, N, k], cnt [S, N] or null -> d2, idx [N, k], inside [N] or null.  One thread per query.
__global__ __launch_bounds__(64) void knn_merge_k(const knn_u64* __restrict__ keys, const long long* __restrict__ cnt,
                                                  int N, int S, int k, long long* __restrict__ d2,
                                                  long long* __restrict__ idx, long long* __restrict__ inside) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= N) return;
  knn_u64 best[KNN_KMAX];
#pragma unroll
  for (int i = 0; i < KNN_KMAX; ++i) best[i] = KNN_EMPTY;
  long long c = 0;
  for (int s = 0; s < S; ++s) {
    const size_t row = (size_t)s * N + q;
    for (int i = 0; i < k; ++i) knn_insert<KNN_KMAX>(best, keys[row * k + i]);
    if (cnt != nullptr) c += cnt[row];
  }
#pragma unroll
  for (int i = 0; i < KNN_KMAX; ++i)
    if (i < k) {
      d2[(size_t)q * k + i] = (long long)(best[i] >> KNN_SHIFT);
      idx[(size_t)q * k + i] = (long long)(best[i] & ((1ull << KNN_SHIFT) - 1ull));
    }
  if (inside != nullptr) inside[q] = c;
}

// waves of the distance kernel for n queries: 32 queries a wave, 1 / 2 / 4 / 8 waves
int knn_waves(long n) { return n <= 32 ? 1 : n <= 64 ? 2 : n <= 128 ? 4 : 8; }

// column tiles per split: about two workgroups per compute unit, or `splits` of them when it is given
int knn_tiles_per_split(long N, long M, int splits) {
  const long tiles = (M + KNN_CT - 1) / KNN_CT, qtiles = (N + 32 * knn_waves(N) - 1) / (32 * knn_waves(N));
  long want = splits > 0 ? splits : (2 * (long)device_cus() + qtiles - 1) / qtiles;
  want = want < 1 ? 1 : (want > tiles ? tiles : want);
  return (int)((tiles + want - 1) / want);
}

template <int NW, int KK>
void knn_dist_launch(bool rad, dim3 grid, hipStream_t st, const int8_t* pa, const int* na, const int8_t* pb,
                     const int* nb, const long long* radius, int N, int M, int Dp, int tps, int excl, int k,
                     knn_u64* keys, long long* cnt) {
  if (rad)
    hipLaunchKernelGGL((knn_dist_k<NW, KK, true>), grid, dim3(64 * NW), 0, st, pa, na, pb, nb, radius, N, M, Dp, tps,
                       excl, k, keys, cnt);
  else
    hipLaunchKernelGGL((knn_dist_k<NW, KK, false>), grid, dim3(64 * NW), 0, st, pa, na, pb, nb, radius, N, M, Dp, tps,
                       excl, k, keys, cnt);
}
template <int NW>
void knn_dist_launch_k(int k, bool rad, dim3 grid, hipStream_t st, const int8_t* pa, const int* na, const int8_t* pb,
                       const int* nb, const long long* radius, int N, int M, int Dp, int tps, int excl, knn_u64* keys,
                       long long* cnt) {
  if (k == 1)
    knn_dist_launch<NW, 1>(rad, grid, st, pa, na, pb, nb, radius, N, M, Dp, tps, excl, k, keys, cnt);
  else
    knn_dist_launch<NW, KNN_KMAX>(rad, grid, st, pa, na, pb, nb, radius, N, M, Dp, tps, excl, k, keys, cnt);
}
}  // namespace

// rows of the packed panel of a set of n images: n rounded up to whole query and column tiles
D3D_API long d3d_knn_rows(long n) {
  const long tile = 32 * knn_waves(n) > KNN_CT ? 32 * knn_waves(n) : KNN_CT;
  return (n + tile - 1) / tile * tile;
}

// the number of splits of M the search of N queries among M candidates takes (`splits` > 0: at most that many)
D3D_API int d3d_knn_splits(long N, long M, int splits) {
  if (N < 1 || M < 1) return 0;
  const long tiles = (M + KNN_CT - 1) / KNN_CT;
  const int tps = knn_tiles_per_split(N, M, splits);
  return (int)((tiles + tps - 1) / tps);
}

// a [N, D], b [M, D] (fp32, or uint8 where a_u8 / b_u8); b == a with the same kind packs once.  radius int64 [M] or
// null.  Workspaces, all fully written before they are read: pa int8 [d3d_knn_rows(N), Dp], na int32
// [d3d_knn_rows(N)], pb / nb the same for M (unused where b == a), Dp = D rounded up to 128; keys [S, N, k] and cnt
// [S, N] 64-bit with S = d3d_knn_splits(N, M, splits).  Outputs d2, idx int64 [N, k], inside int64 [N] (with radius).
D3D_API int d3d_image_knn(const void* a, int a_u8, const void* b, int b_u8, long N, long M, long D, int k, int excl,
                          const long long* radius, int splits, int8_t* pa, int* na, int8_t* pb, int* nb,
                          knn_u64* keys, long long* cnt, long long* d2, long long* idx, long long* inside,
                          hipStream_t st) {
  const bool same = a == b && (a_u8 != 0) == (b_u8 != 0) && N == M;
  const bool rad = radius != nullptr;
  if (a == nullptr || b == nullptr || pa == nullptr || na == nullptr || keys == nullptr || d2 == nullptr ||
      idx == nullptr || (!same && (pb == nullptr || nb == nullptr)) || (rad && (cnt == nullptr || inside == nullptr)))
    return (int)hipErrorInvalidValue;
  if (N < 1 || M < 1 || D < 1 || D > KNN_MAX_D || k < 1 || k > KNN_KMAX || k > M - (excl ? 1 : 0) ||
      N >= (1l << KNN_SHIFT) || M >= (1l << KNN_SHIFT))
    return (int)hipErrorInvalidValue;
  const int Dp = (int)((D + KNN_KC - 1) / KNN_KC * KNN_KC);
  hipLaunchKernelGGL(knn_pack_k, dim3((unsigned)d3d_knn_rows(N)), dim3(256), 0, st, a, a_u8, (int)N, (int)D, Dp,
                     reinterpret_cast<unsigned*>(pa), na);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  if (same) {
    pb = pa;
    nb = na;
  } else {
    hipLaunchKernelGGL(knn_pack_k, dim3((unsigned)d3d_knn_rows(M)), dim3(256), 0, st, b, b_u8, (int)M, (int)D, Dp,
                       reinterpret_cast<unsigned*>(pb), nb);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  const int nw = knn_waves(N), tps = knn_tiles_per_split(N, M, splits), S = d3d_knn_splits(N, M, splits);
  const dim3 grid((unsigned)((N + 32 * nw - 1) / (32 * nw)), (unsigned)S);
  if (grid.y > 65535u) return (int)hipErrorInvalidValue;
  if (nw == 1)
    knn_dist_launch_k<1>(k, rad, grid, st, pa, na, pb, nb, radius, (int)N, (int)M, Dp, tps, excl, keys, cnt);
  else if (nw == 2)
    knn_dist_launch_k<2>(k, rad, grid, st, pa, na, pb, nb, radius, (int)N, (int)M, Dp, tps, excl, keys, cnt);
  else if (nw == 4)
    knn_dist_launch_k<4>(k, rad, grid, st, pa, na, pb, nb, radius, (int)N, (int)M, Dp, tps, excl, keys, cnt);
  else
    knn_dist_launch_k<8>(k, rad, grid, st, pa, na, pb, nb, radius, (int)N, (int)M, Dp, tps, excl, keys, cnt);
  e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(knn_merge_k, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, st, (const knn_u64*)keys,
                     (const long long*)(rad ? cnt : nullptr), (int)N, S, k, d2, idx, rad ? inside : nullptr);
  return (int)hipGetLastError();
}
