// Wave and block primitives of the post-processing kernels (f3r_post.hip, f3r_pnp.hip, f3r_recon.hip, f3r_pose_metric.hip, f3r_loss.hip,
// f3r_scene.hip): one copy of every reduction, rank and search whose fixed order their bit-exact, run-to-run identical outputs rest on.
// Header-only: inline device functions, templates and one kernel template with internal linkage.  A wave is 64 lanes.
//
// The order contract.  Nothing here depends on arrival order; what a floating-point sum adds, it adds in this order:
//   * wave_sum is the xor butterfly with offsets 32, 16, .., 1.  Lane 0 ends with the tree ((l0 + l32) + (l16 + l48)) + ...; a butterfly of
//     __shfl_down leaves the same tree in lane 0, because fp addition is commutative and each level pairs the same partial sums.  Other
//     lanes hold the same 64 values added in other orders: callers store or broadcast lane 0's value only, never "any lane".
//   * block_sum adds lane 0's value of wave 0, 1, .., NT / 64 - 1 in that order, starting from +0.0.  Starting from wave 0's value instead
//     differs only when that value is -0.0.  It never is: rounding to nearest, x + y is -0.0 only when x and y both are, and every per-thread
//     accumulator that feeds a block_sum (the moment sums of align, focal, PnP and the registration, the statistics partials, both loss
//     passes) starts at +0.0, so neither a thread's value nor a wave's sum can be -0.0.  A new caller keeps to that.
//   * digit_peers and compact_rank rank lanes in lane order, and exclusive_scan_rows_kernel is integer arithmetic: slots never depend on
//     which lane or workgroup ran first.
//   * tile_count adds integers, and tile_compact walks a tile in ascending 64-element steps and ranks with compact_rank: the slot of a kept
//     element is the scanned count of the tiles before its own plus the number of kept elements before it in its tile, nothing else.
#pragma once

#include <type_traits>

#include "f3r_carve.h"
#include "f3r_common.h"

// ---- order-preserving integer keys: a < b as numbers <=> key(a) < key(b) as unsigned integers (-0.0 < +0.0, NaNs beyond the infinities)
__host__ __device__ __forceinline__ uint32_t fkey(float f) {
  const uint32_t u = __builtin_bit_cast(uint32_t, f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ __forceinline__ float fkey_inv(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  return __builtin_bit_cast(float, u);
}
__device__ __forceinline__ uint64_t dkey(double v) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double dkey_inv(uint64_t k) {
  const uint64_t u = (k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k;
  return __builtin_bit_cast(double, u);
}

// ---- the 8-bit colour of an image value
__device__ __forceinline__ uint8_t sat_u8(float y) {  // truncation to uint8; below 0 and NaN -> 0, above 255 -> 255
  if (!(y > 0.f)) return 0;
  if (y >= 255.f) return 255;
  return (uint8_t)(int)y;
}
// the colour line of an image value in [-1, 1]: an add and a multiply, each rounded (every file that calls it is built with -ffp-contract=off)
__device__ __forceinline__ uint8_t colour_u8(float v) { return sat_u8((v + 1.0f) * 127.5f); }

// ---- ballots
__device__ __forceinline__ uint64_t lanes_below() { return (1ull << (threadIdx.x & 63)) - 1ull; }

// the lanes with ok set whose 8-bit digit equals this lane's (one ballot per bit); every lane of the wave calls it
__device__ __forceinline__ uint64_t digit_peers(uint32_t d, bool ok) {
  uint64_t peers = __ballot(ok);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (d >> b) & 1u;
    const uint64_t bal = __ballot(bit);
    peers &= bit ? bal : ~bal;
  }
  return peers;
}

__device__ __forceinline__ uint32_t wave_flag_count(bool flag) { return (uint32_t)__popcll(__ballot(flag)); }

// *counter += the wave's count of flag: one integer atomic per wave, none when the count is zero
template <class C>
__device__ __forceinline__ void wave_count_add(bool flag, C* counter) {
  const uint32_t n = wave_flag_count(flag);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(counter, (C)n);
}

// one step of an ordered compaction: this lane's rank among the lanes of its wave that keep; ballot = those lanes (its popcount advances
// the caller's running base)
__device__ __forceinline__ uint32_t compact_rank(bool keep, uint64_t& ballot) {
  ballot = __ballot(keep);
  return (uint32_t)__popcll(ballot & lanes_below());
}

// ---- the last s in [lo, hi) with start[s] <= x, for start ascending and start[lo] <= x: the segment that owns tile or pixel x
template <class I>
__device__ __forceinline__ int last_le(const I* __restrict__ start, int lo, int hi, std::common_type_t<I> x) {
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (start[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

// ---- its mirror image: the first position in [lo, hi) with keys[position] >= want, or hi if there is none, for keys ascending: where the
//      run of a key starts in a sorted array
template <class K>
__device__ __forceinline__ int64_t first_ge(const K* __restrict__ keys, int64_t lo, int64_t hi, std::common_type_t<K> want) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < want) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- sums (see the order contract above)
template <class T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// out[j] = the sum of v[j] over the NT threads of the workgroup, j < N.  red: the caller's LDS, NT / 64 rows of LD >= N; out: LDS or
// global.  Every thread calls it; on return out[] is visible to all of them and red may be reused.
template <int N, int NT, int LD>
__device__ __forceinline__ void block_sum(const double* v, double (*red)[LD], double* out) {
  static_assert(N <= LD && N <= NT && NT % 64 == 0, "block_sum: shape");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const double a = wave_sum(v[j]);
    if (lane == 0) red[wv][j] = a;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    double s = 0.0;
    for (int w = 0; w < NT / 64; ++w) s += red[w][threadIdx.x];
    out[threadIdx.x] = s;
  }
  __syncthreads();
}

// ---- the tile walk of an ordered compaction with K streams (1 or 2), called by one wave.  The tile is the elements [base, stop),
// stop = min(base + TILE, end).  flags(i) gives an in-range element's mask, once per element per kernel: bit k set = kept in stream k; bits
// K and up are the caller's and travel to emit untouched.  Lanes at or past stop have mask 0 and never call flags.
// Count kernel, scan of the counts, then tile_compact with run[k] = the scanned count: that is the whole compaction.
//
// n[k] = the tile's kept elements of stream k, in every lane.  Each lane counts its own elements and one wave_sum adds the lanes: integer
// sums, the same number as a ballot count per step, and the lanes' loads do not wait for one another.
template <int TILE, int K, class Flags>
__device__ __forceinline__ void tile_count(int64_t base, int64_t end, Flags flags, uint32_t (&n)[K]) {
  static_assert(TILE % 64 == 0 && (K == 1 || K == 2), "tile_count: whole waves, one or two streams");
  const int64_t stop = min(base + (int64_t)TILE, end);
#pragma unroll
  for (int k = 0; k < K; ++k) n[k] = 0;
  for (int64_t i = base + (threadIdx.x & 63); i < stop; i += 64) {
    const uint32_t m = (uint32_t)flags(i);
#pragma unroll
    for (int k = 0; k < K; ++k) n[k] += (m >> k) & 1u;
  }
#pragma unroll
  for (int k = 0; k < K; ++k) n[k] = wave_sum(n[k]);
}

// The steps c = base, base + 64, .. < stop in ascending order.  emit(i, mask, slots) runs on the lanes with a stream bit set: slots[k] =
// run[k] + the lane's rank among the tile's keepers of stream k so far, meaningful where mask bit k is set.  A lane's emit follows its
// flags of the same step directly, before any later flags: a kernel may leave what flags looked up in a local for emit (mesh_face_kernel,
// mv_write_kernel).  On return run[k] has advanced by the tile's count.  S: the caller's slot type.
template <int TILE, int K, class S, class Flags, class Emit>
__device__ __forceinline__ void tile_compact(int64_t base, int64_t end, S (&run)[K], Flags flags, Emit emit) {
  static_assert(TILE % 64 == 0 && (K == 1 || K == 2), "tile_compact: whole waves, one or two streams");
  const int64_t stop = min(base + (int64_t)TILE, end);
  const auto step = [&](int64_t c) {
    const int64_t i = c + (threadIdx.x & 63);
    const uint32_t m = i < stop ? (uint32_t)flags(i) : 0u;
    S slots[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      uint64_t bal;
      slots[k] = run[k] + (S)compact_rank((m >> k) & 1u, bal);
      run[k] += (S)__popcll(bal);
    }
    if (m & ((1u << K) - 1u)) emit(i, m, slots);
  };
  if (stop - base == TILE) {  // a full tile has a constant trip count, as the fixed-step kernels had: the compiler unrolls a small step
    for (int s = 0; s < TILE / 64; ++s) step(base + s * 64);
  } else {
    for (int64_t c = base; c < stop; c += 64) step(c);
  }
}

// ---- minima and maxima of integers (for floats: of their order-preserving keys).  Order-free: every tree gives the same value.
template <class T>
__device__ __forceinline__ T wave_min(T x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = min(x, (T)__shfl_xor(x, off, 64));
  return x;
}
template <class T>
__device__ __forceinline__ T wave_max(T x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = max(x, (T)__shfl_xor(x, off, 64));
  return x;
}

// lo = the minimum of lo, hi = the maximum of hi over the NT threads of the workgroup, valid in thread 0 on return.  red: the caller's LDS,
// NT / 64 rows.  Every thread calls it; red may be reused on return.
template <int NT>
__device__ __forceinline__ void block_min_max(uint32_t& lo, uint32_t& hi, uint32_t (*red)[2]) {
  static_assert(NT % 64 == 0, "block_min_max: shape");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  lo = wave_min(lo);
  hi = wave_max(hi);
  if (lane == 0) {
    red[wv][0] = lo;
    red[wv][1] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < NT / 64; ++w) {
      lo = min(lo, red[w][0]);
      hi = max(hi, red[w][1]);
    }
  }
  __syncthreads();
}

// ---- exclusive scan, in place, of row blockIdx.x: uint32 a[start(row) .. start(row) + len(row)); totals[row] = its sum (if totals).
// With ts: row = segment, start = 256 ts[row], len = 256 (ts[row + 1] - ts[row]); without: dense rows of len0, start = row * len0.
// One workgroup of SCAN_NT threads per row.  A template so that only the files that launch it carry a copy.
constexpr int SCAN_NT = 1024;
template <int NT>
static __global__ __launch_bounds__(NT) void exclusive_scan_rows_kernel(uint32_t* __restrict__ a, const int64_t* __restrict__ ts, int64_t len0,
                                                                        uint32_t* __restrict__ totals) {
  __shared__ uint32_t sh[NT];
  const int64_t start = ts ? ts[blockIdx.x] * 256 : (int64_t)blockIdx.x * len0;
  const int64_t len = ts ? (ts[blockIdx.x + 1] - ts[blockIdx.x]) * 256 : len0;
  uint32_t* r = a + start;
  const int64_t per = (len + NT - 1) / NT;
  const int64_t b0 = min((int64_t)threadIdx.x * per, len), b1 = min(b0 + per, len);
  uint32_t s = 0;
  for (int64_t i = b0; i < b1; ++i) s += r[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int off = 1; off < NT; off <<= 1) {
    const uint32_t t = threadIdx.x >= (unsigned)off ? sh[threadIdx.x - off] : 0u;
    __syncthreads();
    sh[threadIdx.x] += t;
    __syncthreads();
  }
  uint32_t run = sh[threadIdx.x] - s;
  for (int64_t i = b0; i < b1; ++i) {
    const uint32_t v = r[i];
    r[i] = run;
    run += v;
  }
  if (threadIdx.x == NT - 1 && totals) totals[blockIdx.x] = sh[NT - 1];
}

// ---- host (align256 and the workspace carver: f3r_carve.h)
inline unsigned blocks_of(int64_t n, int nt) { return (unsigned)((n + nt - 1) / nt); }
