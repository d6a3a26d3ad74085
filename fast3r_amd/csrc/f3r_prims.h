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

// ---- the 8-bit colour of an image value (scene, sky and mesh form (img + 1) * 127.5 themselves)
__device__ __forceinline__ uint8_t sat_u8(float y) {  // truncation to uint8; below 0 and NaN -> 0, above 255 -> 255
  if (!(y > 0.f)) return 0;
  if (y >= 255.f) return 255;
  return (uint8_t)(int)y;
}

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
