// The stable LSD radix sort of (key, 32-bit value) pairs with 8-bit digits, shared by the voxel downsampler (f3r_cloud.hip), the
// sparsification curves of the depth metrics (f3r_depth.hip), the view matcher's index (f3r_match.hip) -- 64-bit keys, the default -- and the
// nearest-neighbour index and query order of the reconstruction metrics (f3r_recon.hip, 32-bit cell keys): per-tile histograms laid out
// digit-major, a two-level exclusive scan, and a scatter that ranks the keys of a tile in index order with ballots.  Keys of equal digits
// keep their order in every pass, so the sort is stable and its output does not depend on the tile geometry; integer atomics on LDS
// counters only, so two runs give the same bits.  Header-only: kernel templates with internal linkage, so each file that includes it
// carries its own copy, and the host driver that launches them.
#pragma once

#include <algorithm>
#include <utility>

#include "f3r_prims.h"

constexpr int SORT_TILE = 2048;                // keys of one sort workgroup
constexpr int SORT_NT = 256;
constexpr int SORT_WAVES = SORT_NT / 64;
constexpr int SORT_SUB = SORT_TILE / SORT_WAVES;  // consecutive keys owned by one wave
constexpr int SORT_PER = SORT_SUB / 64;
static_assert(SORT_NT == 256, "one thread per digit");

// hist[digit * n_tiles + tile] = keys of the tile with that digit: digit-major, so one flat scan gives every (digit, tile) its first slot
template <class K = uint64_t>
static __global__ __launch_bounds__(SORT_NT) void sort_hist_kernel(const K* __restrict__ keys, int64_t n, int shift,
                                                                   uint32_t* __restrict__ hist, int64_t n_tiles) {
  __shared__ uint32_t cnt[256];
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * SORT_TILE, end = min(base + (int64_t)SORT_TILE, n);
  for (int64_t i = base + threadIdx.x; i < end; i += SORT_NT) atomicAdd(&cnt[(uint32_t)(keys[i] >> shift) & 255u], 1u);
  __syncthreads();
  hist[(int64_t)threadIdx.x * n_tiles + blockIdx.x] = cnt[threadIdx.x];
}

// one stable pass (after the two-level scan of the histogram: rows of row_len words, then the rows' totals): wave w owns keys [sub, sub + SORT_SUB) of the tile and ranks them 64 at a time in lane order; a key's slot is the
// scanned first slot of its (digit, tile), plus the same digit's keys in the waves before, plus its rank within its wave
template <class K = uint64_t>
static __global__ __launch_bounds__(SORT_NT) void sort_scatter_kernel(const K* __restrict__ kin, const uint32_t* __restrict__ vin, int64_t n,
                                                                      int shift, const uint32_t* __restrict__ hist, int64_t n_tiles,
                                                                      const uint32_t* __restrict__ row_base, int64_t row_len,
                                                                      K* __restrict__ kout, uint32_t* __restrict__ vout) {
  __shared__ uint32_t cnt[SORT_WAVES][256];
  __shared__ uint32_t gbase[256];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int64_t base = (int64_t)blockIdx.x * SORT_TILE, end = min(base + (int64_t)SORT_TILE, n);
#pragma unroll
  for (int j = 0; j < SORT_WAVES; ++j) cnt[j][tid] = 0;
  {  // the histogram was scanned in rows of row_len words: a word's slot is its place in its row plus the rows before
    const int64_t h = (int64_t)tid * n_tiles + blockIdx.x;
    gbase[tid] = hist[h] + row_base[h / row_len];
  }
  __syncthreads();
  const int64_t sub = base + (int64_t)w * SORT_SUB;
  K k[SORT_PER];
  uint32_t v[SORT_PER], rk[SORT_PER];
#pragma unroll
  for (int s = 0; s < SORT_PER; ++s) {
    const int64_t i = sub + s * 64 + lane;
    const bool ok = i < end;
    k[s] = ok ? kin[i] : (K)0;
    v[s] = ok ? vin[i] : 0u;
  }
#pragma unroll
  for (int s = 0; s < SORT_PER; ++s) {
    const bool ok = sub + s * 64 + lane < end;
    const uint32_t d = (uint32_t)(k[s] >> shift) & 255u;
    const uint64_t peers = digit_peers(d, ok);
    const uint32_t below = (uint32_t)__popcll(peers & lanes_below());
    // cnt[w] is this wave's alone, and a wave's LDS accesses execute in program order: every lane has read before the leader writes
    const uint32_t c = cnt[w][d];
    if (ok && below == 0) cnt[w][d] = c + (uint32_t)__popcll(peers);
    rk[s] = c + below;
  }
  __syncthreads();
  {  // thread = digit: the waves' counts become exclusive prefixes over the waves
    uint32_t run = gbase[tid];
#pragma unroll
    for (int j = 0; j < SORT_WAVES; ++j) {
      const uint32_t c = cnt[j][tid];
      cnt[j][tid] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < SORT_PER; ++s) {
    if (sub + s * 64 + lane < end) {
      const uint32_t d = (uint32_t)(k[s] >> shift) & 255u;
      const uint32_t o = cnt[w][d] + rk[s];
      kout[o] = k[s];
      vout[o] = v[s];
    }
  }
}

// ---- host
template <class K = uint64_t>
struct SortWs {  // the sort's part of a workspace: two key and two value buffers of n entries, the histogram and its rows' totals
  K *keys_a, *keys_b;
  uint32_t *idx_a, *idx_b, *hist, *row_tot;
  int64_t sort_tiles, hist_rows, hist_row_len;
};

template <class K = uint64_t>
inline SortWs<K> sort_ws(Carve& c, int64_t n) {
  SortWs<K> w = {};
  w.sort_tiles = (n + SORT_TILE - 1) / SORT_TILE;
  w.keys_a = c.template take<K>(n);
  w.keys_b = c.template take<K>(n);
  w.idx_a = c.take<uint32_t>(n);
  w.idx_b = c.take<uint32_t>(n);
  // the digit-major histogram is scanned as hist_rows rows of hist_row_len words by as many workgroups, then the rows' totals by one
  const int64_t words = w.sort_tiles * 256;
  w.hist_row_len = std::max<int64_t>(SCAN_NT, (words + SCAN_NT - 1) / SCAN_NT);
  w.hist_rows = (words + w.hist_row_len - 1) / w.hist_row_len;
  w.hist = c.take<uint32_t>((size_t)(w.hist_rows * w.hist_row_len));
  w.row_tot = c.take<uint32_t>(w.hist_rows);
  return w;
}

// `passes` stable passes over the low 8 * passes bits of the n keys in keys_a (values in idx_a).  The sorted pairs end in keys_a / idx_a
// after an even number of passes (none included: the pairs stay where they are) and in keys_b / idx_b after an odd one: *keys and *values
// say where.  Launches only.
template <class K>
inline void sort_pairs_lsd(const SortWs<K>& w, int64_t n, int passes, hipStream_t s, const K** keys, const uint32_t** values) {
  K *kin = w.keys_a, *kout = w.keys_b;
  uint32_t *vin = w.idx_a, *vout = w.idx_b;
  for (int pass = 0; pass < passes; ++pass) {
    const dim3 g((unsigned)w.sort_tiles), b(SORT_NT);
    hipLaunchKernelGGL(sort_hist_kernel<K>, g, b, 0, s, (const K*)kin, n, pass * 8, w.hist, w.sort_tiles);
    // the words past the histogram in the last row hold anything: they follow every word that is read, and the last row's total is not used
    hipLaunchKernelGGL(exclusive_scan_rows_kernel<SCAN_NT>, dim3((unsigned)w.hist_rows), dim3(SCAN_NT), 0, s, w.hist, (const int64_t*)nullptr,
                       w.hist_row_len, w.row_tot);
    hipLaunchKernelGGL(exclusive_scan_rows_kernel<SCAN_NT>, dim3(1), dim3(SCAN_NT), 0, s, w.row_tot, (const int64_t*)nullptr, w.hist_rows,
                       (uint32_t*)nullptr);
    hipLaunchKernelGGL(sort_scatter_kernel<K>, g, b, 0, s, (const K*)kin, (const uint32_t*)vin, n, pass * 8, (const uint32_t*)w.hist,
                       w.sort_tiles, (const uint32_t*)w.row_tot, w.hist_row_len, kout, vout);
    std::swap(kin, kout);
    std::swap(vin, vout);
  }
  *keys = kin;
  *values = vin;
}
