// Reciprocal pointmap matches across views (find_reciprocal_matches, fast3r/dust3r/utils/geometry.py:381-397, over the pairs of
// make_pairs, fast3r/dust3r/image_pairs.py:17-47) on the GPU, batched: one call indexes the candidates of every view, one launch searches
// every directed pair, one pass per pair keeps the mutual nearest neighbours.
//   * the index: the candidates of all views are one array with a segment table.  View v gets a standard index of f3r_nn.h (header, float4
//     records {x, y, z, candidate index local to v} in cell order, a dense cell-start table) in its own slice of one buffer, so grid_search
//     and its lower bound serve unchanged.  The grid of a view spans the box of its own points (no point is clamped into a cell it does not
//     lie in, so the bound holds for far outliers too: they only stretch the cells); its cell comes from the view's own extent and
//     occupancy by the sizing rules of f3r_nn.h (16 points per cell and one refinement from the occupied-cell count), one thread per
//     view.  A view's grid holds at most 4 m + 63 cells (a larger cell where that binds: slower, never inexact), so the key width and
//     every slice are known to the host;
//   * all points are sorted once per round by (view, cell) keys with sort_pairs_lsd (f3r_sort.h);
//   * the search: thread t of directed pair (a -> b) takes record t of a (a's own cell order: neighbouring lanes walk neighbouring cells)
//     and writes the nearest candidate of b (int32, local to b) and the fp64 distance at the query's own candidate index;
//   * reciprocity: per tile of j's candidates a count, one scan over all tiles of all pairs, an ordered write.  No atomic decides a slot.
// Integer atomics for bounding boxes and occupied-cell counts only; two runs give the same bits.  Nothing returns to the host between
// the launches of one entry point; the caller reads the offsets and the flag word back once, after f3r_match_count.
#include "f3r_common.h"

#include <algorithm>
#include <cmath>
#include <cstddef>

#include "f3r_prims.h"
#include "f3r_sort.h"
#include "f3r_nn.h"  // the index layout, the sizing rules (set_grid, key_bits_of, ...), grid_search, Best1 (shared with f3r_recon.hip)

// build.sh compiles this file with -ffp-contract=off, like f3r_recon.hip: dist2 rounds every product and sum on its own, as cKDTree does.

namespace {

constexpr int MATCH_TILE = 2048;     // candidates of view j per workgroup of the reciprocity kernels (F3R_MATCH_TILE)
constexpr int MAX_VIEWS = 65536;
constexpr int CELL_SLACK = 64;       // table words of a view: 4 m + CELL_SLACK, for at most 4 m + CELL_SLACK - 1 cells
constexpr int MATCH_HDR_BYTES = 256;  // word 0: views with a NaN / inf coordinate

struct ViewWs {  // per view: order-preserving keys of the box ends, then the occupied cells of the last sort
  uint32_t mn[3], mx[3], occ, pad;
};

inline int64_t blob_units(int64_t m) { return (2 * HDR_BYTES + 36 * m + 255) / 256; }  // header, 16 m records, 4 m unused, 16 m + 256 table
inline size_t units_bytes(int V) { return align256(4 * ((size_t)V + 1)); }

__device__ __forceinline__ const uint8_t* blob_of(const uint8_t* index, int V, int v) {
  const uint32_t* units = (const uint32_t*)(index + MATCH_HDR_BYTES);
  return index + MATCH_HDR_BYTES + ((4 * ((size_t)V + 1) + 255) & ~(size_t)255) + 256 * (size_t)units[v];  // units_bytes(V) after the header
}

// ---- layout: units[v] = 256-byte units of view v's slice (scanned in place afterwards), the per-view words reset
__global__ void mv_init_kernel(const int64_t* __restrict__ seg, int V, uint32_t* __restrict__ units, ViewWs* __restrict__ vw,
                               uint32_t* __restrict__ flag) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v == 0) *flag = 0;
  if (v > V) return;
  if (v == V) {
    units[v] = 0;
    return;
  }
  const int64_t m = seg[v + 1] - seg[v];
  units[v] = (uint32_t)((2 * HDR_BYTES + 36 * m + 255) / 256);
  ViewWs w;
  for (int a = 0; a < 3; ++a) {
    w.mn[a] = 0xffffffffu;
    w.mx[a] = 0u;
  }
  w.occ = 0;
  w.pad = 0;
  vw[v] = w;
}

// ---- bounding boxes: a wave that lies inside one view reduces first; min / max of integer keys do not depend on order
__global__ __launch_bounds__(256) void mv_bbox_kernel(const float* __restrict__ p, const int64_t* __restrict__ seg, int V, int64_t total,
                                                      ViewWs* __restrict__ vw) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool ok = i < total;
  const int v = ok ? last_le(seg, 0, V, i) : -1;
  uint32_t mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
  if (ok)
    for (int a = 0; a < 3; ++a) mn[a] = mx[a] = fkey(p[i * 3 + a]);
  const int v0 = __shfl(v, 0, 64);
  if (v0 < 0) return;  // lane 0 holds the wave's smallest i
  if (__all(!ok || v == v0)) {
    for (int a = 0; a < 3; ++a) {
      mn[a] = wave_min(mn[a]);
      mx[a] = wave_max(mx[a]);
    }
    if ((threadIdx.x & 63) == 0)
      for (int a = 0; a < 3; ++a) {
        atomicMin(&vw[v0].mn[a], mn[a]);
        atomicMax(&vw[v0].mx[a], mx[a]);
      }
  } else if (ok) {
    for (int a = 0; a < 3; ++a) {
      atomicMin(&vw[v].mn[a], mn[a]);
      atomicMax(&vw[v].mx[a], mx[a]);
    }
  }
}

// ---- one thread per view.  round 0: the box, 16 points per cell if the cloud filled it.  round 1: one refinement from the occupied-cell
//      count of the first sort unless that lands within 8 .. 32 points per cell already: the sizing rules of f3r_nn.h, which f3r_nn_build
//      evaluates on the host.
__global__ void mv_grid_kernel(const int64_t* __restrict__ seg, int V, ViewWs* __restrict__ vw, uint8_t* __restrict__ index, int round,
                               uint32_t* __restrict__ flag) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const int64_t m = seg[v + 1] - seg[v];
  NNHeader* Hp = (NNHeader*)blob_of(index, V, v);
  const int64_t cap = 4 * m + CELL_SLACK - 1;
  if (round == 0) {
    NNHeader H = {};
    H.m = m;
    H.ngrid = 1;
    H.dense = 1;
    double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0};
    bool finite = true;
    if (m > 0)
      for (int a = 0; a < 3; ++a) {
        lo[a] = (double)fkey_inv(vw[v].mn[a]);
        hi[a] = (double)fkey_inv(vw[v].mx[a]);
        finite = finite && isfinite(lo[a]) && isfinite(hi[a]);  // NaN keys order beyond the infinities: any NaN or inf shows at an end
      }
    if (!finite) {
      atomicAdd(flag, 1u);  // a count of views: the search does not run, the caller raises
      for (int a = 0; a < 3; ++a) lo[a] = hi[a] = 0.0;
    }
    set_grid(H.g[0], lo, hi, (m > 0 && finite) ? first_cell_size(box_volume(lo, hi), m) : 1.0, cap);
    H.g[1] = H.g[0];
    H.ncells = H.g[0].ncells;
    H.key_bits = 0;
    *Hp = H;
    return;
  }
  NNHeader H = *Hp;
  const uint32_t occ = vw[v].occ;
  H.occupied = occ;  // of the first sort: 0 below if the grid is refined (nothing counts the cells of the second)
  if (m > 0 && H.g[0].ncells > 1) {
    const double ppc = (double)m / (double)max(occ, 1u);
    if (!occupancy_ok(ppc)) {
      double lo[3], hi[3];
      for (int a = 0; a < 3; ++a) {
        lo[a] = H.g[0].lo[a];
        hi[a] = H.g[0].hi[a];
      }
      set_grid(H.g[0], lo, hi, refined_cell_size(H.g[0].h, ppc), cap);
      H.g[1] = H.g[0];
      H.ncells = H.g[0].ncells;
      H.occupied = 0;
    }
  }
  *Hp = H;
}

// ---- (view, cell) keys; the value is the candidate's index in the concatenation
__global__ __launch_bounds__(256) void mv_key_kernel(const float* __restrict__ p, const int64_t* __restrict__ seg, int V, int64_t total,
                                                     const uint8_t* __restrict__ index, int cell_bits, uint64_t* __restrict__ keys,
                                                     uint32_t* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int v = last_le(seg, 0, V, i);
  const NNHeader& H = *(const NNHeader*)blob_of(index, V, v);
  keys[i] = ((uint64_t)v << cell_bits) | (uint64_t)cell_key(H.g[0], (double)p[i * 3 + 0], (double)p[i * 3 + 1], (double)p[i * 3 + 2]);
  vals[i] = (uint32_t)i;
}

// ---- occupied cells per view: the heads of the runs of equal keys (a histogram over views: integer atomics)
__global__ __launch_bounds__(256) void mv_heads_kernel(const uint64_t* __restrict__ keys, int64_t total, int V, int cell_bits,
                                                       ViewWs* __restrict__ vw) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= total) return;
  const uint64_t k = keys[j];
  const int v = (int)(k >> cell_bits);
  if ((j == 0 || keys[j - 1] != k) && v < V) atomicAdd(&vw[v].occ, 1u);
}

// ---- records of every view in its sorted order
__global__ __launch_bounds__(256) void mv_recs_kernel(const float* __restrict__ p, const uint32_t* __restrict__ order, const int64_t* __restrict__ seg,
                                                      int V, int64_t total, uint8_t* __restrict__ index) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= total) return;
  const int v = last_le(seg, 0, V, j);  // sorted by view first: position j belongs to the view whose segment holds it
  const int64_t s0 = seg[v], i = order[j];
  if (i < s0 || i >= seg[v + 1]) return;  // holds by construction
  float4v* recs = (float4v*)(blob_of(index, V, v) + HDR_BYTES);
  recs[j - s0] = float4v{p[i * 3 + 0], p[i * 3 + 1], p[i * 3 + 2], __uint_as_float((uint32_t)(i - s0))};
}

// ---- cell starts: thread g of the 4 total + CELL_SLACK V table words finds its view, then the first sorted position of its cell
__global__ __launch_bounds__(256) void mv_table_kernel(const uint64_t* __restrict__ keys, const int64_t* __restrict__ seg, int V, int cell_bits,
                                                       uint8_t* __restrict__ index) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= 4 * seg[V] + (int64_t)CELL_SLACK * V) return;
  int v = 0, hi = V;
  while (hi - v > 1) {  // the last view whose first word 4 seg[v] + CELL_SLACK v is <= g
    const int mid = (v + hi) >> 1;
    if (4 * seg[mid] + (int64_t)CELL_SLACK * mid <= g) v = mid; else hi = mid;
  }
  const int64_t c = g - (4 * seg[v] + (int64_t)CELL_SLACK * v);
  uint8_t* blob = (uint8_t*)blob_of(index, V, v);
  const NNHeader& H = *(const NNHeader*)blob;
  if (c > H.ncells) return;
  const uint64_t want = ((uint64_t)v << cell_bits) | (uint64_t)c;  // c == ncells: beyond every key of the view
  ((uint32_t*)(blob + HDR_BYTES + 20 * H.m))[c] = (uint32_t)(first_ge(keys, seg[v], seg[v + 1], want) - seg[v]);
}

// ---- the search: every query of every directed pair in one launch
__global__ __launch_bounds__(128) void mv_search_kernel(const uint8_t* __restrict__ index, int V, const int32_t* __restrict__ directed,
                                                        const int64_t* __restrict__ qoff, int D, int64_t Q, int32_t* __restrict__ nn_idx,
                                                        double* __restrict__ nn_dist) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= Q) return;
  if (*(const uint32_t*)index != 0u) return;  // a view with NaN / inf coordinates: the caller raises, nothing is searched
  const int d = last_le(qoff, 0, D, t);
  const int a = directed[2 * d], b = directed[2 * d + 1];
  if (a < 0 || a >= V || b < 0 || b >= V) return;
  const uint8_t* ia = blob_of(index, V, a);
  const uint8_t* ib = blob_of(index, V, b);
  const int64_t ma = ((const NNHeader*)ia)->m, mb = ((const NNHeader*)ib)->m;
  const int64_t k = t - qoff[d];
  if (k >= ma) return;
  const float4v r = hdr_recs(ia)[k];
  const int64_t qi = __float_as_uint(r.w), o = qoff[d] + qi;
  if (qi >= ma || o >= Q) return;  // holds for tables that follow from the segments
  Best1 best;
  if (mb > 0) grid_search(ib, 0, (double)r[0], (double)r[1], (double)r[2], best);
  const bool found = best.i != 0x7fffffff;
  nn_dist[o] = found ? __dsqrt_rn(best.d2) : INFINITY;
  nn_idx[o] = found ? best.i : (int32_t)mb;  // cKDTree's "no neighbour": index m (0 for an empty view)
}

// ---- reciprocity.  pairs: rows {i, j, directed row of i -> j, directed row of j -> i}; tile t belongs to the pair p with
//      tile_off[p] <= t < tile_off[p + 1] and covers MATCH_TILE candidates of view j.  Candidate q of j matches iff nn_ij[nn_ji[q]] == q.
struct PairView {
  int64_t nj, ni, q_ji, q_ij, sj, si;
  bool ok;
};
__device__ __forceinline__ PairView pair_view(const int32_t* __restrict__ pairs, int p, const int64_t* __restrict__ seg, int V,
                                              const int64_t* __restrict__ qoff, int D, int64_t Q) {
  PairView w = {};
  const int i = pairs[4 * p], j = pairs[4 * p + 1], f = pairs[4 * p + 2], bk = pairs[4 * p + 3];
  if (i < 0 || i >= V || j < 0 || j >= V || f < 0 || f >= D || bk < 0 || bk >= D) return w;
  w.sj = seg[j];
  w.si = seg[i];
  w.nj = seg[j + 1] - w.sj;
  w.ni = seg[i + 1] - w.si;
  w.q_ij = qoff[f];
  w.q_ji = qoff[bk];
  w.ok = w.q_ij + w.ni <= Q && w.q_ji + w.nj <= Q;
  return w;
}
__device__ __forceinline__ bool reciprocal(const PairView& w, const int32_t* __restrict__ nn_idx, int64_t q, int32_t& a) {
  a = nn_idx[w.q_ji + q];
  return w.ni > 0 && a >= 0 && a < w.ni && (int64_t)nn_idx[w.q_ij + a] == q;
}

__global__ __launch_bounds__(64) void mv_count_kernel(const int32_t* __restrict__ pairs, const int64_t* __restrict__ tile_off, int P,
                                                      const int64_t* __restrict__ seg, int V, const int64_t* __restrict__ qoff, int D, int64_t Q,
                                                      const int32_t* __restrict__ nn_idx, uint32_t* __restrict__ cnt) {
  const int64_t tile = blockIdx.x;
  const int p = last_le(tile_off, 0, P, tile);
  const PairView w = pair_view(pairs, p, seg, V, qoff, D, Q);
  uint32_t n[1];
  tile_count<MATCH_TILE>(
      (tile - tile_off[p]) * MATCH_TILE, w.nj,
      [&](int64_t q) {
        int32_t a;
        return w.ok && reciprocal(w, nn_idx, q, a);
      },
      n);
  if (threadIdx.x == 0) cnt[tile] = n[0];
}

// offsets[p] = matches before pair p (the scanned count of its first tile; tile_off[P] is the word after the last tile: the total)
__global__ void mv_offsets_kernel(const uint32_t* __restrict__ cnt, const int64_t* __restrict__ tile_off, int P, const uint8_t* __restrict__ index,
                                  int64_t* __restrict__ offsets) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p <= P) offsets[p] = (int64_t)cnt[tile_off[p]];
  if (p == P + 1) offsets[p] = (int64_t)(*(const uint32_t*)index);  // the flag word rides along: one read-back
}

__global__ __launch_bounds__(64) void mv_write_kernel(const int32_t* __restrict__ pairs, const int64_t* __restrict__ tile_off, int P,
                                                      const int64_t* __restrict__ seg, int V, const int64_t* __restrict__ qoff, int D, int64_t Q,
                                                      const int32_t* __restrict__ nn_idx, const double* __restrict__ nn_dist,
                                                      const uint32_t* __restrict__ cnt, const int32_t* __restrict__ pix,
                                                      const int32_t* __restrict__ widths, int32_t* __restrict__ xy_i, int32_t* __restrict__ xy_j,
                                                      double* __restrict__ dist, int64_t M) {
  const int64_t tile = blockIdx.x;
  const int p = last_le(tile_off, 0, P, tile);
  const PairView w = pair_view(pairs, p, seg, V, qoff, D, Q);
  if (!w.ok) return;
  const int wi = max(widths[pairs[4 * p]], 1), wj = max(widths[pairs[4 * p + 1]], 1);
  int64_t run[1] = {cnt[tile]};
  int32_t a = 0;  // candidate q's neighbour in view i: flags leaves it for emit
  tile_compact<MATCH_TILE>(
      (tile - tile_off[p]) * MATCH_TILE, w.nj, run, [&](int64_t q) { return reciprocal(w, nn_idx, q, a); },
      [&](int64_t q, uint32_t, const int64_t(&slot)[1]) {
        const int64_t o = slot[0];
        if (o >= M) return;
        const int32_t pj = pix[w.sj + q], pi = pix[w.si + a];
        xy_j[2 * o] = pj % wj;
        xy_j[2 * o + 1] = pj / wj;
        xy_i[2 * o] = pi % wi;
        xy_i[2 * o + 1] = pi / wi;
        dist[o] = nn_dist[w.q_ji + q];
      });
}

// ---- host
struct IndexWs {
  SortWs<> sort;
  ViewWs* vw;
  size_t bytes;
};
IndexWs index_ws(void* ws, int64_t total, int V) {
  Carve c(ws, 256);
  IndexWs w;
  w.sort = sort_ws(c, total);
  w.vw = c.take<ViewWs>((size_t)V);
  w.bytes = c.bytes();
  return w;
}

// the segment table of the host: V + 1 ascending words from 0, fewer than 2^31 candidates per view and 2^32 in all
bool seg_ok(const int64_t* seg_host, int V) {
  if (!seg_host || V < 1 || V > MAX_VIEWS || seg_host[0] != 0) return false;
  for (int v = 0; v < V; ++v) {
    const int64_t m = seg_host[v + 1] - seg_host[v];
    if (m < 0 || m >= ((int64_t)1 << 31)) return false;
  }
  return seg_host[V] < ((int64_t)1 << 32);
}

bool aligned(const void* p, size_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

}  // namespace

extern "C" size_t f3r_match_index_bytes(const int64_t* seg_host, int n_views) {
  if (!seg_ok(seg_host, n_views)) return 0;
  size_t units = 0;
  for (int v = 0; v < n_views; ++v) units += (size_t)blob_units(seg_host[v + 1] - seg_host[v]);
  return MATCH_HDR_BYTES + units_bytes(n_views) + 256 * units;
}

extern "C" size_t f3r_match_workspace_bytes(int64_t total, int n_views) {
  if (total < 0 || total >= ((int64_t)1 << 32) || n_views < 1 || n_views > MAX_VIEWS) return 0;
  return index_ws(nullptr, total, n_views).bytes;
}

extern "C" int f3r_match_index(const float* pts, const int64_t* seg, const int64_t* seg_host, int n_views, void* index, size_t index_bytes,
                               void* workspace, size_t ws_bytes, f3r_stream_t stream) {
  F3R_REQUIRE(seg && seg_host && index && workspace, "f3r_match_index: null pointer");
  F3R_REQUIRE(n_views >= 1 && n_views <= MAX_VIEWS, "f3r_match_index: n_views = %d outside 1..%d", n_views, MAX_VIEWS);
  F3R_REQUIRE(seg_ok(seg_host, n_views), "f3r_match_index: the segment table must ascend from 0, below 2^31 candidates per view and 2^32 in all");
  const int V = n_views;
  const int64_t total = seg_host[V];
  F3R_REQUIRE(pts || total == 0, "f3r_match_index: null points");
  F3R_REQUIRE(aligned(pts, 4) && aligned(seg, 8), "f3r_match_index: points / segment table misaligned");
  F3R_REQUIRE(index_bytes >= f3r_match_index_bytes(seg_host, V) && aligned(index, 256), "f3r_match_index: index too small / misaligned");
  F3R_REQUIRE(ws_bytes >= f3r_match_workspace_bytes(total, V) && aligned(workspace, 256), "f3r_match_index: workspace too small / misaligned");
  hipStream_t s = (hipStream_t)stream;
  uint8_t* ix = (uint8_t*)index;
  uint32_t* flag = (uint32_t*)ix;
  uint32_t* units = (uint32_t*)(ix + MATCH_HDR_BYTES);
  const IndexWs w = index_ws(workspace, total, V);
  int64_t max_m = 0;
  for (int v = 0; v < V; ++v) max_m = std::max(max_m, seg_host[v + 1] - seg_host[v]);
  const int cell_bits = key_bits_of(4 * max_m + CELL_SLACK), view_bits = key_bits_of(V);
  const int passes = (cell_bits + view_bits + 7) / 8;  // at most 34 + 16 bits
  hipLaunchKernelGGL(mv_init_kernel, dim3(blocks_of(V + 1, 256)), dim3(256), 0, s, seg, V, units, w.vw, flag);
  hipLaunchKernelGGL(exclusive_scan_rows_kernel<SCAN_NT>, dim3(1), dim3(SCAN_NT), 0, s, units, (const int64_t*)nullptr, (int64_t)V + 1, (uint32_t*)nullptr);
  if (total > 0) hipLaunchKernelGGL(mv_bbox_kernel, dim3(blocks_of(total, 256)), dim3(256), 0, s, pts, seg, V, total, w.vw);
  const uint64_t* ks = w.sort.keys_a;
  const uint32_t* vs = w.sort.idx_a;
  for (int round = 0; round < 2; ++round) {
    hipLaunchKernelGGL(mv_grid_kernel, dim3(blocks_of(V, 64)), dim3(64), 0, s, seg, V, w.vw, ix, round, flag);
    if (total == 0) continue;
    hipLaunchKernelGGL(mv_key_kernel, dim3(blocks_of(total, 256)), dim3(256), 0, s, pts, seg, V, total, (const uint8_t*)ix, cell_bits, w.sort.keys_a,
                       w.sort.idx_a);
    sort_pairs_lsd(w.sort, total, passes, s, &ks, &vs);
    if (round == 0) hipLaunchKernelGGL(mv_heads_kernel, dim3(blocks_of(total, 256)), dim3(256), 0, s, ks, total, V, cell_bits, w.vw);
  }
  if (total > 0) hipLaunchKernelGGL(mv_recs_kernel, dim3(blocks_of(total, 256)), dim3(256), 0, s, pts, vs, seg, V, total, ix);
  hipLaunchKernelGGL(mv_table_kernel, dim3(blocks_of(4 * total + (int64_t)CELL_SLACK * V, 256)), dim3(256), 0, s, ks, seg, V, cell_bits, ix);
  return f3r_check_launch("f3r_match_index");
}

extern "C" int f3r_match_search(const void* index, const int64_t* seg_host, int n_views, const int32_t* directed, const int32_t* directed_host,
                                const int64_t* qoff, const int64_t* qoff_host, int n_directed, int32_t* nn_idx, double* nn_dist,
                                f3r_stream_t stream) {
  F3R_REQUIRE(index && seg_host && qoff_host, "f3r_match_search: null pointer");
  F3R_REQUIRE(seg_ok(seg_host, n_views), "f3r_match_search: bad segment table or n_views = %d outside 1..%d", n_views, MAX_VIEWS);
  F3R_REQUIRE(n_directed >= 0 && n_directed <= (1 << 30), "f3r_match_search: n_directed = %d outside [0, 2^30]", n_directed);
  F3R_REQUIRE(n_directed == 0 || (directed && directed_host && qoff), "f3r_match_search: null pair table");
  F3R_REQUIRE(qoff_host[0] == 0, "f3r_match_search: query offsets must start at 0");
  for (int d = 0; d < n_directed; ++d) {
    const int a = directed_host[2 * d], b = directed_host[2 * d + 1];
    F3R_REQUIRE(a >= 0 && a < n_views && b >= 0 && b < n_views, "f3r_match_search: directed pair %d = (%d, %d) outside the %d views", d, a, b, n_views);
    F3R_REQUIRE(qoff_host[d + 1] - qoff_host[d] == seg_host[a + 1] - seg_host[a], "f3r_match_search: query offsets do not follow from the segments at pair %d",
                d);
  }
  const int64_t Q = qoff_host[n_directed];
  F3R_REQUIRE(Q < ((int64_t)1 << 31), "f3r_match_search: %lld queries in one call (limit 2^31: one thread each in one launch)", (long long)Q);
  if (Q == 0) return F3R_OK;
  F3R_REQUIRE(nn_idx && nn_dist, "f3r_match_search: null output");
  F3R_REQUIRE(aligned(index, 256) && aligned(directed, 4) && aligned(qoff, 8) && aligned(nn_idx, 4) && aligned(nn_dist, 8),
              "f3r_match_search: misaligned buffer");
  hipLaunchKernelGGL(mv_search_kernel, dim3(blocks_of(Q, 128)), dim3(128), 0, (hipStream_t)stream, (const uint8_t*)index, n_views, directed, qoff,
                     n_directed, Q, nn_idx, nn_dist);
  return f3r_check_launch("f3r_match_search");
}

namespace {
// the tables of the reciprocity pass, checked on the host copies: pairs inside the views and the directed rows, tiles that follow from view j
int pairs_ok(const int64_t* seg_host, int V, const int32_t* pairs_host, const int64_t* tile_off_host, int P, const int64_t* qoff_host, int D,
             const char* who) {
  F3R_REQUIRE(seg_ok(seg_host, V), "%s: bad segment table or n_views = %d outside 1..%d", who, V, MAX_VIEWS);
  F3R_REQUIRE(P >= 0 && P <= (1 << 30) && D >= 0 && D <= (1 << 30), "%s: n_pairs = %d or n_directed = %d outside [0, 2^30]", who, P, D);
  F3R_REQUIRE(tile_off_host && qoff_host && (P == 0 || pairs_host), "%s: null host table", who);
  F3R_REQUIRE(tile_off_host[0] == 0 && qoff_host[0] == 0, "%s: tile / query offsets must start at 0", who);
  for (int p = 0; p < P; ++p) {
    const int i = pairs_host[4 * p], j = pairs_host[4 * p + 1], f = pairs_host[4 * p + 2], b = pairs_host[4 * p + 3];
    F3R_REQUIRE(i >= 0 && i < V && j >= 0 && j < V, "%s: pair %d = (%d, %d) outside the %d views", who, p, i, j, V);
    F3R_REQUIRE(f >= 0 && f < D && b >= 0 && b < D, "%s: pair %d names directed rows (%d, %d) outside the %d rows", who, p, f, b, D);
    const int64_t ni = seg_host[i + 1] - seg_host[i], nj = seg_host[j + 1] - seg_host[j];
    F3R_REQUIRE(qoff_host[f + 1] - qoff_host[f] == ni && qoff_host[b + 1] - qoff_host[b] == nj, "%s: pair %d: directed rows of other sizes than its views", who, p);
    F3R_REQUIRE(tile_off_host[p + 1] - tile_off_host[p] == (nj + MATCH_TILE - 1) / MATCH_TILE, "%s: tile offsets do not follow from view j at pair %d", who, p);
  }
  F3R_REQUIRE(tile_off_host[P] < ((int64_t)1 << 21), "%s: %lld tiles in one call (limit 2^21: fewer than 2^32 candidates of the second views)", who,
              (long long)tile_off_host[P]);
  return F3R_OK;
}
}  // namespace

extern "C" int f3r_match_count(const void* index, const int64_t* seg, const int64_t* seg_host, int n_views, const int32_t* pairs,
                               const int32_t* pairs_host, const int64_t* tile_off, const int64_t* tile_off_host, int n_pairs, const int64_t* qoff,
                               const int64_t* qoff_host, int n_directed, const int32_t* nn_idx, uint32_t* tile_counts, int64_t* offsets,
                               f3r_stream_t stream) {
  F3R_REQUIRE(index && seg && tile_off && qoff && tile_counts && offsets, "f3r_match_count: null pointer");
  if (const int rc = pairs_ok(seg_host, n_views, pairs_host, tile_off_host, n_pairs, qoff_host, n_directed, "f3r_match_count")) return rc;
  const int64_t T = tile_off_host[n_pairs], Q = qoff_host[n_directed];
  F3R_REQUIRE((pairs && nn_idx) || T == 0, "f3r_match_count: null pair table / neighbours");
  F3R_REQUIRE(aligned(index, 256) && aligned(seg, 8) && aligned(pairs, 4) && aligned(tile_off, 8) && aligned(qoff, 8) && aligned(nn_idx, 4) &&
                  aligned(tile_counts, 4) && aligned(offsets, 8),
              "f3r_match_count: misaligned buffer");
  hipStream_t s = (hipStream_t)stream;
  (void)hipMemsetAsync(tile_counts + T, 0, 4, s);
  if (T > 0)
    hipLaunchKernelGGL(mv_count_kernel, dim3((unsigned)T), dim3(64), 0, s, pairs, tile_off, n_pairs, seg, n_views, qoff, n_directed, Q, nn_idx, tile_counts);
  hipLaunchKernelGGL(exclusive_scan_rows_kernel<SCAN_NT>, dim3(1), dim3(SCAN_NT), 0, s, tile_counts, (const int64_t*)nullptr, T + 1, (uint32_t*)nullptr);
  hipLaunchKernelGGL(mv_offsets_kernel, dim3(blocks_of(n_pairs + 2, 256)), dim3(256), 0, s, (const uint32_t*)tile_counts, tile_off, n_pairs,
                     (const uint8_t*)index, offsets);
  return f3r_check_launch("f3r_match_count");
}

extern "C" int f3r_match_write(const int64_t* seg, const int64_t* seg_host, int n_views, const int32_t* pairs, const int32_t* pairs_host,
                               const int64_t* tile_off, const int64_t* tile_off_host, int n_pairs, const int64_t* qoff, const int64_t* qoff_host,
                               int n_directed, const int32_t* nn_idx, const double* nn_dist, const uint32_t* tile_counts, const int32_t* pix,
                               const int32_t* widths, int32_t* xy_i, int32_t* xy_j, double* dist, int64_t n_matches, f3r_stream_t stream) {
  F3R_REQUIRE(seg && tile_off && qoff && tile_counts && widths, "f3r_match_write: null pointer");
  if (const int rc = pairs_ok(seg_host, n_views, pairs_host, tile_off_host, n_pairs, qoff_host, n_directed, "f3r_match_write")) return rc;
  const int64_t T = tile_off_host[n_pairs], Q = qoff_host[n_directed];
  F3R_REQUIRE(n_matches >= 0 && n_matches < ((int64_t)1 << 32), "f3r_match_write: n_matches = %lld outside [0, 2^32)", (long long)n_matches);
  if (T == 0 || n_matches == 0) return F3R_OK;
  F3R_REQUIRE(pairs && nn_idx && nn_dist && pix && xy_i && xy_j && dist, "f3r_match_write: null pointer");
  F3R_REQUIRE(aligned(seg, 8) && aligned(pairs, 4) && aligned(tile_off, 8) && aligned(qoff, 8) && aligned(nn_idx, 4) && aligned(nn_dist, 8) &&
                  aligned(tile_counts, 4) && aligned(pix, 4) && aligned(widths, 4) && aligned(xy_i, 4) && aligned(xy_j, 4) && aligned(dist, 8),
              "f3r_match_write: misaligned buffer");
  hipLaunchKernelGGL(mv_write_kernel, dim3((unsigned)T), dim3(64), 0, (hipStream_t)stream, pairs, tile_off, n_pairs, seg, n_views, qoff, n_directed, Q,
                     nn_idx, nn_dist, tile_counts, pix, widths, xy_i, xy_j, dist, n_matches);
  return f3r_check_launch("f3r_match_write");
}
