// Reconstruction metrics (MultiViewDUSt3RLitModule.evaluate_reconstruction, fast3r/models/multiview_dust3r_module.py:551-735, and
// accuracy / completion / completion_ratio, fast3r/eval/recon_metric.py:14-49) on the GPU:
//   * an exact nearest-neighbour index over a point cloud: a uniform grid whose cell is sized from the occupied-cell count (surfaces),
//     points sorted by their 32-bit cell keys with the stable LSD radix sort of f3r_sort.h (slot order never depends on arrival order),
//     float4 records {x, y, z, original index}, a dense cell-start table for small grids and a binary search in the sorted keys
//     otherwise; the grids are sized on the host by the rules of f3r_nn.h;
//   * exact 1-NN (what scipy's cKDTree.query returns: fp64 distances of the fp32 coordinates, ties to the smaller index) by
//     Chebyshev rings of cells around the query's cell, stopped by a lower bound on every unvisited cell (grid_search);
//   * k-NN (k <= 64) and the normal of Open3D's PointCloud.estimate_normals() (KNN 30, fast_normal_computation): one-pass cumulant
//     covariance in fp64, eigenvector of the smallest eigenvalue by Jacobi rotations (f3r_linalg.h);
//   * statistics: fp64 means by a fixed two-level reduction, exact medians (np.median) by an 8 x 8-bit radix select on 64-bit
//     order-preserving keys of the fp64 values, |n_a . n_b[idx]|, the completion ratio;
//   * the per-sample pipeline: per-view torch.quantile thresholds, stable compaction across views in torch.cat order, one weighted
//     similarity registration per sample (the align path's Umeyama solve), s (x R^T) + t.
// Integer atomics only (histogram counts); no float atomics anywhere: every output is deterministic.
#include "f3r_common.h"

#include <algorithm>
#include <cstddef>
#include <cmath>

#include "f3r_linalg.h"
#include "f3r_post_common.h"
#include "f3r_sort.h"  // sort_ws / sort_pairs_lsd, here over 32-bit keys (shared with f3r_cloud.hip, f3r_depth.hip, f3r_match.hip)
#include "f3r_nn.h"    // the index layout, the sizing rules, the cell arithmetic, dist2, grid_search with its bound, Best1 (shared with f3r_match.hip)

// build.sh compiles this file with -ffp-contract=off: every product and sum is rounded on its own, as the reference's numpy / torch CPU
// operations and cKDTree's distance are (the __d*_rn intrinsics alone do not stop the compiler from fusing them into FMAs).

namespace {

constexpr int TILE = 2048;         // pixels per compaction workgroup of f3r_recon_prepare (one wave walks its tile in 64-pixel steps)
constexpr int64_t DENSE_EXTRA = 65536;
constexpr int MISC_BYTES = 512;    // workspace tail: bbox / count words [0, 8), quantiles [8, 14), a header copy from word 16
constexpr int PNT = 1024;

static_assert(64 + sizeof(NNHeader) <= MISC_BYTES, "header");

inline int64_t tiles_of(int64_t n) { return (n + TILE - 1) / TILE; }
inline int64_t dense_cap(int64_t m) { return 2 * m + DENSE_EXTRA; }

// ---------------------------------------------------------------------------------------------------------------------------
// bounding box: order-preserving uint keys with integer atomics (min / max do not depend on order)
__global__ void bbox_kernel(const float* __restrict__ p, int64_t m, uint32_t* __restrict__ bb /*6: min xyz, max xyz*/) {
  uint32_t mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x)
    for (int a = 0; a < 3; ++a) {
      const uint32_t k = fkey(p[i * 3 + a]);
      mn[a] = min(mn[a], k);
      mx[a] = max(mx[a], k);
    }
  for (int a = 0; a < 3; ++a) {
    mn[a] = wave_min(mn[a]);
    mx[a] = wave_max(mx[a]);
  }
  if ((threadIdx.x & 63) == 0)
    for (int a = 0; a < 3; ++a) {
      atomicMin(&bb[a], mn[a]);
      atomicMax(&bb[3 + a], mx[a]);
    }
}

__global__ void key_kernel(const float* __restrict__ p, int64_t n, const NNHeader* __restrict__ hdr, uint32_t* __restrict__ keys,
                           uint32_t* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  keys[i] = point_key(*hdr, p[i * 3 + 0], p[i * 3 + 1], p[i * 3 + 2]);
  vals[i] = (uint32_t)i;
}

__global__ void count_heads_kernel(const uint32_t* __restrict__ keys, int64_t n, uint32_t* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  wave_count_add(i < n && (i == 0 || keys[i] != keys[i - 1]), count);
}

__global__ void dense_start_kernel(const uint32_t* __restrict__ keys, int64_t m, int64_t ncells, uint32_t* __restrict__ start) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c > ncells) return;
  start[c] = (uint32_t)first_ge(keys, 0, m, (uint32_t)c);  // c == ncells: beyond every key
}

__global__ void recs_kernel(const float* __restrict__ p, const uint32_t* __restrict__ order, int64_t m, float4v* __restrict__ recs) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const uint32_t i = order[j];
  recs[j] = float4v{p[(int64_t)i * 3 + 0], p[(int64_t)i * 3 + 1], p[(int64_t)i * 3 + 2], __uint_as_float(i)};
}

// k best in (d2, index) lexicographic order, in LDS columns [slot][thread] (conflict-free)
struct BestK {
  double* d;
  int* id;
  int k, n = 0, stride;
  __device__ double bound() const { return n < k ? INFINITY : d[(k - 1) * stride]; }
  __device__ void add(double dd, int j) {
    if (n == k) {
      const double wd = d[(k - 1) * stride];
      if (!(dd < wd || (dd == wd && j < id[(k - 1) * stride]))) return;
    }
    int p = (n < k) ? n++ : k - 1;
    while (p > 0) {
      const double pd = d[(p - 1) * stride];
      const int pi = id[(p - 1) * stride];
      if (pd < dd || (pd == dd && pi < j)) break;
      d[p * stride] = pd;
      id[p * stride] = pi;
      --p;
    }
    d[p * stride] = dd;
    id[p * stride] = j;
  }
};

__global__ __launch_bounds__(128) void nn1_kernel(const uint8_t* __restrict__ ix, const float* __restrict__ q, const uint32_t* __restrict__ order,
                                                  int64_t n, double* __restrict__ dist, int32_t* __restrict__ idx) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int64_t qi = order[t];
  Best1 b;
  search(ix, (double)q[qi * 3 + 0], (double)q[qi * 3 + 1], (double)q[qi * 3 + 2], b);
  const bool found = b.i != 0x7fffffff;  // always, for the finite queries f3r_nn_query admits
  dist[qi] = found ? __dsqrt_rn(b.d2) : INFINITY;
  idx[qi] = found ? b.i : (int32_t)((const NNHeader*)ix)->m;  // cKDTree's "no neighbour": index m
}

__global__ void empty_query_kernel(int64_t n, double* __restrict__ dist, int32_t* __restrict__ idx) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  dist[t] = INFINITY;  // cKDTree: no neighbour -> inf, index n (= 0)
  idx[t] = 0;
}

constexpr int KNT = 64;  // k-NN threads per workgroup: 64 x 64 slots x 12 bytes of LDS at k = 64

// k nearest of every database point (itself included), walked in sorted order; normal of Open3D's EstimateNormals (fast path):
// cumulants in (distance, index) order, covariance E[x x^T] - mu mu^T, eigenvector of the smallest eigenvalue; < 3 neighbours -> +z
__global__ __launch_bounds__(KNT) void knn_normals_kernel(const uint8_t* __restrict__ ix, const float* __restrict__ pts, int k,
                                                          double* __restrict__ normals, int32_t* __restrict__ knn_idx, double* __restrict__ knn_dist) {
  extern __shared__ char smem[];
  const NNHeader& H = *(const NNHeader*)ix;
  const int64_t j = (int64_t)blockIdx.x * KNT + threadIdx.x;
  if (j >= H.m) return;
  const float4v r = hdr_recs(ix)[j];
  const int64_t self = __float_as_uint(r.w);
  if (self >= H.m) return;  // records hold indices < m by construction
  BestK b;
  b.d = (double*)smem + threadIdx.x;
  b.id = (int*)((double*)smem + (size_t)k * KNT) + threadIdx.x;
  b.k = k;
  b.stride = KNT;
  search(ix, (double)r[0], (double)r[1], (double)r[2], b);
  if (knn_idx)
    for (int s = 0; s < b.n; ++s) {
      knn_idx[self * k + s] = b.id[s * KNT];
      if (knn_dist) knn_dist[self * k + s] = __dsqrt_rn(b.d[s * KNT]);
    }
  if (!normals) return;
  double nrm[3] = {0.0, 0.0, 1.0};
  if (b.n >= 3) {
    double c[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int s = 0; s < b.n; ++s) {
      const int64_t i = b.id[s * KNT];
      const double x = pts[i * 3 + 0], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
      c[0] = __dadd_rn(c[0], x);
      c[1] = __dadd_rn(c[1], y);
      c[2] = __dadd_rn(c[2], z);
      c[3] = __dadd_rn(c[3], __dmul_rn(x, x));
      c[4] = __dadd_rn(c[4], __dmul_rn(x, y));
      c[5] = __dadd_rn(c[5], __dmul_rn(x, z));
      c[6] = __dadd_rn(c[6], __dmul_rn(y, y));
      c[7] = __dadd_rn(c[7], __dmul_rn(y, z));
      c[8] = __dadd_rn(c[8], __dmul_rn(z, z));
    }
    const double cnt = (double)b.n;
    for (int t = 0; t < 9; ++t) c[t] = __ddiv_rn(c[t], cnt);
    double A[3][3], V[3][3];
    A[0][0] = __dsub_rn(c[3], __dmul_rn(c[0], c[0]));
    A[0][1] = A[1][0] = __dsub_rn(c[4], __dmul_rn(c[0], c[1]));
    A[0][2] = A[2][0] = __dsub_rn(c[5], __dmul_rn(c[0], c[2]));
    A[1][1] = __dsub_rn(c[6], __dmul_rn(c[1], c[1]));
    A[1][2] = A[2][1] = __dsub_rn(c[7], __dmul_rn(c[1], c[2]));
    A[2][2] = __dsub_rn(c[8], __dmul_rn(c[2], c[2]));
    f3r_la::jacobi_sym<3>(A, V);
    int e = 0;
    if (A[1][1] < A[e][e]) e = 1;
    if (A[2][2] < A[e][e]) e = 2;
    const double len = sqrt(V[0][e] * V[0][e] + V[1][e] * V[1][e] + V[2][e] * V[2][e]);
    if (len > 0.0)
      for (int a = 0; a < 3; ++a) nrm[a] = V[a][e] / len;
  }
  for (int a = 0; a < 3; ++a) normals[self * 3 + a] = nrm[a];
}

// ---------------------------------------------------------------------------------------------------------------------------
// statistics
constexpr int RED_BLOCKS = 256, RED_NT = 256;

// dots[i] = |nq[i] . ndb[idx[i]]|, numpy's ((a0 b0 + a1 b1) + a2 b2)
__global__ void dots_kernel(const int32_t* __restrict__ idx, const double* __restrict__ nq, const double* __restrict__ ndb, int64_t n,
                            int64_t m_db, double* __restrict__ dots) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t j = idx[i];
  if (j < 0 || j >= m_db) {  // cannot happen for indices from f3r_nn_query on the same cloud
    dots[i] = NAN;
    return;
  }
  const double s = __dadd_rn(__dadd_rn(__dmul_rn(ndb[j * 3 + 0], nq[i * 3 + 0]), __dmul_rn(ndb[j * 3 + 1], nq[i * 3 + 1])),
                             __dmul_rn(ndb[j * 3 + 2], nq[i * 3 + 2]));
  dots[i] = fabs(s);
}

// partial[b] = {sum dist, sum dots, count(dist < th)} over a fixed element -> block assignment, reduced in a fixed tree
__global__ __launch_bounds__(RED_NT) void reduce_kernel(const double* __restrict__ dist, const double* __restrict__ dots, int64_t n, double th,
                                                        double* __restrict__ partial) {
  __shared__ double red[RED_NT / 64][3];
  double a = 0.0, b = 0.0, c = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * RED_NT + threadIdx.x; i < n; i += (int64_t)RED_BLOCKS * RED_NT) {
    a += dist[i];
    if (dots) b += dots[i];
    c += (dist[i] < th) ? 1.0 : 0.0;
  }
  const double v[3] = {a, b, c};
  block_sum<3, RED_NT>(v, red, partial + blockIdx.x * 3);
}

// out[0] = mean dist, out[2] = mean dots, out[4] = completion ratio as np.mean(float32 (d < th)) computes it (exact counts below 2^24)
__global__ void reduce_final_kernel(const double* __restrict__ partial, int64_t n, bool has_dots, double* __restrict__ out) {
  if (threadIdx.x != 0) return;
  double s[3] = {0.0, 0.0, 0.0};
  for (int b = 0; b < RED_BLOCKS; ++b)
    for (int t = 0; t < 3; ++t) s[t] += partial[b * 3 + t];
  out[0] = n ? s[0] / (double)n : NAN;
  out[2] = (has_dots && n) ? s[1] / (double)n : NAN;
  out[4] = n ? (double)__fdiv_rn((float)s[2], (float)n) : NAN;
}

// median select state: {prefix key, remaining rank} for the two middle ranks
struct SelState {
  uint64_t prefix[2];
  int64_t k[2];
};

__global__ void sel_init_kernel(SelState* st, int64_t n, uint32_t* hist) {
  const int t = threadIdx.x;
  if (t < 512) hist[t] = 0;
  if (t == 0) {
    st->prefix[0] = st->prefix[1] = 0;
    st->k[0] = (n - 1) / 2;  // np.median: the middle value, or the mean of the two middle values for even n
    st->k[1] = n / 2;
  }
}

__global__ __launch_bounds__(256) void sel_hist_kernel(const double* __restrict__ v, int64_t n, const SelState* __restrict__ st, int pass,
                                                       uint32_t* __restrict__ hist /*[2][256]*/) {
  __shared__ uint32_t cnt[2][256];
  cnt[0][threadIdx.x] = 0;
  cnt[1][threadIdx.x] = 0;
  __syncthreads();
  const int shift = 56 - 8 * pass;
  const uint64_t mask = pass == 0 ? 0ull : (~0ull << (64 - 8 * pass));
  const uint64_t p0 = st->prefix[0], p1 = st->prefix[1];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const uint64_t key = dkey(v[i]);
    const uint32_t d = (uint32_t)(key >> shift) & 255u;
    if ((key & mask) == p0) atomicAdd(&cnt[0][d], 1u);
    if ((key & mask) == p1) atomicAdd(&cnt[1][d], 1u);
  }
  __syncthreads();
  for (int t = 0; t < 2; ++t)
    if (cnt[t][threadIdx.x]) atomicAdd(&hist[t * 256 + threadIdx.x], cnt[t][threadIdx.x]);
}

__global__ void sel_pick_kernel(SelState* st, int pass, uint32_t* hist) {
  const int t = threadIdx.x;
  if (t < 2) {
    const int shift = 56 - 8 * pass;
    int64_t acc = 0, k = st->k[t];
    int b = 0;
    for (; b < 255; ++b) {
      if (acc + hist[t * 256 + b] > k) break;
      acc += hist[t * 256 + b];
    }
    st->prefix[t] |= (uint64_t)b << shift;
    st->k[t] = k - acc;
  }
  __syncthreads();
  for (int i = t; i < 512; i += blockDim.x) hist[i] = 0;
}

__global__ void sel_final_kernel(const SelState* st, int64_t n, double* out) {
  if (threadIdx.x != 0) return;
  if (n == 0) { *out = NAN; return; }
  const double a = dkey_inv(st->prefix[0]), b = dkey_inv(st->prefix[1]);
  *out = (n & 1) ? a : (a + b) / 2.0;
}

void median_async(const double* v, int64_t n, SelState* st, uint32_t* hist, double* out, hipStream_t s) {
  hipLaunchKernelGGL(sel_init_kernel, dim3(1), dim3(512), 0, s, st, n, hist);
  if (n > 0) {
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 1024);
    for (int pass = 0; pass < 8; ++pass) {
      hipLaunchKernelGGL(sel_hist_kernel, dim3(grid), dim3(256), 0, s, v, n, st, pass, hist);
      hipLaunchKernelGGL(sel_pick_kernel, dim3(1), dim3(256), 0, s, st, pass, hist);
    }
  }
  hipLaunchKernelGGL(sel_final_kernel, dim3(1), dim3(64), 0, s, st, n, out);
}

// ---------------------------------------------------------------------------------------------------------------------------
// evaluate_reconstruction, per sample: the data of sample i is the concatenation over its views of (conf, pred xyz, gt xyz, valid)
// at pixel offsets seg[i*V + j] .. seg[i*V + j + 1]; every sample spans L pixels.
__global__ __launch_bounds__(PNT) void recon_thr_kernel(const float* __restrict__ conf, const int64_t* __restrict__ seg, float q_metric, float q_icp,
                                                        float* __restrict__ thr) {
  __shared__ uint32_t hist[2048];
  __shared__ int64_t sh_i64[2];
  __shared__ float sh_thr;
  const int64_t s0 = seg[blockIdx.x], n = seg[blockIdx.x + 1] - s0;
  const float tm = block_quantile<PNT>(conf + s0, n, q_metric, hist, sh_i64, &sh_thr);
  __syncthreads();
  const float ti = block_quantile<PNT>(conf + s0, n, q_icp, hist, sh_i64, &sh_thr);
  if (threadIdx.x == 0) {
    thr[2 * blockIdx.x] = tm;
    thr[2 * blockIdx.x + 1] = ti;
  }
}

// masks of pixel g of sample i: bit 0 = pred / ICP-GT (valid & conf >= thr_metric), bit 1 = metrics GT (valid), bit 2 = ICP weight
// (conf >= thr_icp); the thresholds are those of the view whose segment holds g
__device__ __forceinline__ uint32_t pix_mask(const float* conf, const uint8_t* valid, const int64_t* seg, const float* thr, int i, int V,
                                                int64_t g) {
  const int s = last_le(seg, i * V, (i + 1) * V, g);
  const float c = conf[g];
  const bool v = valid[g] != 0;
  return (v && c >= thr[2 * s] ? 1u : 0u) | (v ? 2u : 0u) | (c >= thr[2 * s + 1] ? 4u : 0u);
}

__global__ __launch_bounds__(64) void recon_count_kernel(const float* __restrict__ conf, const uint8_t* __restrict__ valid, const int64_t* __restrict__ seg,
                                                         const float* __restrict__ thr, int V, int64_t L, int64_t ntiles, uint32_t* __restrict__ cnt) {
  const int i = blockIdx.y;
  uint32_t n[2];
  tile_count<TILE>((int64_t)blockIdx.x * TILE, L, [&](int64_t p) { return pix_mask(conf, valid, seg, thr, i, V, (int64_t)i * L + p); }, n);
  if (threadIdx.x == 0) {
    cnt[(int64_t)i * ntiles + blockIdx.x] = n[0];
    cnt[((int64_t)gridDim.y + i) * ntiles + blockIdx.x] = n[1];
  }
}

// ordered writes: pred / ICP-GT / weight at [i*L + rank among bit 0], metrics GT at [i*L + rank among bit 1]
__global__ __launch_bounds__(64) void recon_compact_kernel(const float* __restrict__ conf, const float* __restrict__ pred, const float* __restrict__ gt,
                                                           const uint8_t* __restrict__ valid, const int64_t* __restrict__ seg, const float* __restrict__ thr,
                                                           int V, int64_t L, int64_t ntiles, const uint32_t* __restrict__ cnt, float* __restrict__ pred_c,
                                                           float* __restrict__ gticp_c, uint8_t* __restrict__ w_c, float* __restrict__ gt_c) {
  const int i = blockIdx.y;
  uint32_t run[2] = {cnt[(int64_t)i * ntiles + blockIdx.x], cnt[((int64_t)gridDim.y + i) * ntiles + blockIdx.x]};
  tile_compact<TILE>(
      (int64_t)blockIdx.x * TILE, L, run, [&](int64_t p) { return pix_mask(conf, valid, seg, thr, i, V, (int64_t)i * L + p); },
      [&](int64_t p, uint32_t mk, const uint32_t(&k)[2]) {
        const int64_t g = (int64_t)i * L + p;
        if (mk & 1u) {
          const int64_t o = (int64_t)i * L + k[0];
          for (int a = 0; a < 3; ++a) {
            pred_c[o * 3 + a] = pred[g * 3 + a];
            gticp_c[o * 3 + a] = gt[g * 3 + a];
          }
          w_c[o] = (mk & 4u) ? 1 : 0;
        }
        if (mk & 2u) {
          const int64_t o = (int64_t)i * L + k[1];
          for (int a = 0; a < 3; ++a) gt_c[o * 3 + a] = gt[g * 3 + a];
        }
      });
}

// weighted (0/1) Umeyama over the kept points of sample blockIdx.x: fp64 raw moments of the weight-1 pairs, then the align solve
__global__ __launch_bounds__(PNT) void recon_register_kernel(const float* __restrict__ x_c, const float* __restrict__ y_c, const uint8_t* __restrict__ w_c,
                                                             const uint32_t* __restrict__ counts, int64_t L, float* __restrict__ rts) {
  __shared__ double red[PNT / 64][17];
  __shared__ double mm[17];
  const int i = blockIdx.x;
  const int64_t n = counts[i];
  const float* px = x_c + (int64_t)i * L * 3;
  const float* py = y_c + (int64_t)i * L * 3;
  const uint8_t* pw = w_c + (int64_t)i * L;
  double m[17];
#pragma unroll
  for (int j = 0; j < 17; ++j) m[j] = 0.0;
  for (int64_t k = threadIdx.x; k < n; k += PNT) {
    if (!pw[k]) continue;
    const double x0 = px[k * 3 + 0], x1 = px[k * 3 + 1], x2 = px[k * 3 + 2];
    const double y0 = py[k * 3 + 0], y1 = py[k * 3 + 1], y2 = py[k * 3 + 2];
    const double t[17] = {1.0, x0, x1, x2, y0, y1, y2, y0 * x0, y0 * x1, y0 * x2, y1 * x0, y1 * x1, y1 * x2, y2 * x0, y2 * x1, y2 * x2,
                          x0 * x0 + x1 * x1 + x2 * x2};
#pragma unroll
    for (int j = 0; j < 17; ++j) m[j] += t[j];
  }
  block_sum<17, PNT>(m, red, mm);
  if (threadIdx.x == 0) {
    if (mm[0] < 3.0) identity_rts(rts + i * 13);
    else similarity_from_moments(mm, rts + i * 13);
  }
}

// out = s * (x R^T) + t in fp32 (the reference's `s * (x @ R.T) + t`, :664), kept points only
__global__ void recon_apply_kernel(const float* __restrict__ x_c, const float* __restrict__ rts, const uint32_t* __restrict__ counts, int64_t L,
                                   int B, float* __restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (int64_t)B * L) return;
  const int i = (int)(g / L);
  if (g - (int64_t)i * L >= (int64_t)counts[i]) return;
  const float* r = rts + i * 13;
  const float x0 = x_c[g * 3 + 0], x1 = x_c[g * 3 + 1], x2 = x_c[g * 3 + 2];
  const float s = r[12];
#pragma unroll
  for (int c = 0; c < 3; ++c) out[g * 3 + c] = s * (x0 * r[c * 3 + 0] + x1 * r[c * 3 + 1] + x2 * r[c * 3 + 2]) + r[9 + c];
}

// count of non-finite coordinates (integer atomics)
__global__ void nonfinite_kernel(const float* __restrict__ p, int64_t n3, uint32_t* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  wave_count_add(i < n3 && !isfinite(p[i]), count);
}

__global__ void deinterleave_kernel(const float* __restrict__ p, int64_t m, float* __restrict__ x, float* __restrict__ y, float* __restrict__ z) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  x[i] = p[i * 3 + 0];
  y[i] = p[i * 3 + 1];
  z[i] = p[i * 3 + 2];
}

// block b: order statistic k_lo (b even) or k_hi (b odd) of axis b / 2 -> out[b]
__global__ __launch_bounds__(PNT) void axis_quantiles_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                             int64_t m, int64_t k_lo, int64_t k_hi, float* __restrict__ out) {
  __shared__ uint32_t hist[2048];
  __shared__ int64_t sh_i64[2];
  const float* v = blockIdx.x < 2 ? x : (blockIdx.x < 4 ? y : z);
  const uint32_t key = select_kth<PNT>(v, m, (blockIdx.x & 1) ? k_hi : k_lo, hist, sh_i64);
  if (threadIdx.x == 0) out[blockIdx.x] = fkey_inv(key);
}

// count of points outside the box g
__global__ void outside_kernel(const float* __restrict__ p, int64_t m, Grid g, uint32_t* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  wave_count_add(i < m && !in_box(g, p[i * 3 + 0], p[i * 3 + 1], p[i * 3 + 2]), count);
}

__global__ void to_i32_kernel(const uint32_t* __restrict__ a, int n, int32_t* __restrict__ o) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) o[t] = (int32_t)a[t];
}

// the workspaces, sized on a null base and carved on the caller's (a braced list is evaluated left to right: the regions lie in that order).
// First f3r_nn_build / _query: the sort's buffers over 32-bit keys, then the MISC_BYTES tail
struct NNWs {
  SortWs<uint32_t> sort;
  uint32_t* misc;
  size_t bytes;
};
NNWs nn_ws(void* ws, int64_t n) {
  Carve c(ws, 256);
  NNWs w;
  w.sort = sort_ws<uint32_t>(c, n);
  w.misc = c.take<uint32_t>(MISC_BYTES / 4);
  w.bytes = c.bytes();
  return w;
}
struct StatsWs {
  double *dots, *partial;
  SelState* st;
  uint32_t* hist;
  size_t bytes;
};
StatsWs stats_ws(void* ws, int64_t n) {
  Carve c(ws, 256);
  return {c.take<double>(n), c.take<double>(3 * RED_BLOCKS), c.take<SelState>(1), c.take<uint32_t>(512), c.bytes()};
}
struct PrepareWs {
  float* thr;
  uint32_t *cnt, *tot;
  float *pred_c, *gticp_c;
  uint8_t* w_c;
  size_t bytes;
};
PrepareWs prepare_ws(void* ws, int n_samples, int n_views, int64_t L) {
  const size_t B = (size_t)n_samples, BL = B * (size_t)L;
  Carve c(ws, 256);
  return {c.take<float>(2 * B * n_views), c.take<uint32_t>(2 * B * tiles_of(L)), c.take<uint32_t>(2 * B), c.take<float>(3 * BL), c.take<float>(3 * BL),
          c.take<uint8_t>(BL), c.bytes()};
}

constexpr int64_t NO_CAP = INT64_MAX;  // f3r_nn_build bounds its grids by MAX_DIM per axis only: set_grid's cell cap never binds

// key space of the grids: g[1] after g[0]
void finish_grids(NNHeader& H) {
  H.g[1].base = (uint32_t)H.g[0].ncells;
  H.ncells = H.g[0].ncells + (H.ngrid == 2 ? H.g[1].ncells : 0);
  H.key_bits = key_bits_of(H.ncells);
}

}  // namespace

extern "C" size_t f3r_nn_index_bytes(int64_t m) {
  if (m < 0) return 0;
  return align256(HDR_BYTES + 20 * (size_t)m + 4 * (size_t)(dense_cap(m) + 1));
}

extern "C" size_t f3r_nn_workspace_bytes(int64_t n) {
  if (n < 0) return 0;
  return nn_ws(nullptr, n).bytes;
}

extern "C" int f3r_nn_build(const float* pts, int64_t m, void* index, size_t index_bytes, void* workspace, size_t ws_bytes, f3r_stream_t stream) {
  F3R_REQUIRE(index && workspace && (pts || m == 0), "f3r_nn_build: null pointer");
  F3R_REQUIRE(m >= 0 && m < ((int64_t)1 << 31), "f3r_nn_build: m = %lld outside [0, 2^31)", (long long)m);
  F3R_REQUIRE(index_bytes >= f3r_nn_index_bytes(m) && (((uintptr_t)index) & 15) == 0, "f3r_nn_build: index too small / misaligned");
  F3R_REQUIRE(ws_bytes >= f3r_nn_workspace_bytes(m) && (((uintptr_t)workspace) & 255) == 0, "f3r_nn_build: workspace too small / misaligned");
  hipStream_t s = (hipStream_t)stream;
  uint8_t* ix = (uint8_t*)index;
  NNHeader H{};
  H.m = 0;
  H.ngrid = 1;
  const double unit_lo[3] = {0.0, 0.0, 0.0}, unit_hi[3] = {0.0, 0.0, 0.0};
  set_grid(H.g[0], unit_lo, unit_hi, 1.0, NO_CAP);
  finish_grids(H);
  // an empty index first: if the build fails below, the buffer still holds a valid (empty) index
  if (hipMemcpyAsync(ix, &H, sizeof(H), hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return f3r_check_launch("f3r_nn_build");
  if (m == 0) return f3r_check_launch("f3r_nn_build");
  const NNWs w = nn_ws(workspace, m);
  // ---- bounding box.  NaN keys order beyond +-inf, so any NaN or inf coordinate makes an end of the box non-finite.
  const uint32_t bb_init[8] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u, 0u, 0u};
  uint32_t bb[8];
  (void)hipMemcpyAsync(w.misc, bb_init, sizeof(bb_init), hipMemcpyHostToDevice, s);
  hipLaunchKernelGGL(bbox_kernel, dim3(std::min<unsigned>(blocks_of(m, 256), 1024)), dim3(256), 0, s, pts, m, w.misc);
  (void)hipMemcpyAsync(bb, w.misc, sizeof(bb), hipMemcpyDeviceToHost, s);
  if (hipStreamSynchronize(s) != hipSuccess) return f3r_check_launch("f3r_nn_build");
  double lo[3], hi[3];
  for (int a = 0; a < 3; ++a) {
    lo[a] = (double)fkey_inv(bb[a]);
    hi[a] = (double)fkey_inv(bb[3 + a]);
    F3R_REQUIRE(std::isfinite(lo[a]) && std::isfinite(hi[a]), "f3r_nn_build: non-finite coordinates (NaN or inf)");
  }
  double ext = 0.0;
  for (int a = 0; a < 3; ++a) ext = std::max(ext, hi[a] - lo[a]);
  // ---- far outliers: the box of the 1st..99th percentiles per axis, widened by a quarter of its extent on each side.  If the
  //      bounding box is more than 4x as large, the points outside it go to a second grid over the whole box.
  double tlo[3] = {lo[0], lo[1], lo[2]}, thi[3] = {hi[0], hi[1], hi[2]};
  int64_t m_out = 0;
  if (m >= 4096 && ext > 0.0) {
    // fp32 scratch borrowed from the sort before any key is written: keys_a, idx_a, keys_b of the 32-bit carving hold m words each
    float* ax = (float*)w.sort.keys_a;
    float* ay = (float*)w.sort.idx_a;
    float* az = (float*)w.sort.keys_b;
    float* qv = (float*)(w.misc + 8);
    float q[6];
    hipLaunchKernelGGL(deinterleave_kernel, dim3(blocks_of(m, 256)), dim3(256), 0, s, pts, m, ax, ay, az);
    hipLaunchKernelGGL(axis_quantiles_kernel, dim3(6), dim3(PNT), 0, s, ax, ay, az, m, (m - 1) / 100, (m - 1) - (m - 1) / 100, qv);
    (void)hipMemcpyAsync(q, qv, sizeof(q), hipMemcpyDeviceToHost, s);
    if (hipStreamSynchronize(s) != hipSuccess) return f3r_check_launch("f3r_nn_build");
    double text = 0.0;
    for (int a = 0; a < 3; ++a) {
      const double w4 = 0.25 * ((double)q[2 * a + 1] - (double)q[2 * a]);
      tlo[a] = std::max(lo[a], (double)q[2 * a] - w4);
      thi[a] = std::min(hi[a], (double)q[2 * a + 1] + w4);
      text = std::max(text, thi[a] - tlo[a]);
    }
    if (text < 0.25 * ext) {
      Grid t;
      set_grid(t, tlo, thi, 1.0, NO_CAP);
      uint32_t cnt = 0;
      (void)hipMemsetAsync(w.misc + 7, 0, 4, s);
      hipLaunchKernelGGL(outside_kernel, dim3(blocks_of(m, 256)), dim3(256), 0, s, pts, m, t, w.misc + 7);
      (void)hipMemcpyAsync(&cnt, w.misc + 7, 4, hipMemcpyDeviceToHost, s);
      if (hipStreamSynchronize(s) != hipSuccess) return f3r_check_launch("f3r_nn_build");
      m_out = cnt;
    }
  }
  H.m = m;
  if (m_out > 0) {
    H.ngrid = 2;
    set_grid(H.g[1], lo, hi, first_cell_size(box_volume(lo, hi), m_out), NO_CAP);
  } else {
    for (int a = 0; a < 3; ++a) { tlo[a] = lo[a]; thi[a] = hi[a]; }
  }
  const int64_t m_in = m - m_out;
  // ---- cell size of g[0]: 16 points per cell if the cloud filled its box, then one refinement from the occupied-cell count unless
  //      that lands within 8..32 already
  set_grid(H.g[0], tlo, thi, first_cell_size(box_volume(tlo, thi), m_in), NO_CAP);
  finish_grids(H);
  uint32_t* dhdr = w.misc + 16;  // a device copy of the header for the key kernel (after the bbox / count / quantile words)
  const uint32_t *ks = w.sort.keys_a, *vs = w.sort.idx_a;
  for (int round = 0; round < 2; ++round) {
    (void)hipMemcpyAsync(dhdr, &H, sizeof(H), hipMemcpyHostToDevice, s);
    hipLaunchKernelGGL(key_kernel, dim3(blocks_of(m, 256)), dim3(256), 0, s, pts, m, (const NNHeader*)dhdr, w.sort.keys_a, w.sort.idx_a);
    sort_pairs_lsd(w.sort, m, (H.key_bits + 7) / 8, s, &ks, &vs);
    uint32_t occ = 0;
    (void)hipMemsetAsync(w.misc + 7, 0, 4, s);
    hipLaunchKernelGGL(count_heads_kernel, dim3(blocks_of(m, 256)), dim3(256), 0, s, ks, m, w.misc + 7);
    (void)hipMemcpyAsync(&occ, w.misc + 7, 4, hipMemcpyDeviceToHost, s);
    if (hipStreamSynchronize(s) != hipSuccess) return f3r_check_launch("f3r_nn_build");
    H.occupied = occ;
    const double ppc = (double)m / (double)std::max<uint32_t>(occ, 1);
    if (round == 1 || occupancy_ok(ppc) || H.g[0].ncells == 1) break;
    const double h_old = H.g[0].h;
    set_grid(H.g[0], tlo, thi, refined_cell_size(h_old, ppc), NO_CAP);
    finish_grids(H);
    if (H.g[0].h == h_old) break;
  }
  // ---- records, keys, cell table
  H.dense = (H.ncells <= dense_cap(m)) ? 1 : 0;
  hipLaunchKernelGGL(recs_kernel, dim3(blocks_of(m, 256)), dim3(256), 0, s, pts, vs, m, (float4v*)(ix + HDR_BYTES));
  uint32_t* keys = (uint32_t*)(ix + HDR_BYTES + 16 * m);
  (void)hipMemcpyAsync(keys, ks, 4 * (size_t)m, hipMemcpyDeviceToDevice, s);
  if (H.dense)
    hipLaunchKernelGGL(dense_start_kernel, dim3(blocks_of(H.ncells + 1, 256)), dim3(256), 0, s, keys, m, H.ncells, (uint32_t*)(ix + HDR_BYTES + 20 * m));
  (void)hipMemcpyAsync(ix, &H, sizeof(H), hipMemcpyHostToDevice, s);
  if (hipStreamSynchronize(s) != hipSuccess) return f3r_check_launch("f3r_nn_build");
  return f3r_check_launch("f3r_nn_build");
}

static int read_header(const void* index, NNHeader* H, hipStream_t s) {
  if (hipMemcpyAsync(H, index, sizeof(NNHeader), hipMemcpyDeviceToHost, s) != hipSuccess) return -1;
  return hipStreamSynchronize(s) == hipSuccess ? 0 : -1;
}

extern "C" int f3r_nn_query(const void* index, const float* query, int64_t n, double* dist, int32_t* idx, void* workspace, size_t ws_bytes,
                            f3r_stream_t stream) {
  F3R_REQUIRE(index && workspace && ((query && dist && idx) || n == 0), "f3r_nn_query: null pointer");
  F3R_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "f3r_nn_query: n = %lld outside [0, 2^31)", (long long)n);
  F3R_REQUIRE(ws_bytes >= f3r_nn_workspace_bytes(n) && (((uintptr_t)workspace) & 255) == 0, "f3r_nn_query: workspace too small / misaligned");
  F3R_REQUIRE((((uintptr_t)index) & 15) == 0, "f3r_nn_query: index misaligned");
  if (n == 0) return F3R_OK;
  hipStream_t s = (hipStream_t)stream;
  // cKDTree rejects non-finite queries (ValueError); so does this, before the search
  const NNWs w = nn_ws(workspace, n);
  uint32_t* bad = w.misc;
  uint32_t nbad = 0;
  (void)hipMemsetAsync(bad, 0, 4, s);
  hipLaunchKernelGGL(nonfinite_kernel, dim3(blocks_of(3 * n, 256)), dim3(256), 0, s, query, 3 * n, bad);
  (void)hipMemcpyAsync(&nbad, bad, 4, hipMemcpyDeviceToHost, s);
  NNHeader H;
  if (read_header(index, &H, s)) return f3r_check_launch("f3r_nn_query");
  F3R_REQUIRE(nbad == 0, "f3r_nn_query: %u non-finite query coordinates (NaN or inf)", nbad);
  if (H.m == 0) {
    hipLaunchKernelGGL(empty_query_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, n, dist, idx);
    return f3r_check_launch("f3r_nn_query");
  }
  // queries sorted by their (clamped) cell of the same grid: neighbouring threads walk neighbouring cells
  const uint32_t *ks, *order;
  hipLaunchKernelGGL(key_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, query, n, (const NNHeader*)index, w.sort.keys_a, w.sort.idx_a);
  sort_pairs_lsd(w.sort, n, (H.key_bits + 7) / 8, s, &ks, &order);
  hipLaunchKernelGGL(nn1_kernel, dim3(blocks_of(n, 128)), dim3(128), 0, s, (const uint8_t*)index, query, order, n, dist, idx);
  return f3r_check_launch("f3r_nn_query");
}

extern "C" int f3r_estimate_normals(const void* index, const float* pts, int k, double* normals, int32_t* knn_idx, double* knn_dist,
                                    f3r_stream_t stream) {
  F3R_REQUIRE(index && pts, "f3r_estimate_normals: null pointer");
  F3R_REQUIRE(k >= 1 && k <= 64, "f3r_estimate_normals: k = %d outside 1..64", k);
  F3R_REQUIRE(normals || knn_idx, "f3r_estimate_normals: no output");
  F3R_REQUIRE((((uintptr_t)index) & 15) == 0, "f3r_estimate_normals: index misaligned");
  hipStream_t s = (hipStream_t)stream;
  NNHeader H;
  if (read_header(index, &H, s)) return f3r_check_launch("f3r_estimate_normals");
  if (H.m == 0) return F3R_OK;
  const int kk = (int)std::min<int64_t>(k, H.m);  // Open3D: k = min(knn, size)
  const size_t lds = (size_t)kk * KNT * 12;
  hipLaunchKernelGGL(knn_normals_kernel, dim3(blocks_of(H.m, KNT)), dim3(KNT), lds, s, (const uint8_t*)index, pts, kk, normals, knn_idx, knn_dist);
  return f3r_check_launch("f3r_estimate_normals");
}

extern "C" size_t f3r_recon_stats_workspace_bytes(int64_t n) {
  if (n < 0) return 0;
  return stats_ws(nullptr, n).bytes;
}

extern "C" int f3r_recon_stats(const double* dist, const int32_t* idx, const double* normals_q, const double* normals_db, int64_t n, int64_t m_db,
                               double dist_th,
                               double* out, void* workspace, size_t ws_bytes, f3r_stream_t stream) {
  F3R_REQUIRE(out && workspace && (dist || n == 0), "f3r_recon_stats: null pointer");
  F3R_REQUIRE(n >= 0 && m_db >= 0, "f3r_recon_stats: n or m_db < 0");
  F3R_REQUIRE(!normals_q == !normals_db && (!normals_q || idx || n == 0), "f3r_recon_stats: normals need both clouds' normals and idx");
  F3R_REQUIRE(ws_bytes >= f3r_recon_stats_workspace_bytes(n) && (((uintptr_t)workspace) & 255) == 0, "f3r_recon_stats: workspace too small / misaligned");
  hipStream_t s = (hipStream_t)stream;
  const auto [dots, partial, st, hist, bytes] = stats_ws(workspace, n);
  const bool nrm = normals_q != nullptr;
  if (nrm && n) hipLaunchKernelGGL(dots_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, idx, normals_q, normals_db, n, m_db, dots);
  hipLaunchKernelGGL(reduce_kernel, dim3(RED_BLOCKS), dim3(RED_NT), 0, s, dist, nrm ? dots : nullptr, n, dist_th, partial);
  hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(64), 0, s, partial, n, nrm, out);
  median_async(dist, n, st, hist, out + 1, s);
  if (nrm) median_async(dots, n, st, hist, out + 3, s);
  else (void)hipMemcpyAsync(out + 3, out + 2, 8, hipMemcpyDeviceToDevice, s);  // NaN
  return f3r_check_launch("f3r_recon_stats");
}

extern "C" size_t f3r_recon_prepare_workspace_bytes(int n_samples, int n_views, int64_t L) {
  if (n_samples <= 0 || n_views <= 0 || L <= 0) return 0;
  return prepare_ws(nullptr, n_samples, n_views, L).bytes;
}

extern "C" int f3r_recon_prepare(const float* conf, const float* pred, const float* gt, const uint8_t* valid, const int64_t* seg, int n_samples,
                                 int n_views, int64_t L, float q_metric, float q_icp, float* pred_out, float* gt_out, int32_t* counts, float* rts,
                                 void* workspace, size_t ws_bytes, f3r_stream_t stream) {
  F3R_REQUIRE(conf && pred && gt && valid && seg && pred_out && gt_out && counts && rts && workspace, "f3r_recon_prepare: null pointer");
  F3R_REQUIRE(n_samples > 0 && n_views > 0 && L > 0 && L < ((int64_t)1 << 31), "f3r_recon_prepare: bad sizes");
  F3R_REQUIRE(q_metric >= 0.f && q_metric <= 1.f && q_icp >= 0.f && q_icp <= 1.f, "f3r_recon_prepare: quantile outside [0, 1]");
  F3R_REQUIRE(ws_bytes >= f3r_recon_prepare_workspace_bytes(n_samples, n_views, L) && (((uintptr_t)workspace) & 255) == 0,
              "f3r_recon_prepare: workspace too small / misaligned");
  hipStream_t s = (hipStream_t)stream;
  const int B = n_samples, V = n_views;
  const int64_t nt = tiles_of(L);
  const size_t BL = (size_t)B * (size_t)L;
  const auto [thr, cnt, tot, pred_c, gticp_c, w_c, bytes] = prepare_ws(workspace, B, V, L);
  hipLaunchKernelGGL(recon_thr_kernel, dim3(B * V), dim3(PNT), 0, s, conf, seg, q_metric, q_icp, thr);
  hipLaunchKernelGGL(recon_count_kernel, dim3((unsigned)nt, B), dim3(64), 0, s, conf, valid, seg, thr, V, L, nt, cnt);
  hipLaunchKernelGGL(exclusive_scan_rows_kernel<SCAN_NT>, dim3(2 * B), dim3(SCAN_NT), 0, s, cnt, (const int64_t*)nullptr, nt, tot);
  hipLaunchKernelGGL(recon_compact_kernel, dim3((unsigned)nt, B), dim3(64), 0, s, conf, pred, gt, valid, seg, thr, V, L, nt, cnt, pred_c, gticp_c, w_c,
                     gt_out);
  hipLaunchKernelGGL(recon_register_kernel, dim3(B), dim3(PNT), 0, s, pred_c, gticp_c, w_c, tot, L, rts);
  hipLaunchKernelGGL(recon_apply_kernel, dim3(blocks_of((int64_t)BL, 256)), dim3(256), 0, s, pred_c, rts, tot, L, B, pred_out);
  hipLaunchKernelGGL(to_i32_kernel, dim3(blocks_of(2 * B, 64)), dim3(64), 0, s, tot, 2 * B, counts);
  return f3r_check_launch("f3r_recon_prepare");
}
