// The exact nearest-neighbour index shared by the reconstruction metrics (f3r_recon.hip) and the view matcher (f3r_match.hip): the layout of
// one index (a header, float4 records {x, y, z, index} in cell order, the sorted keys, the cell-start table), the rules that size a grid
// (set_grid, the first cell size, the occupancy test, the refinement: host and device functions, so that the host-driven builder of
// f3r_recon.hip and the device-driven one of f3r_match.hip evaluate one text), the cell arithmetic, the fp64 distance, and the ring walk
// with the lower bound that makes it exact.  Header-only: functions in an unnamed namespace, so each file that includes it carries its
// own copy.  Files that include it are compiled with -ffp-contract=off (see dist2).
#pragma once

#include <cmath>
#include <cstddef>

#include "f3r_prims.h"

namespace {

constexpr int MAX_DIM = 1024;      // grid cells per axis: keys fit 30 bits
constexpr int HDR_BYTES = 256;
constexpr double SLACK = 1e-6;     // cells: covers the rounding of the cell coordinates in the lower bounds (see grid_search)

// one uniform grid: its cells are keys [base, base + ncells) of the index's key space; every point it holds lies in [lo, hi]
struct Grid {
  double lo[3], hi[3];
  double h, inv_h;
  int32_t dims[3];
  uint32_t base;
  int64_t ncells;
};

// g[0] covers the box of most points; with ngrid == 2 it is trimmed to the 1st..99th percentiles (plus a margin) and g[1] covers
// the whole bounding box but holds only the points outside g[0] (far outliers), so that they do not stretch g[0]'s cells
struct NNHeader {
  Grid g[2];
  int32_t ngrid;
  int32_t dense;     // 1: uint32 start[ncells + 1] after the keys; 0: binary search in the sorted keys
  int64_t m, ncells, occupied;
  int32_t key_bits, pad;
};
static_assert(sizeof(NNHeader) <= HDR_BYTES, "header");
static_assert(sizeof(Grid) == 88 && offsetof(NNHeader, ngrid) == 176, "tests/test_recon_metric_gpu.py reads ngrid at byte 176");

// ---- sizing a grid.  Each builder evaluates these where it always has (f3r_nn_build on the host, mv_grid_kernel on the device: cbrt and sqrt
//      of the two sides need not agree to the last bit, and h decides the bytes of the index).  fmax / fmin / floor mean the same on both sides
//      for the finite boxes these see.  The bound of grid_search holds for any h: these rules decide the speed, never the result.
__host__ __device__ inline int key_bits_of(int64_t n) {  // bits that hold 0 .. n - 1
  int b = 0;
  while (b < 62 && ((int64_t)1 << b) < n) ++b;
  return b;
}

// grid of cell h over the (finite) box [lo, hi]: at most MAX_DIM cells per axis and cap cells in all
__host__ __device__ inline void set_grid(Grid& g, const double lo[3], const double hi[3], double h, int64_t cap) {
  double ext = 0.0;
  for (int a = 0; a < 3; ++a) ext = fmax(ext, hi[a] - lo[a]);
  if (!(ext > 0.0)) h = 1.0;
  else if (!(h >= ext / (MAX_DIM - 0.5))) h = ext / (MAX_DIM - 0.5);  // also a NaN / zero h
  for (int it = 0;; ++it) {
    g.h = h;
    g.inv_h = 1.0 / h;
    g.ncells = 1;
    for (int a = 0; a < 3; ++a) {
      g.lo[a] = lo[a];
      g.hi[a] = hi[a];
      g.dims[a] = (int)fmin(fmax(floor((hi[a] - lo[a]) * g.inv_h) + 1.0, 1.0), (double)MAX_DIM);
      g.ncells *= g.dims[a];
    }
    if (g.ncells <= cap) break;
    // too many cells for the caller's table: a larger cell (h > ext gives one cell, so this ends)
    h = it < 200 ? h * fmax(cbrt((double)g.ncells / (double)cap), 1.0) * 1.1 : 2.0 * ext;
  }
  g.base = 0;
}

__host__ __device__ inline double box_volume(const double lo[3], const double hi[3]) {
  double ext = 0.0, vol = 1.0;
  for (int a = 0; a < 3; ++a) ext = fmax(ext, hi[a] - lo[a]);
  for (int a = 0; a < 3; ++a) vol *= fmax(hi[a] - lo[a], 1e-3 * ext);
  return vol;
}

// the first cell: PPC_TARGET points per cell if the count points filled the volume
constexpr double PPC_TARGET = 16.0;
__host__ __device__ inline double first_cell_size(double volume, int64_t count) { return cbrt(volume * PPC_TARGET / (double)count); }

// points per occupied cell after a sort: within a factor of two of the target, the grid stays as it is
__host__ __device__ inline bool occupancy_ok(double ppc) { return ppc >= 0.5 * PPC_TARGET && ppc <= 2.0 * PPC_TARGET; }

// one refinement.  Too few points per cell: a surface (~h^2 per cell); too many: the points fill a smaller volume than the box (~h^3 per cell)
__host__ __device__ inline double refined_cell_size(double h, double ppc) {
  return h * (ppc < 0.5 * PPC_TARGET ? sqrt(PPC_TARGET / ppc) : cbrt(PPC_TARGET / ppc));
}

__device__ __forceinline__ const float4v* hdr_recs(const uint8_t* ix) { return (const float4v*)(ix + HDR_BYTES); }
__device__ __forceinline__ const uint32_t* hdr_keys(const uint8_t* ix, int64_t m) { return (const uint32_t*)(ix + HDR_BYTES + 16 * m); }
__device__ __forceinline__ const uint32_t* hdr_table(const uint8_t* ix, int64_t m) { return (const uint32_t*)(ix + HDR_BYTES + 20 * m); }

__device__ __forceinline__ int cell_coord(double u, int G) {
  const double f = floor(u);
  if (!(f >= 0.0)) return 0;  // also NaN
  if (f >= (double)(G - 1)) return G - 1;
  return (int)f;
}

__device__ __forceinline__ uint32_t cell_key(const Grid& g, double x, double y, double z) {
  const int cx = cell_coord((x - g.lo[0]) * g.inv_h, g.dims[0]);
  const int cy = cell_coord((y - g.lo[1]) * g.inv_h, g.dims[1]);
  const int cz = cell_coord((z - g.lo[2]) * g.inv_h, g.dims[2]);
  return g.base + ((uint32_t)cz * (uint32_t)g.dims[1] + (uint32_t)cy) * (uint32_t)g.dims[0] + (uint32_t)cx;
}

__device__ __forceinline__ bool in_box(const Grid& g, double x, double y, double z) {
  return x >= g.lo[0] && x <= g.hi[0] && y >= g.lo[1] && y <= g.hi[1] && z >= g.lo[2] && z <= g.hi[2];
}

// the grid a point belongs to (the same rule for database points and, for ordering only, for queries)
__device__ __forceinline__ uint32_t point_key(const NNHeader& H, float x, float y, float z) {
  const double X = x, Y = y, Z = z;
  return (H.ngrid == 2 && !in_box(H.g[0], X, Y, Z)) ? cell_key(H.g[1], X, Y, Z) : cell_key(H.g[0], X, Y, Z);
}

// squared distance of fp32 points in fp64, ((dx^2 + dy^2) + dz^2) without contraction: what cKDTree computes on its float64 copies
__device__ __forceinline__ double dist2(double qx, double qy, double qz, const float4v r) {
  const double dx = __dsub_rn(qx, (double)r[0]), dy = __dsub_rn(qy, (double)r[1]), dz = __dsub_rn(qz, (double)r[2]);
  return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

// Exact search.  u = (q - lo) / h is the query's continuous cell coordinate, ci its cell clamped to the grid.  Every database
// point of a grid lies in its (clamped) cell c_p, and since the grid spans the box [lo, hi] of its points, u_p in [c_p, c_p + 1]
// (to within the rounding of u, far below SLACK cells).  Ring R = the cells at Chebyshev distance R from ci.  A cell c at
// distance >= R has an axis a with |c_a - ci_a| >= R:
//   * upper side (c_a >= ci_a + R, exists only if ci_a + R <= G_a - 1, so ci_a < G_a - 1 and u_a < ci_a + 1):
//       |p_a - q_a| >= (c_a - u_a) h >= (ci_a + R - u_a) h  > (R - 1) h
//   * lower side (c_a <= ci_a - R, exists only if ci_a >= R >= 1, so u_a >= ci_a):
//       |p_a - q_a| >= (u_a - c_a - 1) h >= (u_a - ci_a + R - 1) h >= (R - 1) h
// and on every other axis b, |p_b - q_b| >= out_b h, out_b = the distance of u_b from [0, G_b] (non-zero for queries outside the
// box).  So  LB(R)^2 = h^2 min over (a, side) of [gap_a^2 + sum_{b != a} out_b^2]  bounds the squared distance of every point in
// every unvisited ring, each gap shrunk by SLACK.  The search stops once LB(R)^2 > best^2 (strict: a point at exactly the best
// distance but a smaller index is still visited), or when no side has cells left; a cell whose own box is farther than the best
// is skipped.  Queries outside the box are exact: they only visit more rings.  With two grids each is searched in turn with the
// same running result (the one holding the query first), and the bound of each covers exactly its own points.
template <class V>
__device__ void grid_search(const uint8_t* __restrict__ ix, int gi, double qx, double qy, double qz, V& vis) {
  const NNHeader& H = *(const NNHeader*)ix;
  const Grid& g = H.g[gi];
  const float4v* __restrict__ recs = hdr_recs(ix);
  const uint32_t* __restrict__ keys = hdr_keys(ix, H.m);
  const uint32_t* __restrict__ table = hdr_table(ix, H.m);
  const double q[3] = {qx, qy, qz};
  double u[3], out2[3];
  int ci[3], G[3];
  for (int a = 0; a < 3; ++a) {
    G[a] = g.dims[a];
    u[a] = (q[a] - g.lo[a]) * g.inv_h;
    ci[a] = cell_coord(u[a], G[a]);
    const double o = u[a] < 0.0 ? -u[a] : (u[a] > (double)G[a] ? u[a] - (double)G[a] : 0.0);
    const double os = fmax(o - SLACK, 0.0);
    out2[a] = os * os;
  }
  const double h2 = g.h * g.h;
  for (int R = 0;; ++R) {
    if (R > 0) {
      double lb2 = INFINITY;
      for (int a = 0; a < 3; ++a) {
        double g = INFINITY;
        if (ci[a] + R <= G[a] - 1) g = (double)(ci[a] + R) - u[a];
        if (ci[a] - R >= 0) g = fmin(g, u[a] - (double)(ci[a] - R + 1));
        if (g == INFINITY) continue;
        g = fmax(g - SLACK, 0.0);
        lb2 = fmin(lb2, g * g + (out2[0] + out2[1] + out2[2] - out2[a]));
      }
      if (lb2 == INFINITY) break;            // every cell has been visited
      if (lb2 * h2 > vis.bound()) break;     // nothing unvisited can be as close as the current result
    }
    const int z0 = max(ci[2] - R, 0), z1 = min(ci[2] + R, G[2] - 1);
    const int y0 = max(ci[1] - R, 0), y1 = min(ci[1] + R, G[1] - 1);
    const int x0 = max(ci[0] - R, 0), x1 = min(ci[0] + R, G[0] - 1);
    for (int cz = z0; cz <= z1; ++cz) {
      const double gz = fmax(fmax((double)cz - u[2], u[2] - (double)(cz + 1)) - SLACK, 0.0);
      for (int cy = y0; cy <= y1; ++cy) {
        const double gy = fmax(fmax((double)cy - u[1], u[1] - (double)(cy + 1)) - SLACK, 0.0);
        const bool full = (abs(cz - ci[2]) == R) || (abs(cy - ci[1]) == R);
        const int step = full ? 1 : 2 * R;
        for (int cx = full ? x0 : ci[0] - R; cx <= (full ? x1 : ci[0] + R); cx += step) {
          if (cx < 0 || cx >= G[0]) continue;
          const double gx = fmax(fmax((double)cx - u[0], u[0] - (double)(cx + 1)) - SLACK, 0.0);
          if ((gx * gx + gy * gy + gz * gz) * h2 > vis.bound()) continue;
          const uint32_t key = g.base + ((uint32_t)cz * (uint32_t)G[1] + (uint32_t)cy) * (uint32_t)G[0] + (uint32_t)cx;
          int64_t j, e;
          if (H.dense) {
            j = table[key];
            e = table[key + 1];
          } else {
            j = first_ge(keys, 0, H.m, key);
            e = H.m;
          }
          for (; j < e; ++j) {
            if (!H.dense && keys[j] != key) break;
            const float4v r = recs[j];
            vis.add(dist2(qx, qy, qz, r), (int)__float_as_uint(r.w));
          }
        }
      }
    }
  }
}

template <class V>
__device__ void search(const uint8_t* __restrict__ ix, double qx, double qy, double qz, V& vis) {
  const NNHeader& H = *(const NNHeader*)ix;
  if (H.ngrid == 1) {
    grid_search(ix, 0, qx, qy, qz, vis);
    return;
  }
  const int first = in_box(H.g[0], qx, qy, qz) ? 0 : 1;
  grid_search(ix, first, qx, qy, qz, vis);
  grid_search(ix, 1 - first, qx, qy, qz, vis);
}

struct Best1 {
  double d2 = INFINITY;
  int i = 0x7fffffff;
  __device__ double bound() const { return d2; }
  __device__ void add(double d, int j) {
    if (d < d2 || (d == d2 && j < i)) { d2 = d; i = j; }
  }
};

}  // namespace
