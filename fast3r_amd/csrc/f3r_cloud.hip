// Point-cloud export (ABI 420; include/f3r.h "point-cloud export"): export_combined_ply of the reference's notebooks/demo_multiview.ipynb
// and the two Open3D downsamplers it calls, for a cloud that never leaves the device.
//
// * combine: per view conf > np.percentile(conf, p) (thresholds from f3r_mesh_threshold), the colour line, concatenation in view order then
//   pixel order -- kept pixels per tile, one scan, one ballot-compaction write.  The same two kernels compact a cloud by a byte mask.
// * voxel: VoxelDownSample's fp64 index arithmetic, a stable LSD radix sort of (64-bit key, point index) with 8-bit digits (per-tile
//   histograms, digit-major, a two-level scan, ballot ranking), segment heads, and per voxel one thread that adds its run sequentially
//   in fp64 in original index order -- Open3D's accumulation in Open3D's order, so the sums do not depend on scheduling.
// * farthest point: FarthestPointDownSample's loop.  One workgroup keeps points and distances in registers for the whole loop; the tiled
//   path is one plain launch per iteration, and the launch boundary is its only cross-workgroup synchronisation.
// The arg-max comparator is (larger distance, then smaller index): a total order, so no reduction shape changes the result.
// Integer atomics only (LDS histogram counters, the bounds keys): two runs give the same bits.  Built with -ffp-contract=off.
#include "f3r_common.h"
#include "f3r_post_common.h"
#include "f3r_view_row.h"
#include "f3r_sort.h"  // the LSD passes of the voxel sort (SORT_TILE, sort_ws, sort_pairs_lsd), shared with f3r_depth.hip

#include <algorithm>

namespace {

constexpr int CLOUD_TILE = 1024;               // pixels, or sorted keys, of one compaction workgroup (one wave; tile_compact, f3r_prims.h)
constexpr int CLOUD_STEPS = CLOUD_TILE / 64;     // the combine kernels: 16 steps of 64
constexpr int FPS_TILE = 1024;               // points of one tile of the tiled path
constexpr int FPS_NT = 256;
constexpr int FPS_PER = FPS_TILE / FPS_NT;
constexpr int FPS_MAX_GRID = 1024;             // workgroups (= partials) of one tiled launch at most
constexpr int FPS_ONE_NT = 1024;
constexpr int FPS_ONE_MAX = 8192;
constexpr int FPS_ONE_PER = FPS_ONE_MAX / FPS_ONE_NT;
constexpr int BOUNDS_NT = 256;
static_assert(CLOUD_TILE == F3R_CLOUD_TILE && SORT_TILE == F3R_CLOUD_SORT_TILE && FPS_TILE == F3R_CLOUD_FPS_TILE &&
                  FPS_ONE_MAX == F3R_CLOUD_FPS_ONE_MAX,
              "include/f3r.h states the tile lengths");

// ---------------------------------------------------------------------------------------------------------------------------
// combine (rows: ViewRow, f3r_view_row.h).  These two kernels keep their own fixed-step loops, not tile_count / tile_compact of
// f3r_prims.h: measured through the walker the combine stage was 2 to 3 % slower than these loops (docs/rows_f.md).
// cnt[tile] = kept pixels of the tile (n_tiles + 1 words; the last is zeroed for the scan's total)
__global__ __launch_bounds__(64) void combine_count_kernel(const ViewRow* __restrict__ rows, const int64_t* __restrict__ ts, int S,
                                                           const float* __restrict__ thr, uint32_t* __restrict__ cnt, int64_t n_tiles) {
  const int seg = last_le(ts, 0, S, blockIdx.x);
  const ViewRow r = rows[seg];
  const int64_t n = r.H * r.W, base = (blockIdx.x - ts[seg]) * CLOUD_TILE;
  const bool use_conf = thr && r.conf;
  const float t = use_conf ? thr[seg] : 0.f;
  uint32_t c = 0;
  for (int s = 0; s < CLOUD_STEPS; ++s) c += wave_flag_count(view_keep(r, use_conf, t, base + s * 64 + threadIdx.x, n));
  if (threadIdx.x == 0) {
    cnt[blockIdx.x] = c;
    if (blockIdx.x == 0) cnt[n_tiles] = 0;
  }
}

__global__ __launch_bounds__(64) void combine_write_kernel(const ViewRow* __restrict__ rows, const int64_t* __restrict__ ts, int S,
                                                           const float* __restrict__ thr, const uint32_t* __restrict__ scan, int flip,
                                                           float* __restrict__ out_p, uint8_t* __restrict__ out_c) {
  const int seg = last_le(ts, 0, S, blockIdx.x);
  const ViewRow r = rows[seg];
  const int64_t n = r.H * r.W, base = (blockIdx.x - ts[seg]) * CLOUD_TILE;
  const bool use_conf = thr && r.conf;
  const float t = use_conf ? thr[seg] : 0.f;
  int64_t run = scan[blockIdx.x];
  for (int s = 0; s < CLOUD_STEPS; ++s) {
    const int64_t i = base + s * 64 + threadIdx.x;
    const bool keep = view_keep(r, use_conf, t, i, n);
    uint64_t bal;
    const int64_t o = run + compact_rank(keep, bal);
    if (keep) {
      const float x = r.pts[i * 3 + 0], y = r.pts[i * 3 + 1], z = r.pts[i * 3 + 2];  // store_point through out_p's __restrict__
      out_p[o * 3 + 0] = x;
      out_p[o * 3 + 1] = flip ? z : y;
      out_p[o * 3 + 2] = flip ? -y : z;
      if (r.img_u8) {
        const uint8_t* g = (const uint8_t*)r.img + i * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out_c[o * 3 + ch] = g[ch];
      } else {
        const float* g = (const float*)r.img;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out_c[o * 3 + ch] = colour_u8(g[(int64_t)ch * n + i]);
      }
    }
    run += __popcll(bal);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// bounds: out = { min key x, y, z | max key x, y, z | non-finite coordinates | 0 }
__global__ void bounds_init_kernel(uint32_t* __restrict__ out) {
  if (threadIdx.x < 8) out[threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;
}

__global__ __launch_bounds__(BOUNDS_NT) void bounds_kernel(const float* __restrict__ p, int64_t n, uint32_t* __restrict__ out) {
  uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u}, bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * BOUNDS_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * BOUNDS_NT) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float v = p[i * 3 + a];
      if ((__builtin_bit_cast(uint32_t, v) & 0x7f800000u) == 0x7f800000u) {
        ++bad;
      } else {
        const uint32_t k = fkey(v);
        lo[a] = min(lo[a], k);
        hi[a] = max(hi[a], k);
      }
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = wave_min(lo[a]);
    hi[a] = wave_max(hi[a]);
  }
  bad = wave_sum(bad);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      atomicMin(&out[a], lo[a]);
      atomicMax(&out[3 + a], hi[a]);
    }
    if (bad) atomicAdd(&out[6], bad);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// voxel keys: floor((p - vmin) / voxel_size) per axis in fp64, packed x-major; idx = the identity
__global__ __launch_bounds__(256) void voxel_key_kernel(const float* __restrict__ p, int64_t n, double vx, double vy, double vz, double vs,
                                                        int sh_x, int sh_y, uint64_t* __restrict__ keys, uint32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double fx = floor(((double)p[i * 3 + 0] - vx) / vs), fy = floor(((double)p[i * 3 + 1] - vy) / vs),
               fz = floor(((double)p[i * 3 + 2] - vz) / vs);
  const uint64_t ix = (uint64_t)(int64_t)fmax(fx, 0.0), iy = (uint64_t)(int64_t)fmax(fy, 0.0), iz = (uint64_t)(int64_t)fmax(fz, 0.0);
  keys[i] = (ix << sh_x) | (iy << sh_y) | iz;
  idx[i] = (uint32_t)i;
}

// segment heads: key differs from its predecessor's.  cnt[tile] = heads of the tile (n_tiles + 1 words, the last zeroed)
__device__ __forceinline__ bool is_head(const uint64_t* __restrict__ keys, int64_t i) { return i == 0 || keys[i] != keys[i - 1]; }

__global__ __launch_bounds__(64) void head_count_kernel(const uint64_t* __restrict__ keys, int64_t n, uint32_t* __restrict__ cnt,
                                                        int64_t n_tiles) {
  uint32_t c[1];
  tile_count<CLOUD_TILE>((int64_t)blockIdx.x * CLOUD_TILE, n, [&](int64_t i) { return is_head(keys, i); }, c);
  if (threadIdx.x == 0) {
    cnt[blockIdx.x] = c[0];
    if (blockIdx.x == 0) cnt[n_tiles] = 0;
  }
}

// starts[v] = first sorted position of voxel v; starts[n_voxels] = n; *n_voxels = the scan's total
__global__ __launch_bounds__(64) void head_starts_kernel(const uint64_t* __restrict__ keys, int64_t n, const uint32_t* __restrict__ scan,
                                                         int64_t n_tiles, uint32_t* __restrict__ starts, uint32_t* __restrict__ n_voxels) {
  uint32_t run[1] = {scan[blockIdx.x]};
  tile_compact<CLOUD_TILE>((int64_t)blockIdx.x * CLOUD_TILE, n, run, [&](int64_t i) { return is_head(keys, i); },
                           [&](int64_t i, uint32_t, const uint32_t(&o)[1]) { starts[o[0]] = (uint32_t)i; });
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint32_t total = scan[n_tiles];
    starts[total] = (uint32_t)n;
    *n_voxels = total;
  }
}

// one thread per voxel: its run in sorted order is its points in original index order (the sort is stable); sequential fp64 sums
__global__ __launch_bounds__(256) void voxel_sums_kernel(const float* __restrict__ p, const uint8_t* __restrict__ col,
                                                         const uint32_t* __restrict__ idx, const uint32_t* __restrict__ starts, int64_t n_voxels,
                                                         float* __restrict__ out_p, uint8_t* __restrict__ out_c, int32_t* __restrict__ counts) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n_voxels) return;
  const uint32_t b = starts[v], e = starts[v + 1];
  double sx = 0.0, sy = 0.0, sz = 0.0, sr = 0.0, sg = 0.0, sb = 0.0;
  for (uint32_t q = b; q < e; ++q) {
    const int64_t i = idx[q];
    sx += (double)p[i * 3 + 0];
    sy += (double)p[i * 3 + 1];
    sz += (double)p[i * 3 + 2];
    if (col) {
      sr += (double)col[i * 3 + 0] / 255.0;
      sg += (double)col[i * 3 + 1] / 255.0;
      sb += (double)col[i * 3 + 2] / 255.0;
    }
  }
  const double cnt = (double)(e - b);
  out_p[v * 3 + 0] = (float)(sx / cnt);
  out_p[v * 3 + 1] = (float)(sy / cnt);
  out_p[v * 3 + 2] = (float)(sz / cnt);
  if (col) {  // averages of values in [0, 1] times 255.0 lie in [0, 255]: the truncation needs no saturation
    out_c[v * 3 + 0] = (uint8_t)(int)(sr / cnt * 255.0);
    out_c[v * 3 + 1] = (uint8_t)(int)(sg / cnt * 255.0);
    out_c[v * 3 + 2] = (uint8_t)(int)(sb / cnt * 255.0);
  }
  counts[v] = (int32_t)(e - b);
}

// ---------------------------------------------------------------------------------------------------------------------------
// farthest point sampling
__device__ __forceinline__ void take_better(double od, int32_t oi, double& d, int32_t& i) {  // (larger distance, then smaller index)
  if (od > d || (od == d && oi < i)) {
    d = od;
    i = oi;
  }
}

__device__ __forceinline__ void wave_best(double& d, int32_t& i) {  // every lane ends with the wave's best: the order is total
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double od = __shfl_xor(d, off, 64);
    const int32_t oi = __shfl_xor(i, off, 64);
    take_better(od, oi, d, i);
  }
}

// the workgroup's best in every thread.  sd / si: NT / 64 LDS slots that no thread writes again before the next barrier it passes
template <int NT>
__device__ __forceinline__ void block_best(double& d, int32_t& i, double* sd, int32_t* si) {
  wave_best(d, i);
  if ((threadIdx.x & 63) == 0) {
    sd[threadIdx.x >> 6] = d;
    si[threadIdx.x >> 6] = i;
  }
  __syncthreads();
  d = sd[0];
  i = si[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) take_better(sd[w], si[w], d, i);
}

__device__ __forceinline__ double sq_dist(float x, float y, float z, double sx, double sy, double sz) {
  const double dx = (double)x - sx, dy = (double)y - sy, dz = (double)z - sz;
  return (dx * dx + dy * dy) + dz * dz;
}

// the whole loop in one workgroup: thread t keeps points t, t + NT, .. and their distances in registers
__global__ __launch_bounds__(FPS_ONE_NT) void fps_one_kernel(const float* __restrict__ p, int n, int k, int start, int32_t* __restrict__ selected) {
  __shared__ double sd[2][FPS_ONE_NT / 64];
  __shared__ int32_t si[2][FPS_ONE_NT / 64];
  float px[FPS_ONE_PER], py[FPS_ONE_PER], pz[FPS_ONE_PER];
  double d[FPS_ONE_PER];
#pragma unroll
  for (int s = 0; s < FPS_ONE_PER; ++s) {
    const int j = s * FPS_ONE_NT + threadIdx.x;
    const bool ok = j < n;
    px[s] = ok ? p[(int64_t)j * 3 + 0] : 0.f;
    py[s] = ok ? p[(int64_t)j * 3 + 1] : 0.f;
    pz[s] = ok ? p[(int64_t)j * 3 + 2] : 0.f;
    d[s] = __builtin_inf();
  }
  int far = start;
  for (int it = 0; it < k; ++it) {
    if (threadIdx.x == 0) selected[it] = far;
    if (it == k - 1) break;  // the distances after the last selection are never read
    const double sx = (double)p[(int64_t)far * 3 + 0], sy = (double)p[(int64_t)far * 3 + 1], sz = (double)p[(int64_t)far * 3 + 2];
    double bd = -1.0;
    int32_t bi = 0x7fffffff;
#pragma unroll
    for (int s = 0; s < FPS_ONE_PER; ++s) {
      const int j = s * FPS_ONE_NT + threadIdx.x;
      if (j < n) {
        d[s] = fmin(d[s], sq_dist(px[s], py[s], pz[s], sx, sy, sz));
        take_better(d[s], j, bd, bi);
      }
    }
    block_best<FPS_ONE_NT>(bd, bi, sd[it & 1], si[it & 1]);  // ping-pong: a slot is rewritten two barriers later
    if (bd > 0.0) far = bi;
  }
}

// one iteration of the tiled path: far = the best of the previous launch's partials (launch 0: start), then this workgroup's tiles
__global__ __launch_bounds__(FPS_NT) void fps_tiled_kernel(const float* __restrict__ p, int64_t n, int64_t n_tiles, int it, int start, int update,
                                                           double* __restrict__ d, const double* __restrict__ pd_in,
                                                           const int32_t* __restrict__ pi_in, double* __restrict__ pd_out,
                                                           int32_t* __restrict__ pi_out, int32_t* __restrict__ selected) {
  __shared__ double sd[2][FPS_NT / 64];
  __shared__ int32_t si[2][FPS_NT / 64];
  int far = start;
  if (it > 0) {
    double bd = -1.0;
    int32_t bi = 0x7fffffff;
    for (int q = threadIdx.x; q < (int)gridDim.x; q += FPS_NT) take_better(pd_in[q], pi_in[q], bd, bi);
    block_best<FPS_NT>(bd, bi, sd[0], si[0]);
    far = bd > 0.0 ? bi : selected[it - 1];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) selected[it] = far;
  if (!update) return;
  const double sx = (double)p[(int64_t)far * 3 + 0], sy = (double)p[(int64_t)far * 3 + 1], sz = (double)p[(int64_t)far * 3 + 2];
  double bd = -1.0;
  int32_t bi = 0x7fffffff;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
#pragma unroll
    for (int s = 0; s < FPS_PER; ++s) {
      const int64_t j = tile * FPS_TILE + s * FPS_NT + threadIdx.x;
      if (j < n) {
        double dj = sq_dist(p[j * 3 + 0], p[j * 3 + 1], p[j * 3 + 2], sx, sy, sz);
        if (it > 0) dj = fmin(d[j], dj);  // launch 0 starts from inf: d is written before it is ever read
        d[j] = dj;
        take_better(dj, (int32_t)j, bd, bi);
      }
    }
  }
  block_best<FPS_NT>(bd, bi, sd[1], si[1]);
  if (threadIdx.x == 0) {
    pd_out[blockIdx.x] = bd;
    pi_out[blockIdx.x] = bi;
  }
}

__global__ void cloud_mark_kernel(const int32_t* __restrict__ selected, int64_t k, uint8_t* __restrict__ mask) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < k) mask[selected[i]] = 1;  // repeats store the same byte
}

template <class IDX>
__global__ void cloud_gather_kernel(const float* __restrict__ p, const uint8_t* __restrict__ col, const IDX* __restrict__ index, int64_t m,
                                    float* __restrict__ out_p, uint8_t* __restrict__ out_c) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= m) return;
  const int64_t i = (int64_t)index[o];
#pragma unroll
  for (int a = 0; a < 3; ++a) out_p[o * 3 + a] = p[i * 3 + a];
  if (col) {
#pragma unroll
    for (int a = 0; a < 3; ++a) out_c[o * 3 + a] = col[i * 3 + a];
  }
}

// ---- host
bool cloud_n_ok(int64_t n) { return n >= 1 && n < (1ll << 31); }

struct VoxelWs {
  SortWs<> sort;  // first: the sort's buffers (f3r_sort.h), in the order this workspace has always had them
  uint32_t *idx_a, *hscan, *starts;
  int64_t head_tiles;
  size_t bytes;
};

VoxelWs voxel_ws(void* base, int64_t n) {
  Carve c(base, 256);
  VoxelWs w = {};
  w.head_tiles = (n + CLOUD_TILE - 1) / CLOUD_TILE;
  w.sort = sort_ws(c, n);
  w.idx_a = w.sort.idx_a;
  w.hscan = c.take<uint32_t>(w.head_tiles + 1);
  w.starts = c.take<uint32_t>(n + 1);
  w.bytes = c.bytes();
  return w;
}

int voxel_passes(const int* bits) { return (bits[0] + bits[1] + bits[2] + 7) / 8; }

struct FpsWs {
  double *d, *part_d;
  int32_t* part_i;
  size_t bytes;
};

FpsWs fps_ws(void* base, int64_t n) {
  Carve c(base, 256);
  FpsWs w = {};
  w.d = c.take<double>(n);
  w.part_d = c.take<double>(2 * FPS_MAX_GRID);
  w.part_i = c.take<int32_t>(2 * FPS_MAX_GRID);
  w.bytes = c.bytes();
  return w;
}

}  // namespace

extern "C" int f3r_cloud_combine_count(const int64_t* table, int n_views, int64_t n_tiles, const float* thresholds, uint32_t* scan,
                                       f3r_stream_t stream) {
  F3R_REQUIRE(table && scan, "f3r_cloud_combine_count: null table or scan");
  F3R_REQUIRE(n_views >= 1 && n_tiles >= n_views && n_tiles < (1ll << 31), "f3r_cloud_combine_count: %d views, %lld tiles; need at least one view and one tile per view",
              n_views, (long long)n_tiles);
  hipStream_t s = (hipStream_t)stream;
  const ViewRow* rows = (const ViewRow*)table;
  const int64_t* ts = table + (int64_t)n_views * 12;
  hipLaunchKernelGGL(combine_count_kernel, dim3((unsigned)n_tiles), dim3(64), 0, s, rows, ts, n_views, thresholds, scan, n_tiles);
  hipLaunchKernelGGL(exclusive_scan_rows_kernel<SCAN_NT>, dim3(1), dim3(SCAN_NT), 0, s, scan, (const int64_t*)nullptr, n_tiles + 1,
                     (uint32_t*)nullptr);
  return f3r_check_launch("f3r_cloud_combine_count");
}

extern "C" int f3r_cloud_combine_write(const int64_t* table, int n_views, int64_t n_tiles, const float* thresholds, const uint32_t* scan,
                                       int flip_axes, float* points, uint8_t* colors, f3r_stream_t stream) {
  F3R_REQUIRE(table && scan && points && colors, "f3r_cloud_combine_write: null pointer");
  F3R_REQUIRE(n_views >= 1 && n_tiles >= n_views && n_tiles < (1ll << 31), "f3r_cloud_combine_write: %d views, %lld tiles; need at least one view and one tile per view",
              n_views, (long long)n_tiles);
  const ViewRow* rows = (const ViewRow*)table;
  const int64_t* ts = table + (int64_t)n_views * 12;
  hipLaunchKernelGGL(combine_write_kernel, dim3((unsigned)n_tiles), dim3(64), 0, (hipStream_t)stream, rows, ts, n_views, thresholds, scan,
                     flip_axes ? 1 : 0, points, colors);
  return f3r_check_launch("f3r_cloud_combine_write");
}

extern "C" int f3r_cloud_bounds(const float* points, int64_t n, uint32_t* out, f3r_stream_t stream) {
  F3R_REQUIRE(points && out, "f3r_cloud_bounds: null pointer");
  F3R_REQUIRE(cloud_n_ok(n), "f3r_cloud_bounds: n = %lld; need 1 <= n < 2^31", (long long)n);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(bounds_init_kernel, dim3(1), dim3(64), 0, s, out);
  const unsigned grid = std::min<unsigned>(blocks_of(n, BOUNDS_NT * 8), 2048u);
  hipLaunchKernelGGL(bounds_kernel, dim3(grid), dim3(BOUNDS_NT), 0, s, points, n, out);
  return f3r_check_launch("f3r_cloud_bounds");
}

extern "C" size_t f3r_cloud_voxel_workspace_bytes(int64_t n) {
  if (!cloud_n_ok(n)) return 0;
  return voxel_ws(nullptr, n).bytes;
}

extern "C" int f3r_cloud_voxel_sort(const float* points, int64_t n, const double* min_bound, double voxel_size, const int* bits, void* workspace,
                                    size_t workspace_bytes, uint32_t* n_voxels, f3r_stream_t stream) {
  F3R_REQUIRE(points && min_bound && bits && workspace && n_voxels, "f3r_cloud_voxel_sort: null pointer");
  F3R_REQUIRE(cloud_n_ok(n), "f3r_cloud_voxel_sort: n = %lld; need 1 <= n < 2^31", (long long)n);
  F3R_REQUIRE(voxel_size > 0.0 && voxel_size < __builtin_inf(), "f3r_cloud_voxel_sort: voxel_size = %g; need a finite value > 0", voxel_size);
  for (int a = 0; a < 3; ++a) {
    F3R_REQUIRE(bits[a] >= 0 && bits[a] <= 31, "f3r_cloud_voxel_sort: bits[%d] = %d outside [0, 31]", a, bits[a]);
    F3R_REQUIRE(min_bound[a] == min_bound[a] && min_bound[a] - min_bound[a] == 0.0, "f3r_cloud_voxel_sort: min_bound[%d] is not finite", a);
  }
  F3R_REQUIRE(bits[0] + bits[1] + bits[2] <= 63, "f3r_cloud_voxel_sort: %d key bits; at most 63 (voxel_size too small for this extent)",
              bits[0] + bits[1] + bits[2]);
  const VoxelWs w = voxel_ws(workspace, n);
  F3R_REQUIRE(workspace_bytes >= w.bytes, "f3r_cloud_voxel_sort: workspace too small (%zu bytes; need %zu)", workspace_bytes, w.bytes);
  hipStream_t s = (hipStream_t)stream;
  const double half = 0.5 * voxel_size;
  hipLaunchKernelGGL(voxel_key_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, points, n, min_bound[0] - half, min_bound[1] - half,
                     min_bound[2] - half, voxel_size, bits[1] + bits[2], bits[2], w.sort.keys_a, w.sort.idx_a);
  const uint64_t* kin;
  const uint32_t* vin;
  sort_pairs_lsd(w.sort, n, voxel_passes(bits), s, &kin, &vin);
  const dim3 gh((unsigned)w.head_tiles), bh(64);
  hipLaunchKernelGGL(head_count_kernel, gh, bh, 0, s, kin, n, w.hscan, w.head_tiles);
  hipLaunchKernelGGL(exclusive_scan_rows_kernel<SCAN_NT>, dim3(1), dim3(SCAN_NT), 0, s, w.hscan, (const int64_t*)nullptr, w.head_tiles + 1,
                     (uint32_t*)nullptr);
  hipLaunchKernelGGL(head_starts_kernel, gh, bh, 0, s, kin, n, (const uint32_t*)w.hscan, w.head_tiles, w.starts, n_voxels);
  if (vin != w.idx_a)  // an odd number of passes left the order in the second buffer: the sums read the first
    if (hipMemcpyAsync(w.idx_a, vin, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, s) != hipSuccess) {
      (void)hipGetLastError();
      f3r_set_error("f3r_cloud_voxel_sort: copying the sorted order failed");
      return F3R_ERR_LAUNCH;
    }
  return f3r_check_launch("f3r_cloud_voxel_sort");
}

extern "C" int f3r_cloud_voxel_sums(const float* points, const uint8_t* colors, int64_t n, int64_t n_voxels, const void* workspace,
                                    size_t workspace_bytes, float* out_points, uint8_t* out_colors, int32_t* counts, f3r_stream_t stream) {
  F3R_REQUIRE(points && workspace && out_points && counts && (out_colors || !colors), "f3r_cloud_voxel_sums: null pointer");
  F3R_REQUIRE(cloud_n_ok(n) && n_voxels >= 1 && n_voxels <= n, "f3r_cloud_voxel_sums: n = %lld, n_voxels = %lld; need 1 <= n_voxels <= n < 2^31",
              (long long)n, (long long)n_voxels);
  const VoxelWs w = voxel_ws((void*)workspace, n);
  F3R_REQUIRE(workspace_bytes >= w.bytes, "f3r_cloud_voxel_sums: workspace too small (%zu bytes; need %zu)", workspace_bytes, w.bytes);
  hipLaunchKernelGGL(voxel_sums_kernel, dim3(blocks_of(n_voxels, 256)), dim3(256), 0, (hipStream_t)stream, points, colors,
                     (const uint32_t*)w.idx_a, (const uint32_t*)w.starts, n_voxels, out_points, out_colors, counts);
  return f3r_check_launch("f3r_cloud_voxel_sums");
}

extern "C" size_t f3r_cloud_fps_workspace_bytes(int64_t n) {
  if (!cloud_n_ok(n)) return 0;
  return fps_ws(nullptr, n).bytes;
}

extern "C" int f3r_cloud_fps(const float* points, int64_t n, int64_t num_samples, int64_t start_index, int mode, void* workspace,
                             size_t workspace_bytes, int32_t* selected, f3r_stream_t stream) {
  F3R_REQUIRE(points && selected, "f3r_cloud_fps: null pointer");
  F3R_REQUIRE(cloud_n_ok(n), "f3r_cloud_fps: n = %lld; need 1 <= n < 2^31", (long long)n);
  F3R_REQUIRE(num_samples >= 1 && num_samples <= n, "f3r_cloud_fps: num_samples = %lld outside [1, %lld]", (long long)num_samples, (long long)n);
  F3R_REQUIRE(start_index >= 0 && start_index < n, "f3r_cloud_fps: start_index = %lld outside [0, %lld)", (long long)start_index, (long long)n);
  F3R_REQUIRE(mode >= 0 && mode <= 2, "f3r_cloud_fps: mode = %d; 0 auto, 1 one workgroup, 2 tiled", mode);
  F3R_REQUIRE(mode != 1 || n <= FPS_ONE_MAX, "f3r_cloud_fps: the one-workgroup path takes n <= %d, got %lld", FPS_ONE_MAX, (long long)n);
  hipStream_t s = (hipStream_t)stream;
  if (mode == 1 || (mode == 0 && n <= FPS_ONE_MAX)) {
    hipLaunchKernelGGL(fps_one_kernel, dim3(1), dim3(FPS_ONE_NT), 0, s, points, (int)n, (int)num_samples, (int)start_index, selected);
    return f3r_check_launch("f3r_cloud_fps");
  }
  F3R_REQUIRE(workspace, "f3r_cloud_fps: null workspace");
  const FpsWs w = fps_ws(workspace, n);
  F3R_REQUIRE(workspace_bytes >= w.bytes, "f3r_cloud_fps: workspace too small (%zu bytes; need %zu)", workspace_bytes, w.bytes);
  const int64_t n_tiles = (n + FPS_TILE - 1) / FPS_TILE;
  const unsigned grid = (unsigned)std::min<int64_t>(n_tiles, FPS_MAX_GRID);
  for (int64_t it = 0; it < num_samples; ++it) {
    const int in = (int)((it & 1) ^ 1), out = (int)(it & 1);
    hipLaunchKernelGGL(fps_tiled_kernel, dim3(grid), dim3(FPS_NT), 0, s, points, n, n_tiles, (int)it, (int)start_index,
                       it + 1 < num_samples ? 1 : 0, w.d, (const double*)(w.part_d + in * FPS_MAX_GRID),
                       (const int32_t*)(w.part_i + in * FPS_MAX_GRID), w.part_d + out * FPS_MAX_GRID, w.part_i + out * FPS_MAX_GRID, selected);
  }
  return f3r_check_launch("f3r_cloud_fps");
}

extern "C" int f3r_cloud_mark(const int32_t* selected, int64_t num_samples, int64_t n, uint8_t* mask, f3r_stream_t stream) {
  F3R_REQUIRE(selected && mask, "f3r_cloud_mark: null pointer");
  F3R_REQUIRE(cloud_n_ok(n) && num_samples >= 1 && num_samples <= n, "f3r_cloud_mark: n = %lld, num_samples = %lld; need 1 <= num_samples <= n < 2^31",
              (long long)n, (long long)num_samples);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(mask, 0, (size_t)n, s) != hipSuccess) {
    (void)hipGetLastError();
    f3r_set_error("f3r_cloud_mark: clearing the mask failed");
    return F3R_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(cloud_mark_kernel, dim3(blocks_of(num_samples, 256)), dim3(256), 0, s, selected, num_samples, mask);
  return f3r_check_launch("f3r_cloud_mark");
}

extern "C" int f3r_cloud_gather(const float* points, const uint8_t* colors, const void* index, int index_i64, int64_t n, int64_t m,
                                float* out_points, uint8_t* out_colors, f3r_stream_t stream) {
  F3R_REQUIRE(points && index && out_points && (out_colors || !colors), "f3r_cloud_gather: null pointer");
  F3R_REQUIRE(cloud_n_ok(n) && m >= 1 && m < (1ll << 31), "f3r_cloud_gather: n = %lld, m = %lld; need 1 <= n, m < 2^31", (long long)n, (long long)m);
  const dim3 g(blocks_of(m, 256)), b(256);
  if (index_i64)
    hipLaunchKernelGGL(cloud_gather_kernel<int64_t>, g, b, 0, (hipStream_t)stream, points, colors, (const int64_t*)index, m, out_points, out_colors);
  else
    hipLaunchKernelGGL(cloud_gather_kernel<int32_t>, g, b, 0, (hipStream_t)stream, points, colors, (const int32_t*)index, m, out_points, out_colors);
  return f3r_check_launch("f3r_cloud_gather");
}
