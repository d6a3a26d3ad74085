// Map pictures (include/f3r.h "map pictures"): the images of plot_confidence_maps, maybe_plot_local_depth_and_conf and plot_rgb_images of
// the reference's notebooks/demo_multiview.ipynb, i.e. what matplotlib.pylab.imsave(path, map, cmap=...) and imsave(path, uint8 image)
// write.  One call covers every map of a sheet through a per-map device table; a map may be a channel of an interleaved tensor read in
// place (element stride) and lands at its own row pitch, so a cell of a contact sheet is written directly.
// * maps_range_kernel: per map the fp32 minimum and maximum as order-preserving integer keys, min- and max-reduced with integer atomics
//   (no order dependence: two runs give the same bits); a NaN anywhere makes the maximum's key all ones, which reads back as "both NaN".
// * maps_color_kernel: matplotlib's Normalize and Colormap.__call__(bytes=True), one rounded operation at a time (this file is built with
//   -ffp-contract=off): an fp32 subtraction, a correctly rounded fp64 division by the fp64 range rounded to fp32, an fp32 multiplication,
//   through a 256-entry table staged in LDS as RGBA words.
// * maps_rgb_kernel: trunc((x + 1) * 127.5) clipped to 0..255 per channel of three fp32 planes, alpha 255.
// A tile is F3R_MAPS_TILE = 1024 consecutive pixels of one map: 256 threads x 4 pixels.  A thread's four pixels are read as one 16-byte
// load when the map is dense (element stride 1) and its base 16-byte aligned, and written as one 16-byte store when they lie in one row at
// a 16-byte aligned address; otherwise pixel by pixel (the strided channel, a base that is not aligned, a row's end, the map's tail).
#include <algorithm>

#include "f3r_prims.h"

namespace {

constexpr int MAPS_NT = 256;
constexpr int MAPS_PER = 4;                       // pixels per thread
constexpr int MAPS_TILE = MAPS_NT * MAPS_PER;     // F3R_MAPS_TILE
constexpr int MAPS_ROW = 6;                       // words of a table row
constexpr unsigned MAPS_MAX_GRID = 2048;          // workgroups of a launch, at most: each takes a contiguous run of tiles
constexpr uint32_t KEY_POS_INF = 0xff800000u;     // fkey(+inf): the largest key of a value that is not a NaN
static_assert(MAPS_TILE == F3R_MAPS_TILE, "F3R_MAPS_TILE");

struct MapRow {
  const float* src;
  int64_t stride;
  int H, W;
  uint8_t* dst;
  int64_t pitch;
};

__device__ __forceinline__ MapRow load_row(const int64_t* __restrict__ table, int m) {
  const int64_t* r = table + (int64_t)m * MAPS_ROW;
  return {(const float*)r[0], r[1], (int)r[2], (int)r[3], (uint8_t*)r[4], r[5]};
}

// the thread's four pixels p0 .. p0 + 3 of plane `src` (n pixels, element stride `stride`); entries at or beyond n are left alone
__device__ __forceinline__ void load4(const float* __restrict__ src, int64_t stride, int p0, int n, bool dense16, float v[MAPS_PER]) {
  if (dense16 && p0 + MAPS_PER <= n) {
    const float4v q = *reinterpret_cast<const float4v*>(src + p0);
#pragma unroll
    for (int j = 0; j < MAPS_PER; ++j) v[j] = q[j];
  } else {
#pragma unroll
    for (int j = 0; j < MAPS_PER; ++j)
      if (p0 + j < n) v[j] = src[(int64_t)(p0 + j) * stride];
  }
}

// the thread's four RGBA words to pixels p0 .. p0 + 3 of a W-wide picture at dst, row pitch `pitch` bytes
__device__ __forceinline__ void store4(uint8_t* __restrict__ dst, int64_t pitch, int W, int p0, int n, const uint32_t c[MAPS_PER]) {
  const int y = p0 / W, x = p0 - y * W;
  uint8_t* at = dst + (int64_t)y * pitch + 4 * (int64_t)x;
  if (p0 + MAPS_PER <= n && x + MAPS_PER <= W && (reinterpret_cast<uintptr_t>(at) & 15u) == 0) {
    *reinterpret_cast<u32x4*>(at) = u32x4{c[0], c[1], c[2], c[3]};
    return;
  }
  int yy = y, xx = x;
#pragma unroll
  for (int j = 0; j < MAPS_PER; ++j) {
    if (p0 + j >= n) break;
    *reinterpret_cast<uint32_t*>(dst + (int64_t)yy * pitch + 4 * (int64_t)xx) = c[j];
    if (++xx == W) { xx = 0; ++yy; }
  }
}

__global__ void maps_init_kernel(uint32_t* __restrict__ keys, int n_maps) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m < n_maps) {
    keys[2 * m] = ~0u;
    keys[2 * m + 1] = 0u;
  }
}

// Work distribution of the three tile kernels: workgroup b takes the tiles [b chunk, (b + 1) chunk), chunk = ceil(n_tiles / gridDim.x): a
// contiguous run, so it finds its first map by one search and then walks the table forward, streams consecutive memory, and (the range
// pass) reduces across the workgroup once per map it touches, not once per tile.  Two consecutive tiles of one map are taken together, both
// loads issued before either is used.
struct Chunk {
  int64_t tile, end;
  int m;
};
__device__ __forceinline__ Chunk chunk_of(const int64_t* __restrict__ starts, int n_maps, int64_t n_tiles) {
  const int64_t per = (n_tiles + gridDim.x - 1) / gridDim.x, t0 = (int64_t)blockIdx.x * per;
  Chunk c{t0, min(t0 + per, n_tiles), 0};
  if (c.tile < c.end) c.m = last_le(starts, 0, n_maps, c.tile);
  return c;
}
constexpr int MAPS_PAIR = 2;   // tiles taken together

__global__ __launch_bounds__(MAPS_NT) void maps_range_kernel(const int64_t* __restrict__ table, int n_maps, int64_t n_tiles,
                                                             uint32_t* __restrict__ keys) {
  __shared__ uint32_t red[MAPS_NT / 64][2];
  const int64_t* starts = table + (int64_t)n_maps * MAPS_ROW;
  Chunk c = chunk_of(starts, n_maps, n_tiles);
  uint32_t lo = ~0u, hi = 0u;
  auto flush = [&](int m) {   // every thread calls it: the workgroup's extremes of map m go to its keys
    block_min_max<MAPS_NT>(lo, hi, red);
    if (threadIdx.x == 0) {
      atomicMin(&keys[2 * m], lo);
      atomicMax(&keys[2 * m + 1], hi);
    }
    lo = ~0u;
    hi = 0u;
  };
  while (c.tile < c.end) {
    if (c.tile >= starts[c.m + 1]) {
      flush(c.m);
      do ++c.m; while (c.tile >= starts[c.m + 1]);
    }
    const MapRow r = load_row(table, c.m);
    const int n = r.H * r.W, steps = (int)min((int64_t)MAPS_PAIR, min(c.end, starts[c.m + 1]) - c.tile);
    const bool dense16 = r.stride == 1 && (reinterpret_cast<uintptr_t>(r.src) & 15u) == 0;
    float v[MAPS_PAIR][MAPS_PER];
    int p0[MAPS_PAIR];
#pragma unroll
    for (int s = 0; s < MAPS_PAIR; ++s) {
      p0[s] = (int)(c.tile + s - starts[c.m]) * MAPS_TILE + (int)threadIdx.x * MAPS_PER;
      if (s < steps && p0[s] < n) load4(r.src, r.stride, p0[s], n, dense16, v[s]);
    }
#pragma unroll
    for (int s = 0; s < MAPS_PAIR; ++s) {
      if (s < steps && p0[s] < n) {
#pragma unroll
        for (int j = 0; j < MAPS_PER; ++j) {
          if (p0[s] + j < n) {
            const uint32_t k = v[s][j] != v[s][j] ? ~0u : fkey(v[s][j]);   // a NaN: beyond every value on both sides
            lo = min(lo, k);
            hi = max(hi, k);
          }
        }
      }
    }
    c.tile += steps;
  }
  if (c.end > (int64_t)blockIdx.x * ((n_tiles + gridDim.x - 1) / gridDim.x)) flush(c.m);   // a workgroup without tiles has nothing to add
}

__global__ __launch_bounds__(MAPS_NT) void maps_color_kernel(const int64_t* __restrict__ table, int n_maps, int64_t n_tiles,
                                                             const uint8_t* __restrict__ lut, const uint32_t* __restrict__ keys,
                                                             float* __restrict__ ranges) {
  __shared__ uint32_t rgba[256];
  static_assert(MAPS_NT == 256, "one table entry per thread");
  rgba[threadIdx.x] = (uint32_t)lut[3 * threadIdx.x] | (uint32_t)lut[3 * threadIdx.x + 1] << 8 | (uint32_t)lut[3 * threadIdx.x + 2] << 16 | 0xff000000u;
  __syncthreads();
  const int64_t* starts = table + (int64_t)n_maps * MAPS_ROW;
  Chunk c = chunk_of(starts, n_maps, n_tiles);
  while (c.tile < c.end) {
    while (c.tile >= starts[c.m + 1]) ++c.m;
    const MapRow r = load_row(table, c.m);
    const int n = r.H * r.W, steps = (int)min((int64_t)MAPS_PAIR, min(c.end, starts[c.m + 1]) - c.tile);
    const uint32_t khi = keys[2 * c.m + 1];
    const bool has_nan = khi > KEY_POS_INF;
    const float qnan = __builtin_bit_cast(float, 0x7fc00000u);
    const float vmin = has_nan ? qnan : fkey_inv(keys[2 * c.m]), vmax = has_nan ? qnan : fkey_inv(khi);
    if (c.tile == starts[c.m] && threadIdx.x == 0) {
      ranges[2 * c.m] = vmin;
      ranges[2 * c.m + 1] = vmax;
    }
    const bool flat = vmin == vmax;
    const double span = (double)vmax - (double)vmin;   // fp64, as numpy computes it from matplotlib's Python floats: finite where fp32 overflows
    const bool dense16 = r.stride == 1 && (reinterpret_cast<uintptr_t>(r.src) & 15u) == 0;
    float v[MAPS_PAIR][MAPS_PER];
    int p0[MAPS_PAIR];
#pragma unroll
    for (int s = 0; s < MAPS_PAIR; ++s) {
      p0[s] = (int)(c.tile + s - starts[c.m]) * MAPS_TILE + (int)threadIdx.x * MAPS_PER;
      if (s < steps && p0[s] < n) load4(r.src, r.stride, p0[s], n, dense16, v[s]);
    }
#pragma unroll
    for (int s = 0; s < MAPS_PAIR; ++s) {
      if (s < steps && p0[s] < n) {
        uint32_t col[MAPS_PER];
#pragma unroll
        for (int j = 0; j < MAPS_PER; ++j) {
          if (p0[s] + j >= n) break;
          const float x = flat ? 0.f : (float)((double)(v[s][j] - vmin) / span);
          float xa = x * 256.f;
          if (xa == 256.f) xa = 255.f;
          if (xa != xa) {
            col[j] = 0u;                                // the colormap's "bad" entry: transparent black
          } else {
            const int i = xa < 0.f ? 0 : (xa >= 256.f ? 255 : (int)xa);   // under and over take the end colours; in between, truncation
            col[j] = rgba[i];
          }
        }
        store4(r.dst, r.pitch, r.W, p0[s], n, col);
      }
    }
    c.tile += steps;
  }
}

__global__ __launch_bounds__(MAPS_NT) void maps_rgb_kernel(const int64_t* __restrict__ table, int n_maps, int64_t n_tiles) {
  const int64_t* starts = table + (int64_t)n_maps * MAPS_ROW;
  Chunk c = chunk_of(starts, n_maps, n_tiles);
  for (; c.tile < c.end; ++c.tile) {
    while (c.tile >= starts[c.m + 1]) ++c.m;
    const MapRow r = load_row(table, c.m);
    const int n = r.H * r.W, p0 = (int)(c.tile - starts[c.m]) * MAPS_TILE + (int)threadIdx.x * MAPS_PER;
    if (p0 >= n) continue;
    float v[3][MAPS_PER];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float* plane = r.src + (int64_t)ch * n * r.stride;
      const bool dense16 = r.stride == 1 && (reinterpret_cast<uintptr_t>(plane) & 15u) == 0;
      load4(plane, r.stride, p0, n, dense16, v[ch]);
    }
    uint32_t col[MAPS_PER] = {0xff000000u, 0xff000000u, 0xff000000u, 0xff000000u};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
#pragma unroll
      for (int j = 0; j < MAPS_PER; ++j)
        if (p0 + j < n) col[j] |= (uint32_t)colour_u8(v[ch][j]) << (8 * ch);
    store4(r.dst, r.pitch, r.W, p0, n, col);
  }
}

}  // namespace

extern "C" int f3r_maps_colorize(const int64_t* table, const int64_t* host_rows, int n_maps, int64_t n_tiles, int mode, const uint8_t* lut,
                                 uint32_t* keys, float* ranges, f3r_stream_t stream) {
  F3R_REQUIRE(table && host_rows, "f3r_maps_colorize: null table or host_rows");
  F3R_REQUIRE(n_maps >= 1, "f3r_maps_colorize: n_maps = %d; need >= 1", n_maps);
  F3R_REQUIRE(mode == F3R_MAPS_LUT || mode == F3R_MAPS_RGB, "f3r_maps_colorize: unknown mode %d", mode);
  F3R_REQUIRE(mode == F3R_MAPS_RGB || (lut && keys && ranges), "f3r_maps_colorize: null lut, keys or ranges");
  int64_t tiles = 0;
  for (int m = 0; m < n_maps; ++m) {
    const int64_t* r = host_rows + (int64_t)m * MAPS_ROW;
    const int64_t src = r[0], stride = r[1], H = r[2], W = r[3], dst = r[4], pitch = r[5];
    F3R_REQUIRE(src && dst, "f3r_maps_colorize: map %d: null source or destination", m);
    F3R_REQUIRE(H >= 1 && W >= 1 && H <= (1ll << 30) && W <= (1ll << 30) && H * W <= (1ll << 30),
                "f3r_maps_colorize: map %d is %lld x %lld; need H, W >= 1 and H W <= 2^30", m, (long long)H, (long long)W);
    F3R_REQUIRE(stride >= 1 && stride < (1ll << 31), "f3r_maps_colorize: map %d: element stride %lld; need 1 <= stride < 2^31", m, (long long)stride);
    F3R_REQUIRE(pitch >= 4 * W, "f3r_maps_colorize: map %d: pitch %lld is smaller than 4 W = %lld", m, (long long)pitch, (long long)(4 * W));
    F3R_REQUIRE((src & 3) == 0 && (dst & 3) == 0 && (pitch & 3) == 0, "f3r_maps_colorize: map %d: source, destination and pitch must be 4-byte aligned", m);
    tiles += (H * W + MAPS_TILE - 1) / MAPS_TILE;
  }
  F3R_REQUIRE(tiles == n_tiles, "f3r_maps_colorize: n_tiles = %lld, the maps have %lld tiles of %d pixels", (long long)n_tiles, (long long)tiles, MAPS_TILE);
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = (unsigned)std::min<int64_t>(n_tiles, MAPS_MAX_GRID);
  if (mode == F3R_MAPS_RGB) {
    hipLaunchKernelGGL(maps_rgb_kernel, dim3(grid), dim3(MAPS_NT), 0, s, table, n_maps, n_tiles);
    return f3r_check_launch("f3r_maps_colorize");
  }
  hipLaunchKernelGGL(maps_init_kernel, dim3(blocks_of(n_maps, 256)), dim3(256), 0, s, keys, n_maps);
  hipLaunchKernelGGL(maps_range_kernel, dim3(grid), dim3(MAPS_NT), 0, s, table, n_maps, n_tiles, keys);
  hipLaunchKernelGGL(maps_color_kernel, dim3(grid), dim3(MAPS_NT), 0, s, table, n_maps, n_tiles, lut, keys, ranges);
  return f3r_check_launch("f3r_maps_colorize");
}
