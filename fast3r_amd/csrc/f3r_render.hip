// Point-splat renderer (ABI 430; include/f3r.h "point-splat renderer"): the pictures of render_cumulative_pts3d_viz of the reference's
// notebooks/demo_multiview.ipynb, for a cloud that never leaves the device.  The notebook draws the cloud with pyrender (GL points, a
// perspective camera with zfar = None, no lighting on the point path); here that is a z-buffered splat.
//
// * splat: one thread per point.  The eye-space arithmetic is fp64 in the order the header states, each operation rounded on its own
//   (built with -ffp-contract=off); the point's square is min-reduced into a uint64 key per pixel, (bits of fp32(d) << 32) | point
//   index, with 64-bit integer atomicMin.  d >= znear > 0, so the bits of fp32(d) order as d does.  The smallest key wins: the nearest
//   point, at equal depth the lowest index -- GL_LESS for points drawn in index order.  A relaxed load of the current key skips the atomic
//   when the point already loses; a stale value is never smaller than the current one, so this cannot change the result.
// * resolve: key -> colour of the point in the low word, or the background where the key is all ones; optionally the depth in the high word.
// * centre: the fp64 sum of the coordinates by the order contract of f3r_prims.h (per thread, wave_sum, block_sum), then the workgroups'
//   partials in a second launch of one workgroup, again per thread, wave_sum, block_sum.  The grid is a function of n alone.
// Integer atomics only: two runs give the same bits.
#include "f3r_common.h"
#include "f3r_pixel.h"  // first_center_ge, shared with the triangle rasteriser
#include "f3r_prims.h"

#include <algorithm>

namespace {

constexpr int SPLAT_NT = 256;
constexpr int RESOLVE_NT = 256;
constexpr int CENTER_NT = 256;
constexpr int CENTER_PER = 8;                       // points of one thread of a full first-stage workgroup, at least
constexpr int CENTER_PARTS = F3R_RENDER_CENTER_PARTS;  // first-stage workgroups at most
constexpr uint64_t EMPTY_KEY = ~0ull;

struct Camera {  // the 17 doubles of the entry point, and the viewport
  double v[12];
  double sx, sy, cx, cy, znear;
  double half_w, half_h, half_s;  // W / 2, H / 2, point_size / 2
  int W, H;
};

__global__ __launch_bounds__(SPLAT_NT) void splat_kernel(const float* __restrict__ p, int64_t n0, int64_t n1, Camera c,
                                                         uint64_t* __restrict__ keys) {
  const int64_t idx = n0 + (int64_t)blockIdx.x * SPLAT_NT + threadIdx.x;
  if (idx >= n1) return;
  const double x = (double)p[idx * 3 + 0], y = (double)p[idx * 3 + 1], z = (double)p[idx * 3 + 2];
  const double ex = ((c.v[0] * x + c.v[1] * y) + c.v[2] * z) + c.v[3];
  const double ey = ((c.v[4] * x + c.v[5] * y) + c.v[6] * z) + c.v[7];
  const double ez = ((c.v[8] * x + c.v[9] * y) + c.v[10] * z) + c.v[11];
  const double d = -ez;
  const double px = c.sx * ex + c.cx * d, py = c.sy * ey + c.cy * d;  // clip-space x and y; clip-space w is d
  const float df = (float)d;
  // every comparison fails on a NaN
  if (!(d >= c.znear && fabs(px) <= d && fabs(py) <= d && df < __builtin_inff())) return;
  const double xw = (px / d + 1.0) * c.half_w, yw = (py / d + 1.0) * c.half_h;
  const int i0 = first_center_ge(xw - c.half_s, c.W), i1 = first_center_ge(xw + c.half_s, c.W);
  const int j0 = first_center_ge(yw - c.half_s, c.H), j1 = first_center_ge(yw + c.half_s, c.H);
  const uint64_t key = ((uint64_t)__builtin_bit_cast(uint32_t, df) << 32) | (uint64_t)(uint32_t)idx;
  for (int j = j0; j < j1; ++j) {
    uint64_t* row = keys + (int64_t)(c.H - 1 - j) * c.W;  // window row j is image row H - 1 - j
    for (int i = i0; i < i1; ++i) {
#ifndef F3R_RENDER_NO_EARLY_OUT  // defined by measurement builds only: docs/rows_f.md times the splat with and without this load
      if (__hip_atomic_load(row + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= key) continue;
#endif
      atomicMin((unsigned long long*)(row + i), (unsigned long long)key);
    }
  }
}

__global__ __launch_bounds__(RESOLVE_NT) void resolve_kernel(const uint64_t* __restrict__ keys, const uint8_t* __restrict__ colors, int64_t n,
                                                             int64_t pixels, uint32_t background, uint8_t* __restrict__ image,
                                                             float* __restrict__ depth) {
  const int64_t q = (int64_t)blockIdx.x * RESOLVE_NT + threadIdx.x;
  if (q >= pixels) return;
  const uint64_t k = keys[q];
  const int64_t idx = (int64_t)(k & 0xffffffffull);
  const bool covered = k != EMPTY_KEY && idx < n;  // a key that names no point of this cloud (a caller's error) reads as empty
  uint8_t r = (uint8_t)background, g = (uint8_t)(background >> 8), b = (uint8_t)(background >> 16);
  if (covered) {
    r = colors[idx * 3 + 0];
    g = colors[idx * 3 + 1];
    b = colors[idx * 3 + 2];
  }
  image[q * 3 + 0] = r;
  image[q * 3 + 1] = g;
  image[q * 3 + 2] = b;
  if (depth) depth[q] = covered ? __builtin_bit_cast(float, (uint32_t)(k >> 32)) : __builtin_inff();
}

// stage 1: workgroup b adds points b NT + t, (b + G) NT + t, .. per thread in that order, then block_sum -> parts[b][3]
__global__ __launch_bounds__(CENTER_NT) void center_partial_kernel(const float* __restrict__ p, int64_t n, double* __restrict__ parts) {
  __shared__ double red[CENTER_NT / 64][3];
  double s[3] = {0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * CENTER_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * CENTER_NT) {
    s[0] += (double)p[i * 3 + 0];
    s[1] += (double)p[i * 3 + 1];
    s[2] += (double)p[i * 3 + 2];
  }
  block_sum<3, CENTER_NT, 3>(s, red, parts + (int64_t)blockIdx.x * 3);
}

// stage 2, one workgroup: thread t adds partials t, t + NT, .. in that order, then block_sum -> out[3]
__global__ __launch_bounds__(CENTER_NT) void center_final_kernel(const double* __restrict__ parts, int n_parts, double* __restrict__ out) {
  __shared__ double red[CENTER_NT / 64][3];
  double s[3] = {0.0, 0.0, 0.0};
  for (int q = threadIdx.x; q < n_parts; q += CENTER_NT) {
    s[0] += parts[q * 3 + 0];
    s[1] += parts[q * 3 + 1];
    s[2] += parts[q * 3 + 2];
  }
  block_sum<3, CENTER_NT, 3>(s, red, out);
}

bool is_finite(double v) { return v - v == 0.0; }  // false for NaN and the infinities

bool viewport_ok(int W, int H) { return W >= 1 && H >= 1 && (int64_t)W * H < (1ll << 31); }

}  // namespace

extern "C" int f3r_render_clear(uint64_t* keys, int W, int H, f3r_stream_t stream) {
  F3R_REQUIRE(keys, "f3r_render_clear: null keys");
  F3R_REQUIRE(viewport_ok(W, H), "f3r_render_clear: viewport %d x %d; need W, H >= 1 and W H < 2^31", W, H);
  if (hipMemsetAsync(keys, 0xff, (size_t)W * H * sizeof(uint64_t), (hipStream_t)stream) != hipSuccess) {
    (void)hipGetLastError();
    f3r_set_error("f3r_render_clear: setting the keys failed");
    return F3R_ERR_LAUNCH;
  }
  return 0;
}

extern "C" int f3r_render_splat(const float* points, int64_t n, int64_t n0, int64_t n1, const double* camera, double point_size, int W, int H,
                                uint64_t* keys, f3r_stream_t stream) {
  F3R_REQUIRE(points && camera && keys, "f3r_render_splat: null pointer");
  F3R_REQUIRE(viewport_ok(W, H), "f3r_render_splat: viewport %d x %d; need W, H >= 1 and W H < 2^31", W, H);
  F3R_REQUIRE(n >= 1 && n < (1ll << 32), "f3r_render_splat: n = %lld; need 1 <= n < 2^32 (the key holds a 32-bit point index)", (long long)n);
  F3R_REQUIRE(n0 >= 0 && n0 <= n1 && n1 <= n, "f3r_render_splat: points [%lld, %lld) of %lld; need 0 <= n0 <= n1 <= n", (long long)n0,
              (long long)n1, (long long)n);
  F3R_REQUIRE(is_finite(point_size) && point_size > 0.0, "f3r_render_splat: point_size = %g; need a finite value > 0", point_size);
  for (int k = 0; k < 17; ++k) F3R_REQUIRE(is_finite(camera[k]), "f3r_render_splat: camera[%d] is not finite", k);
  F3R_REQUIRE(camera[16] > 0.0, "f3r_render_splat: znear = %g; need > 0", camera[16]);
  if (n0 == n1) return 0;
  Camera c;
  for (int k = 0; k < 12; ++k) c.v[k] = camera[k];
  c.sx = camera[12];
  c.sy = camera[13];
  c.cx = camera[14];
  c.cy = camera[15];
  c.znear = camera[16];
  c.half_w = (double)W * 0.5;
  c.half_h = (double)H * 0.5;
  c.half_s = point_size * 0.5;
  c.W = W;
  c.H = H;
  hipLaunchKernelGGL(splat_kernel, dim3(blocks_of(n1 - n0, SPLAT_NT)), dim3(SPLAT_NT), 0, (hipStream_t)stream, points, n0, n1, c,
                     keys);
  return f3r_check_launch("f3r_render_splat");
}

extern "C" int f3r_render_resolve(const uint64_t* keys, const uint8_t* colors, int64_t n, int W, int H, uint32_t background, uint8_t* image,
                                  float* depth, f3r_stream_t stream) {
  F3R_REQUIRE(keys && colors && image, "f3r_render_resolve: null pointer");
  F3R_REQUIRE(viewport_ok(W, H), "f3r_render_resolve: viewport %d x %d; need W, H >= 1 and W H < 2^31", W, H);
  F3R_REQUIRE(n >= 1 && n < (1ll << 32), "f3r_render_resolve: n = %lld; need 1 <= n < 2^32", (long long)n);
  F3R_REQUIRE(background < (1u << 24), "f3r_render_resolve: background = 0x%x; need r | g << 8 | b << 16", background);
  const int64_t pixels = (int64_t)W * H;
  hipLaunchKernelGGL(resolve_kernel, dim3(blocks_of(pixels, RESOLVE_NT)), dim3(RESOLVE_NT), 0, (hipStream_t)stream, keys, colors, n, pixels,
                     background, image, depth);
  return f3r_check_launch("f3r_render_resolve");
}

extern "C" int f3r_render_center(const float* points, int64_t n, double* partials, double* out, f3r_stream_t stream) {
  F3R_REQUIRE(points && partials && out, "f3r_render_center: null pointer");
  F3R_REQUIRE(n >= 1 && n < (1ll << 32), "f3r_render_center: n = %lld; need 1 <= n < 2^32", (long long)n);
  hipStream_t s = (hipStream_t)stream;
  const int grid = (int)std::min<int64_t>((n + CENTER_NT * CENTER_PER - 1) / (CENTER_NT * CENTER_PER), CENTER_PARTS);
  hipLaunchKernelGGL(center_partial_kernel, dim3(grid), dim3(CENTER_NT), 0, s, points, n, partials);
  hipLaunchKernelGGL(center_final_kernel, dim3(1), dim3(CENTER_NT), 0, s, (const double*)partials, grid, out);
  return f3r_check_launch("f3r_render_center");
}
