// Triangle rasteriser (include/f3r.h "triangle rasteriser"): depth-tested, flat-coloured triangles into the key buffer of the point-splat
// renderer (f3r_render.hip), so that meshes (build_mesh) and camera pyramids (camera_meshes) share one picture with the points and
// f3r_render_resolve turns the keys into colours unchanged.
//
// * The arithmetic is fp64 in the order the header states, each operation rounded on its own (built with -ffp-contract=off).  One
//   __device__ function sets a triangle up (setup) and one draws a pixel (pixel): both stages below call them, so both give the same bits.
// * stage 1: one thread per triangle.  A triangle whose pixel box holds at most F3R_RASTER_SMALL_PIXELS pixels is drawn by its thread; a
//   larger one (a rubber sheet across a depth edge, a camera pyramid near the eye) is appended to a queue of face offsets: a ballot
//   compaction per wave and one integer atomicAdd per wave on the queue's counter.
// * stage 2: one wave per queued triangle; the 64 lanes stride over the pixel box.  The waves stride over the queue, whose length they
//   read from the counter: no host round trip between the stages.
// The queue's order depends on arrival; the keys do not, because the 64-bit integer atomicMin commutes.  No floating-point atomics.
#include "f3r_common.h"
#include "f3r_pixel.h"
#include "f3r_prims.h"

#include <algorithm>

namespace {

constexpr int RASTER_NT = 256;
constexpr int RASTER_WAVES = RASTER_NT / 64;
constexpr int STAGE2_BLOCKS = 4096;  // workgroups of stage 2 at most; its waves stride over the queue
constexpr int64_t HEADER_BYTES = 256;  // the workspace's head: uint32 counter (queue length of the launch), uint64 total at byte 8

struct RasterCamera {  // the 17 doubles of the entry point, and the viewport
  double v[12];
  double sx, sy, cx, cy, znear;
  double half_w, half_h;
  int W, H;
};

struct Triangle {
  double x0, y0, x1, y1, x2, y2;  // window coordinates
  double r0, r1, r2, dmin, dmax, A;
  int i0, i1, j0, j1;  // the pixel box: columns [i0, i1), window rows [j0, j1)
};

__device__ __forceinline__ bool finite(double v) { return v - v == 0.0; }  // false for NaN and the infinities

// vertex a of the mesh -> window position and eye distance, as splat_kernel computes them.  false: the vertex is nearer than znear, or a
// comparison met a NaN, or a window coordinate is not finite
__device__ __forceinline__ bool project(const float* __restrict__ vtx, int64_t a, const RasterCamera& c, double& xw, double& yw, double& d) {
  const double x = (double)vtx[a * 3 + 0], y = (double)vtx[a * 3 + 1], z = (double)vtx[a * 3 + 2];
  const double ex = ((c.v[0] * x + c.v[1] * y) + c.v[2] * z) + c.v[3];
  const double ey = ((c.v[4] * x + c.v[5] * y) + c.v[6] * z) + c.v[7];
  const double ez = ((c.v[8] * x + c.v[9] * y) + c.v[10] * z) + c.v[11];
  d = -ez;
  const double px = c.sx * ex + c.cx * d, py = c.sy * ey + c.cy * d;
  if (!(d >= c.znear)) return false;
  xw = (px / d + 1.0) * c.half_w;
  yw = (py / d + 1.0) * c.half_h;
  return finite(xw) && finite(yw);
}

// face f -> t.  false: the face is skipped (an index outside [0, nv), a vertex not drawable, no area).  The indices are checked before
// any vertex is read
template <class I>
__device__ __forceinline__ bool setup(const float* __restrict__ vtx, int64_t nv, const I* __restrict__ faces, int64_t f,
                                      const RasterCamera& c, Triangle& t) {
  const int64_t a = (int64_t)faces[f * 3 + 0], b = (int64_t)faces[f * 3 + 1], cc = (int64_t)faces[f * 3 + 2];
  if (a < 0 || a >= nv || b < 0 || b >= nv || cc < 0 || cc >= nv) return false;
  double d0, d1, d2;
  if (!project(vtx, a, c, t.x0, t.y0, d0)) return false;
  if (!project(vtx, b, c, t.x1, t.y1, d1)) return false;
  if (!project(vtx, cc, c, t.x2, t.y2, d2)) return false;
  t.A = (t.x1 - t.x0) * (t.y2 - t.y0) - (t.y1 - t.y0) * (t.x2 - t.x0);
  if (t.A == 0.0 || !finite(t.A)) return false;
  const double xmin = fmin(fmin(t.x0, t.x1), t.x2), xmax = fmax(fmax(t.x0, t.x1), t.x2);
  const double ymin = fmin(fmin(t.y0, t.y1), t.y2), ymax = fmax(fmax(t.y0, t.y1), t.y2);
  // edges are inclusive: the box ends with the first centre >= the maximum, which the triangle covers when it equals the maximum
  t.i0 = first_center_ge(xmin, c.W);
  t.i1 = min(first_center_ge(xmax, c.W) + 1, c.W);
  t.j0 = first_center_ge(ymin, c.H);
  t.j1 = min(first_center_ge(ymax, c.H) + 1, c.H);
  t.r0 = 1.0 / d0;
  t.r1 = 1.0 / d1;
  t.r2 = 1.0 / d2;
  t.dmin = fmin(fmin(d0, d1), d2);
  t.dmax = fmax(fmax(d0, d1), d2);
  return true;
}

__device__ __forceinline__ int64_t box_pixels(const Triangle& t) {
  return t.i1 > t.i0 && t.j1 > t.j0 ? (int64_t)(t.i1 - t.i0) * (t.j1 - t.j0) : 0;
}

// pixel (column i, window row j) of triangle t: the coverage test, the perspective-correct depth, the key
__device__ __forceinline__ void pixel(const Triangle& t, int i, int j, uint32_t index, const RasterCamera& c, uint64_t* __restrict__ keys) {
  const double cx = (double)i + 0.5, cy = (double)j + 0.5;
  const double w0 = (t.x2 - t.x1) * (cy - t.y1) - (t.y2 - t.y1) * (cx - t.x1);
  const double w1 = (t.x0 - t.x2) * (cy - t.y2) - (t.y0 - t.y2) * (cx - t.x2);
  const double w2 = (t.x1 - t.x0) * (cy - t.y0) - (t.y1 - t.y0) * (cx - t.x0);
  const bool covered = t.A > 0.0 ? (w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0) : (w0 <= 0.0 && w1 <= 0.0 && w2 <= 0.0);
  if (!covered) return;
  const double inv = (w0 * t.r0 + w1 * t.r1) + w2 * t.r2;
  double dd = ((w0 + w1) + w2) / inv;
  if (!(dd >= t.dmin)) dd = t.dmin;  // also where 0 / 0 made a NaN
  if (dd > t.dmax) dd = t.dmax;
  const float df = (float)dd;
  const uint64_t key = ((uint64_t)__builtin_bit_cast(uint32_t, df) << 32) | (uint64_t)index;
  uint64_t* slot = keys + (int64_t)(c.H - 1 - j) * c.W + i;  // window row j is image row H - 1 - j
  if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= key) return;
  atomicMin((unsigned long long*)slot, (unsigned long long)key);
}

// stage 1: faces [fa, fb), one thread each.  queue[k] = the offset f - fa of the k-th large triangle, *counter = their number
template <class I>
__global__ __launch_bounds__(RASTER_NT) void raster_stage1_kernel(const float* __restrict__ vtx, int64_t nv, const I* __restrict__ faces,
                                                                  int64_t fa, int64_t fb, uint32_t index_base, RasterCamera c,
                                                                  uint64_t* __restrict__ keys, uint32_t* __restrict__ counter,
                                                                  uint32_t* __restrict__ queue) {
  const int64_t f = fa + (int64_t)blockIdx.x * RASTER_NT + threadIdx.x;
  bool large = false;
  Triangle t;
  if (f < fb && setup(vtx, nv, faces, f, c, t)) {
    const int64_t pixels = box_pixels(t);
    large = pixels > F3R_RASTER_SMALL_PIXELS;
    if (!large) {
      const uint32_t index = index_base + (uint32_t)f;
      for (int j = t.j0; j < t.j1; ++j)
        for (int i = t.i0; i < t.i1; ++i) pixel(t, i, j, index, c, keys);
    }
  }
  // every lane of the wave arrives here: the ballot ranks the large triangles, lane 0 reserves their slots
  uint64_t ballot;
  const uint32_t rank = compact_rank(large, ballot);
  if (ballot == 0) return;  // uniform over the wave
  uint32_t base = 0;
  if ((threadIdx.x & 63) == 0) base = atomicAdd(counter, (uint32_t)__popcll(ballot));
  base = __shfl(base, 0, 64);
  if (large) queue[base + rank] = (uint32_t)(f - fa);
}

// stage 2: one wave per queued triangle, the lanes stride over its pixel box
template <class I>
__global__ __launch_bounds__(RASTER_NT) void raster_stage2_kernel(const float* __restrict__ vtx, int64_t nv, const I* __restrict__ faces,
                                                                  int64_t fa, int64_t slots, uint32_t index_base, RasterCamera c,
                                                                  uint64_t* __restrict__ keys, const uint32_t* __restrict__ counter,
                                                                  const uint32_t* __restrict__ queue, uint64_t* __restrict__ total) {
  const int64_t count = min((int64_t)*counter, slots);  // never more than the queue holds
  if (blockIdx.x == 0 && threadIdx.x == 0) *total += (uint64_t)count;  // one writer; launches on a stream run in order
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * RASTER_WAVES + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * RASTER_WAVES;
  for (int64_t q = wave; q < count; q += waves) {
    const int64_t off = (int64_t)queue[q];
    if (off >= slots) continue;
    const int64_t f = fa + off;
    Triangle t;
    if (!setup(vtx, nv, faces, f, c, t)) continue;  // the same answer stage 1 got
    const int bw = t.i1 - t.i0;
    const int64_t pixels = box_pixels(t);
    const uint32_t index = index_base + (uint32_t)f;
    for (int64_t p = lane; p < pixels; p += 64) pixel(t, t.i0 + (int)(p % bw), t.j0 + (int)(p / bw), index, c, keys);
  }
}

bool is_finite(double v) { return v - v == 0.0; }

bool viewport_ok(int W, int H) { return W >= 1 && H >= 1 && (int64_t)W * H < (1ll << 31); }

template <class I>
int launch_chunks(const float* vtx, int64_t nv, const void* faces, int64_t f0, int64_t f1, uint32_t index_base, const RasterCamera& c,
                  uint64_t* keys, char* ws, int64_t faces_per_launch, hipStream_t s) {
  uint32_t* counter = (uint32_t*)ws;
  uint64_t* total = (uint64_t*)(ws + 8);
  uint32_t* queue = (uint32_t*)(ws + HEADER_BYTES);
  if (hipMemsetAsync(ws, 0, 16, s) != hipSuccess) return 1;
  for (int64_t fa = f0; fa < f1; fa += faces_per_launch) {
    const int64_t fb = std::min(fa + faces_per_launch, f1), m = fb - fa;
    if (fa != f0 && hipMemsetAsync(counter, 0, sizeof(uint32_t), s) != hipSuccess) return 1;
    hipLaunchKernelGGL(raster_stage1_kernel<I>, dim3(blocks_of(m, RASTER_NT)), dim3(RASTER_NT), 0, s, vtx, nv, (const I*)faces, fa, fb,
                       index_base, c, keys, counter, queue);
    const unsigned grid2 = (unsigned)std::min<int64_t>(blocks_of(m, RASTER_WAVES), STAGE2_BLOCKS);
    hipLaunchKernelGGL(raster_stage2_kernel<I>, dim3(grid2), dim3(RASTER_NT), 0, s, vtx, nv, (const I*)faces, fa, m, index_base, c, keys,
                       (const uint32_t*)counter, (const uint32_t*)queue, total);
  }
  return 0;
}

}  // namespace

extern "C" size_t f3r_raster_workspace_bytes(int64_t faces_per_launch) {
  if (faces_per_launch < 1 || faces_per_launch >= (1ll << 31)) return 0;
  return (size_t)(HEADER_BYTES + faces_per_launch * (int64_t)sizeof(uint32_t));
}

extern "C" int f3r_raster_triangles(const float* vertices, int64_t nv, const void* faces, int index_dtype, int64_t nf, int64_t f0, int64_t f1,
                                    int64_t index_base, const double* camera, int W, int H, uint64_t* keys, void* workspace,
                                    size_t workspace_bytes, int64_t faces_per_launch, f3r_stream_t stream) {
  F3R_REQUIRE(vertices && faces && camera && keys && workspace, "f3r_raster_triangles: null pointer");
  F3R_REQUIRE(viewport_ok(W, H), "f3r_raster_triangles: viewport %d x %d; need W, H >= 1 and W H < 2^31", W, H);
  F3R_REQUIRE(index_dtype == F3R_INDEX_I32 || index_dtype == F3R_INDEX_I64, "f3r_raster_triangles: index_dtype = %d; need F3R_INDEX_I32 or "
              "F3R_INDEX_I64", index_dtype);
  F3R_REQUIRE(nv >= 1, "f3r_raster_triangles: nv = %lld; need >= 1", (long long)nv);
  F3R_REQUIRE(nf >= 0 && f0 >= 0 && f0 <= f1 && f1 <= nf, "f3r_raster_triangles: faces [%lld, %lld) of %lld; need 0 <= f0 <= f1 <= nf",
              (long long)f0, (long long)f1, (long long)nf);
  F3R_REQUIRE(index_base >= 0 && index_base < (1ll << 32) && index_base + nf < (1ll << 32), "f3r_raster_triangles: index_base = %lld, nf = "
              "%lld; need index_base >= 0 and index_base + nf < 2^32 (the key holds a 32-bit index)", (long long)index_base, (long long)nf);
  for (int k = 0; k < 17; ++k) F3R_REQUIRE(is_finite(camera[k]), "f3r_raster_triangles: camera[%d] is not finite", k);
  F3R_REQUIRE(camera[16] > 0.0, "f3r_raster_triangles: znear = %g; need > 0", camera[16]);
  F3R_REQUIRE(faces_per_launch >= 1 && faces_per_launch < (1ll << 31), "f3r_raster_triangles: faces_per_launch = %lld; need 1 <= "
              "faces_per_launch < 2^31", (long long)faces_per_launch);
  F3R_REQUIRE(workspace_bytes >= f3r_raster_workspace_bytes(faces_per_launch), "f3r_raster_triangles: workspace of %zu bytes; need %zu "
              "(f3r_raster_workspace_bytes)", workspace_bytes, f3r_raster_workspace_bytes(faces_per_launch));
  F3R_REQUIRE((uintptr_t)workspace % 8 == 0, "f3r_raster_triangles: the workspace must be 8-byte aligned");
  if (f0 == f1) return 0;
  RasterCamera c;
  for (int k = 0; k < 12; ++k) c.v[k] = camera[k];
  c.sx = camera[12];
  c.sy = camera[13];
  c.cx = camera[14];
  c.cy = camera[15];
  c.znear = camera[16];
  c.half_w = (double)W * 0.5;
  c.half_h = (double)H * 0.5;
  c.W = W;
  c.H = H;
  hipStream_t s = (hipStream_t)stream;
  const int failed = index_dtype == F3R_INDEX_I64
                         ? launch_chunks<int64_t>(vertices, nv, faces, f0, f1, (uint32_t)index_base, c, keys, (char*)workspace, faces_per_launch, s)
                         : launch_chunks<int32_t>(vertices, nv, faces, f0, f1, (uint32_t)index_base, c, keys, (char*)workspace, faces_per_launch, s);
  if (failed) {
    (void)hipGetLastError();
    f3r_set_error("f3r_raster_triangles: clearing the queue's counter failed");
    return F3R_ERR_LAUNCH;
  }
  return f3r_check_launch("f3r_raster_triangles");
}
