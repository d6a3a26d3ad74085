// Cross-view occlusion filter for confidences (BasePCOptimizer.clean_pointcloud, fast3r/dust3r/cloud_opt/base_opt.py:279-317) on the GPU.
// Every pixel of view i is projected into the cameras of its neighbours j; one that lands in front of camera j's depth map and is less
// confident than the pixel it lands on has its confidence clipped to max_bad_conf.
//   * within one i the loop over j is an OR: the clip is idempotent and before its first clip the pixel holds its input value, so a pixel ends
//     clipped iff some j says "in cone, in front, c_i (the input) < res_j".  All pixels and all j of view i run in parallel, with early exit;
//   * across i it is sequential: view i reads res_j, cleaned already for j < i and still the input for j > i.  One launch per target view, in
//     ascending order on one stream; a launch reads the working copy of the other views and writes only view i's slice (i is never its own
//     neighbour: the entry point refuses such a list), so nothing races inside a launch and nothing waits on another workgroup.
// The view table (one row per view: the world-to-camera matrix, the pinhole, the shape, the 64-bit element offset) is written by the prologue
// from the fp64 closed-form inverse of the pose.  Row j is the same for every lane of a wave: it is read through a wave-uniform index.
// docs/rows_f.md "clean_pointcloud" has the contract and the argument.
#include "f3r_common.h"

#include <cmath>
#include <cstddef>

#include "f3r_prims.h"

// build.sh compiles this file with -ffp-contract=off: every product, sum and quotient below is rounded on its own, in the order written, and
// tests/clean_ref.py repeats them as separate fp32 tensor operations.  Plain `/` and rintf: no approximate reciprocal.

namespace {

constexpr int CLEAN_NT = 256;                  // one thread per pixel of the target view
constexpr int CLEAN_MAX_SIDE = 1 << 24;        // H, W exact as floats: the cone test compares rounded floats with them

struct alignas(16) CleanView {  // 80 bytes
  float m[12];                  // world -> camera, rows of 4
  float fx, fy, cx, cy;
  int32_t H, W;
  int64_t off;                  // first element of the view in conf / depth / out (and, times 3, in pts)
};

// ---- prologue: out = conf, n_lowered = 0, and per view the table row.  table: int64 [N][3] = H, W, offset
__global__ __launch_bounds__(CLEAN_NT) void clean_prologue_kernel(const float* __restrict__ conf, float* __restrict__ out, int64_t total,
                                                                  const float* __restrict__ poses, const float* __restrict__ intr,
                                                                  const int64_t* __restrict__ table, int N, CleanView* __restrict__ views,
                                                                  uint32_t* __restrict__ n_lowered, uint32_t* __restrict__ flag) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = t; e < total; e += stride) out[e] = conf[e];
  for (int64_t v = t; v < N; v += stride) {
    n_lowered[v] = 0u;
    const float* P = poses + 16 * v;
    double a[3][3], tr[3];
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) a[r][c] = (double)P[4 * r + c];
      tr[r] = (double)P[4 * r + 3];
    }
    double co[3][3];  // the adjugate: inverse = co / det
    co[0][0] = a[1][1] * a[2][2] - a[1][2] * a[2][1];
    co[0][1] = a[0][2] * a[2][1] - a[0][1] * a[2][2];
    co[0][2] = a[0][1] * a[1][2] - a[0][2] * a[1][1];
    co[1][0] = a[1][2] * a[2][0] - a[1][0] * a[2][2];
    co[1][1] = a[0][0] * a[2][2] - a[0][2] * a[2][0];
    co[1][2] = a[0][2] * a[1][0] - a[0][0] * a[1][2];
    co[2][0] = a[1][0] * a[2][1] - a[1][1] * a[2][0];
    co[2][1] = a[0][1] * a[2][0] - a[0][0] * a[2][1];
    co[2][2] = a[0][0] * a[1][1] - a[0][1] * a[1][0];
    const double det = (a[0][0] * co[0][0] + a[0][1] * co[1][0]) + a[0][2] * co[2][0];
    if (!(det != 0.0) || !isfinite(det)) atomicOr(flag, 1u);  // NaN, inf or singular: the caller raises
    CleanView w;
    for (int r = 0; r < 3; ++r) {
      double inv[3];
      for (int c = 0; c < 3; ++c) {
        inv[c] = co[r][c] / det;
        w.m[4 * r + c] = (float)inv[c];
      }
      w.m[4 * r + 3] = (float)(-((inv[0] * tr[0] + inv[1] * tr[1]) + inv[2] * tr[2]));
    }
    w.fx = intr[4 * v + 0];
    w.fy = intr[4 * v + 1];
    w.cx = intr[4 * v + 2];
    w.cy = intr[4 * v + 3];
    w.H = (int32_t)table[3 * v + 0];
    w.W = (int32_t)table[3 * v + 1];
    w.off = table[3 * v + 2];
    views[v] = w;
  }
}

// ---- one target view.  `res` is read at the other views' slices and written at view i's: not __restrict__, not const
__global__ __launch_bounds__(CLEAN_NT) void clean_view_kernel(const float* __restrict__ pts, const float* __restrict__ conf,
                                                              const float* __restrict__ depth, const float* __restrict__ poses,
                                                              const CleanView* __restrict__ views, int N, int i,
                                                              const int64_t* __restrict__ starts, const int32_t* __restrict__ nbr,
                                                              float one_minus_tol, float max_bad_conf, int camera_frame, float* res,
                                                              uint32_t* __restrict__ n_lowered, const uint32_t* __restrict__ flag) {
  if (*flag != 0u) return;  // a pose without an inverse: the caller raises, nothing is tested (the same word for every lane)
  const CleanView& me = views[i];
  const int64_t npix = (int64_t)me.H * me.W, p = (int64_t)blockIdx.x * CLEAN_NT + threadIdx.x;
  bool live = p < npix;  // lanes past the image stay in the loop's ballots and do nothing
  float x = 0.f, y = 0.f, z = 0.f, c = 0.f;
  if (live) {
    const float* q = pts + 3 * (me.off + p);
    x = q[0];
    y = q[1];
    z = q[2];
    c = conf[me.off + p];  // the input value: only this launch writes view i's slice
    if (camera_frame) {
      const float* T = poses + 16 * (int64_t)i;
      const float xw = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
      const float yw = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
      const float zw = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
      x = xw;
      y = yw;
      z = zw;
    }
  }
  bool bad = false;
  const int64_t k0 = starts[i], k1 = starts[i + 1];
  for (int64_t k = k0; k < k1; ++k) {
    if (!__any(live)) break;  // every lane of the wave has stopped
    const int j = __builtin_amdgcn_readfirstlane(nbr[k]);
    if (j < 0 || j >= N || j == i) continue;  // holds for a list the entry point accepted
    const CleanView& v = views[j];  // wave-uniform address
    if (live) {
      const float X = ((v.m[0] * x + v.m[1] * y) + v.m[2] * z) + v.m[3];
      const float Y = ((v.m[4] * x + v.m[5] * y) + v.m[6] * z) + v.m[7];
      const float Z = ((v.m[8] * x + v.m[9] * y) + v.m[10] * z) + v.m[11];
      const float u = (v.fx * X + v.cx * Z) / Z;
      const float w = (v.fy * Y + v.cy * Z) / Z;
      const float ur = rintf(u), vr = rintf(w);
      // on the rounded floats: NaN fails, -0.0 passes, a huge value is never converted to an integer
      if (Z > 0.f && ur >= 0.f && ur < (float)v.W && vr >= 0.f && vr < (float)v.H) {
        const int64_t e = v.off + ((int64_t)(int)vr * v.W + (int)ur);
        const float d = depth[e], r = res[e];
        if (Z < one_minus_tol * d && c < r) {
          bad = true;
          live = false;
        }
      }
    }
  }
  bool changed = false;
  if (bad) {
    const float lowered = fminf(c, max_bad_conf);
    changed = lowered != c;
    res[me.off + p] = lowered;
  }
  wave_count_add(changed, n_lowered + i);
}

bool aligned(const void* p, size_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

size_t clean_ws_bytes(int N) { return align256((size_t)N * sizeof(CleanView)); }

}  // namespace

extern "C" size_t f3r_clean_workspace_bytes(int n_views) {
  if (n_views < 1) return 0;
  return clean_ws_bytes(n_views);
}

extern "C" int f3r_clean_confidence(const float* pts, const float* conf, const float* depth, const float* poses, const float* intrinsics,
                                    const int64_t* table, const int64_t* table_host, int n_views, const int32_t* nbr, const int32_t* nbr_host,
                                    int64_t n_nbr, double tol, float max_bad_conf, int frame, float* out_conf, uint32_t* n_lowered,
                                    uint32_t* flag, void* workspace, size_t workspace_bytes, f3r_stream_t stream) {
  F3R_REQUIRE(n_views >= 1, "f3r_clean_confidence: n_views = %d; need at least one view", n_views);
  F3R_REQUIRE(pts && conf && depth && poses && intrinsics && table && table_host && out_conf && n_lowered && flag && workspace,
              "f3r_clean_confidence: null pointer");
  F3R_REQUIRE(tol >= 0.0 && tol < 1.0, "f3r_clean_confidence: tol = %g outside [0, 1)", tol);  // NaN fails both
  F3R_REQUIRE(max_bad_conf == max_bad_conf, "f3r_clean_confidence: max_bad_conf is NaN");
  F3R_REQUIRE(frame == F3R_CLEAN_WORLD || frame == F3R_CLEAN_CAMERA, "f3r_clean_confidence: frame = %d (F3R_CLEAN_WORLD or F3R_CLEAN_CAMERA)", frame);
  const int N = n_views;
  int64_t run = 0;
  for (int v = 0; v < N; ++v) {
    const int64_t H = table_host[3 * v], W = table_host[3 * v + 1];
    F3R_REQUIRE(H >= 1 && W >= 1 && H <= CLEAN_MAX_SIDE && W <= CLEAN_MAX_SIDE && H * W <= (int64_t)0x7fffffff,
                "f3r_clean_confidence: view %d is %lld x %lld; need 1 <= H, W <= 2^24 and H W <= 2^31 - 1", v, (long long)H, (long long)W);
    F3R_REQUIRE(table_host[3 * v + 2] == run, "f3r_clean_confidence: the offset of view %d is %lld, the running sum of the shapes is %lld", v,
                (long long)table_host[3 * v + 2], (long long)run);
    run += H * W;
  }
  const int64_t* starts_host = table_host + 3 * (int64_t)N;
  F3R_REQUIRE(n_nbr >= 0 && starts_host[0] == 0 && starts_host[N] == n_nbr, "f3r_clean_confidence: the neighbour lists must start at 0 and end at n_nbr = %lld",
              (long long)n_nbr);
  F3R_REQUIRE(n_nbr == 0 || (nbr && nbr_host), "f3r_clean_confidence: null neighbour list");
  for (int v = 0; v < N; ++v) {
    const int64_t a = starts_host[v], b = starts_host[v + 1];
    F3R_REQUIRE(a <= b && b <= n_nbr, "f3r_clean_confidence: the neighbour list of view %d is [%lld, %lld) of %lld", v, (long long)a, (long long)b,
                (long long)n_nbr);
    for (int64_t k = a; k < b; ++k) {
      const int j = nbr_host[k];
      F3R_REQUIRE(j >= 0 && j < N && j != v, "f3r_clean_confidence: neighbour %d of view %d (a view is not its own neighbour; %d views)", j, v, N);
      F3R_REQUIRE(k == a || nbr_host[k - 1] < j, "f3r_clean_confidence: the neighbours of view %d must ascend", v);
    }
  }
  F3R_REQUIRE(workspace_bytes >= clean_ws_bytes(N) && aligned(workspace, 256), "f3r_clean_confidence: workspace too small / misaligned");
  F3R_REQUIRE(aligned(pts, 4) && aligned(conf, 4) && aligned(depth, 4) && aligned(poses, 4) && aligned(intrinsics, 4) && aligned(table, 8) &&
                  aligned(nbr, 4) && aligned(out_conf, 4) && aligned(n_lowered, 4) && aligned(flag, 4),
              "f3r_clean_confidence: misaligned buffer");
  hipStream_t s = (hipStream_t)stream;
  CleanView* views = (CleanView*)workspace;
  const int64_t total = run;
  (void)hipMemsetAsync(flag, 0, 4, s);
  const unsigned pro_blocks = (unsigned)std::min<int64_t>(std::max<int64_t>(blocks_of(std::max<int64_t>(total, N), CLEAN_NT), 1), 4096);
  hipLaunchKernelGGL(clean_prologue_kernel, dim3(pro_blocks), dim3(CLEAN_NT), 0, s, conf, out_conf, total, poses, intrinsics, table, N, views,
                     n_lowered, flag);
  const int64_t* starts = table + 3 * (int64_t)N;
  const float one_minus_tol = (float)(1.0 - tol);  // the reference's Python double 1 - tol, then a float scalar against a float tensor
  for (int i = 0; i < N; ++i) {
    if (starts_host[i + 1] == starts_host[i]) continue;  // no neighbour: nothing can lower view i
    const int64_t npix = table_host[3 * i] * table_host[3 * i + 1];
    hipLaunchKernelGGL(clean_view_kernel, dim3(blocks_of(npix, CLEAN_NT)), dim3(CLEAN_NT), 0, s, pts, conf, depth, poses,
                       (const CleanView*)views, N, i, starts, nbr, one_minus_tol, max_bad_conf, frame == F3R_CLEAN_CAMERA ? 1 : 0, out_conf,
                       n_lowered, (const uint32_t*)flag);
  }
  return f3r_check_launch("f3r_clean_confidence");
}
