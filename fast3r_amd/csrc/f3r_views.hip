// Ground-truth views (include/f3r.h "ground-truth views"): what the reference's dataset path makes of a posed RGB-D frame --
// BaseStereoViewDataset._crop_resize_if_necessary (fast3r/dust3r/datasets/base/base_stereo_view_dataset.py:165-221), ImgNorm,
// depthmap_to_absolute_camera_coordinates (dust3r/utils/geometry.py:186-243) and transpose_to_landscape -- for a whole launch group: the views
// of a call whose host plans (fast3r_amd/gt_views.py plan_view) are equal.  They share the two crop boxes, the filter tables and the nearest
// tables; each has its own source pointers, intrinsics and pose, read from small device tables.
// * gtview_hpass_lds_kernel (gtview_hpass_kernel for very wide windows) / gtview_vpass_kernel: Pillow's two resampling passes (src/libImaging/Resample.c: 22-bit fixed-point weights, an
//   accumulator that starts at 1 << 21, an arithmetic shift by 22, saturation to 8 bits, an 8-bit intermediate between the passes).  The
//   source is read only inside crop box 1 -- the tables are made for the cropped size, so taps are clipped at the window's edges --, only the
//   columns and rows crop box 2 keeps are computed, and the vertical pass writes the bytes and ((u / 255) - 0.5) / 0.5 as planes in one go,
//   transposed for a portrait group.
// * gtview_unproject_kernel: depth gathered through OpenCV's nearest-neighbour index tables, x = (u - cu) z / fu and y = (v - cv) z / fv in
//   fp64 with every operation rounded (this file is built with -ffp-contract=off) and rounded once to fp32, the world point R X + t in fp32,
//   valid = z > 0 [&& the point is finite].  A depth that is not finite raises one flag word with a plain store.
// A thread owns four consecutive pixels of an output row: twelve bytes of the pictures go out as three words, four floats of a plane or of
// the depth map as one 16-byte store, four points as three, whenever the run lies in one row at an aligned address; otherwise element by
// element (a row's tail, a width that is no multiple of four).  Grids are capped and stride over the work.
#include <algorithm>

#include "f3r_prims.h"

namespace {

constexpr int GTV_NT = 256;
constexpr int GTV_PER = 4;                     // pixels per thread
constexpr unsigned GTV_MAX_GRID = 2048;        // workgroups of a launch, at most
constexpr int GTV_HP_NT = 128;                 // threads of the LDS-staged horizontal pass: a row of 512 outputs is 128 quads
constexpr int GTV_HP_MAX_W = 16384;            // the widest window whose row (48 KB) that pass stages in LDS
constexpr int GTV_CAM = F3R_GTVIEW_CAM_WORDS;  // floats of a row of the camera table: K (9), then the pose (16)

struct GtvGeo {
  int win_x, win_y, win_w, win_h;      // crop box 1 in the frame
  int crop_x, crop_y, out_w, out_h;    // crop box 2 in the resized window
  int transpose;
};

__device__ __forceinline__ uint8_t clip8(int32_t s) {
  s >>= 22;  // arithmetic shift, as Resample.c's clip8
  return (uint8_t)(s < 0 ? 0 : (s > 255 ? 255 : s));
}

// the thread's 4 pixels x 3 bytes to `at`; `n` of them exist
__device__ __forceinline__ void store_rgb4(uint8_t* __restrict__ at, const uint8_t b[3 * GTV_PER], int n) {
  if (n == GTV_PER && (reinterpret_cast<uintptr_t>(at) & 3u) == 0) {
    uint32_t* w = reinterpret_cast<uint32_t*>(at);
#pragma unroll
    for (int i = 0; i < 3; ++i)
      w[i] = (uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 | (uint32_t)b[4 * i + 3] << 24;
    return;
  }
#pragma unroll
  for (int j = 0; j < GTV_PER; ++j)
    if (j < n) {
      at[3 * j] = b[3 * j];
      at[3 * j + 1] = b[3 * j + 1];
      at[3 * j + 2] = b[3 * j + 2];
    }
}

__device__ __forceinline__ void store_f4(float* __restrict__ at, const float v[GTV_PER], int n) {
  if (n == GTV_PER && (reinterpret_cast<uintptr_t>(at) & 15u) == 0) {
    *reinterpret_cast<float4v*>(at) = float4v{v[0], v[1], v[2], v[3]};
    return;
  }
#pragma unroll
  for (int j = 0; j < GTV_PER; ++j)
    if (j < n) at[j] = v[j];
}

// the four output pixels ox0 .. ox0 + 3 of the horizontal pass from `line`, the window's row (in LDS or in memory)
__device__ __forceinline__ void hpass_quad(const uint8_t* line, const GtvGeo& g, const int32_t* __restrict__ bounds,
                                           const int32_t* __restrict__ kk, int ksize, int ox0, int n, uint8_t b[3 * GTV_PER]) {
#pragma unroll
  for (int j = 0; j < GTV_PER; ++j) {
    if (j >= n) break;
    const int o = g.crop_x + ox0 + j;
    const int xmin = max(bounds[2 * o], 0), cnt = min(bounds[2 * o + 1], g.win_w - xmin);   // never beyond the window, whatever the table holds
    const int32_t* k = kk + (int64_t)o * ksize;
    const uint8_t* p = line + 3 * (int64_t)xmin;
    int32_t s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
    for (int x = 0; x < cnt; ++x) {
      const int32_t w = k[x];
      s0 += (int32_t)p[3 * x] * w;
      s1 += (int32_t)p[3 * x + 1] * w;
      s2 += (int32_t)p[3 * x + 2] * w;
    }
    b[3 * j] = clip8(s0);
    b[3 * j + 1] = clip8(s1);
    b[3 * j + 2] = clip8(s2);
  }
}

// horizontal pass: tmp[view][row][out_w][3], row = source row win_y + row0 + row of the window, column = resized column crop_x + ox.
// A workgroup takes one row of one view at a time: it copies the window's 3 win_w bytes to LDS once, as words where the address allows
// (the LDS copy keeps the source's alignment modulo 4), and every output pixel then reads its taps from LDS -- about nine taps of three
// bytes each at a LANCZOS shrink of 1.25, which as byte loads from memory made this the slowest kernel of the three.
__global__ __launch_bounds__(GTV_HP_NT) void gtview_hpass_lds_kernel(const int64_t* __restrict__ srcs, int n_views, GtvGeo g,
                                                                     const int32_t* __restrict__ bounds, const int32_t* __restrict__ kk,
                                                                     int ksize, int row0, int rows, uint8_t* __restrict__ tmp) {
  extern __shared__ __attribute__((aligned(16))) uint8_t gtv_line[];
  const int quads = (g.out_w + GTV_PER - 1) / GTV_PER, nbytes = 3 * g.win_w;
  const int64_t pairs = (int64_t)n_views * rows;
  for (int64_t vr = blockIdx.x; vr < pairs; vr += gridDim.x) {
    const int row = (int)(vr % rows), v = (int)(vr / rows);
    const uint8_t* src = reinterpret_cast<const uint8_t*>(srcs[2 * v]) + (int64_t)(g.win_y + row0 + row) * srcs[2 * v + 1] + 3 * (int64_t)g.win_x;
    const int skew = (int)(reinterpret_cast<uintptr_t>(src) & 3u);       // LDS byte `skew + i` holds src[i]
    const int head = min(nbytes, (4 - skew) & 3), words = (nbytes - head) / 4;
    uint8_t* line = gtv_line + skew;
    for (int i = threadIdx.x; i < head; i += GTV_HP_NT) line[i] = src[i];
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(src + head);
    uint32_t* lw = reinterpret_cast<uint32_t*>(line + head);
    for (int i = threadIdx.x; i < words; i += GTV_HP_NT) lw[i] = sw[i];
    for (int i = head + 4 * words + threadIdx.x; i < nbytes; i += GTV_HP_NT) line[i] = src[i];
    __syncthreads();
    for (int q = threadIdx.x; q < quads; q += GTV_HP_NT) {
      const int ox0 = q * GTV_PER, n = min(GTV_PER, g.out_w - ox0);
      uint8_t b[3 * GTV_PER] = {};
      hpass_quad(line, g, bounds, kk, ksize, ox0, n, b);
      store_rgb4(tmp + ((vr * g.out_w) + ox0) * 3, b, n);
    }
    __syncthreads();
  }
}

// the same pass with the taps read from memory: for a window wider than GTV_HP_MAX_W pixels, whose row does not fit the LDS budget
__global__ __launch_bounds__(GTV_NT) void gtview_hpass_kernel(const int64_t* __restrict__ srcs, int n_views, GtvGeo g,
                                                              const int32_t* __restrict__ bounds, const int32_t* __restrict__ kk, int ksize,
                                                              int row0, int rows, uint8_t* __restrict__ tmp) {
  const int quads = (g.out_w + GTV_PER - 1) / GTV_PER;
  const int64_t total = (int64_t)n_views * rows * quads;
  for (int64_t i = (int64_t)blockIdx.x * GTV_NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * GTV_NT) {
    const int q = (int)(i % quads);
    const int64_t vr = i / quads;
    const int row = (int)(vr % rows), v = (int)(vr / rows);
    const uint8_t* line = reinterpret_cast<const uint8_t*>(srcs[2 * v]) + (int64_t)(g.win_y + row0 + row) * srcs[2 * v + 1] + 3 * (int64_t)g.win_x;
    const int ox0 = q * GTV_PER, n = min(GTV_PER, g.out_w - ox0);
    uint8_t b[3 * GTV_PER] = {};
    hpass_quad(line, g, bounds, kk, ksize, ox0, n, b);
    store_rgb4(tmp + ((vr * g.out_w) + ox0) * 3, b, n);
  }
}

// output pixel (oy, ox) of the landscape layout is pixel (iy, ix) of the cropped picture: the same, or swapped for a portrait group
__device__ __forceinline__ void image_yx(const GtvGeo& g, int oy, int ox, int& iy, int& ix) {
  iy = g.transpose ? ox : oy;
  ix = g.transpose ? oy : ox;
}

// vertical pass over the intermediate: img_u8[view][OH][OW][3] and img[view][3][OH][OW], (OH, OW) = (out_h, out_w), swapped when transposed
__global__ __launch_bounds__(GTV_NT) void gtview_vpass_kernel(const uint8_t* __restrict__ tmp, int n_views, GtvGeo g,
                                                              const int32_t* __restrict__ bounds, const int32_t* __restrict__ kk, int ksize,
                                                              int row0, int rows, uint8_t* __restrict__ img_u8, float* __restrict__ img) {
  const int OW = g.transpose ? g.out_h : g.out_w, OH = g.transpose ? g.out_w : g.out_h;
  const int quads = (OW + GTV_PER - 1) / GTV_PER;
  const int64_t total = (int64_t)n_views * OH * quads;
  for (int64_t i = (int64_t)blockIdx.x * GTV_NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * GTV_NT) {
    const int q = (int)(i % quads);
    const int64_t vr = i / quads;
    const int oy = (int)(vr % OH), v = (int)(vr / OH);
    const int ox0 = q * GTV_PER, n = min(GTV_PER, OW - ox0);
    const uint8_t* plane = tmp + (int64_t)v * rows * g.out_w * 3;
    uint8_t b[3 * GTV_PER] = {};
    float f[3][GTV_PER] = {};
    // four pixels of one picture row share their taps, and their twelve bytes of an intermediate row are three aligned words
    const bool words = !g.transpose && n == GTV_PER && (g.out_w & 3) == 0;
    if (words) {
      const int o = g.crop_y + oy;
      const int first = bounds[2 * o] - row0, cnt = bounds[2 * o + 1];
      const int32_t* k = kk + (int64_t)o * ksize;
      int32_t s[3 * GTV_PER];
#pragma unroll
      for (int e = 0; e < 3 * GTV_PER; ++e) s[e] = 1 << 21;
      for (int y = 0; y < cnt; ++y) {
        const int r = first + y;
        if ((unsigned)r >= (unsigned)rows) continue;   // never beyond the intermediate, whatever the table holds
        const uint32_t* p = reinterpret_cast<const uint32_t*>(plane + ((int64_t)r * g.out_w + ox0) * 3);
        const uint32_t w3[3] = {p[0], p[1], p[2]};
        const int32_t w = k[y];
#pragma unroll
        for (int e = 0; e < 3 * GTV_PER; ++e) s[e] += (int32_t)((w3[e / 4] >> (8 * (e % 4))) & 0xffu) * w;
      }
#pragma unroll
      for (int e = 0; e < 3 * GTV_PER; ++e) {
        const uint8_t u = clip8(s[e]);
        b[e] = u;
        f[e % 3][e / 3] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)u, 255.0f), 0.5f), 0.5f);
      }
    }
#pragma unroll
    for (int j = 0; j < GTV_PER; ++j) {
      if (words || j >= n) break;
      int iy, ix;
      image_yx(g, oy, ox0 + j, iy, ix);
      const int o = g.crop_y + iy;
      const int first = bounds[2 * o] - row0, cnt = bounds[2 * o + 1];
      const int32_t* k = kk + (int64_t)o * ksize;
      int32_t s[3] = {1 << 21, 1 << 21, 1 << 21};
      for (int y = 0; y < cnt; ++y) {
        const int r = first + y;
        if ((unsigned)r >= (unsigned)rows) continue;   // never beyond the intermediate, whatever the table holds
        const uint8_t* p = plane + ((int64_t)r * g.out_w + ix) * 3;
        const int32_t w = k[y];
        s[0] += (int32_t)p[0] * w;
        s[1] += (int32_t)p[1] * w;
        s[2] += (int32_t)p[2] * w;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const uint8_t u = clip8(s[c]);
        b[3 * j + c] = u;
        f[c][j] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)u, 255.0f), 0.5f), 0.5f);   // ToTensor, then Normalize(0.5, 0.5), in torchvision's order
      }
    }
    const int64_t at = (vr * OW) + ox0;   // (v OH + oy) OW + ox0
    store_rgb4(img_u8 + at * 3, b, n);
#pragma unroll
    for (int c = 0; c < 3; ++c) store_f4(img + (((int64_t)v * 3 + c) * OH + oy) * OW + ox0, f[c], n);
  }
}

__global__ __launch_bounds__(GTV_NT) void gtview_unproject_kernel(const int64_t* __restrict__ srcs, const float* __restrict__ cams, int n_views,
                                                                  GtvGeo g, const int32_t* __restrict__ nx, const int32_t* __restrict__ ny,
                                                                  int flags, float* __restrict__ depth_out, float* __restrict__ pts,
                                                                  uint8_t* __restrict__ valid, int32_t* __restrict__ flag) {
  const int OW = g.transpose ? g.out_h : g.out_w, OH = g.transpose ? g.out_w : g.out_h;
  const int quads = (OW + GTV_PER - 1) / GTV_PER;
  const int64_t total = (int64_t)n_views * OH * quads;
  const bool with_pose = flags & F3R_GTVIEW_POSE, finite_mask = flags & F3R_GTVIEW_FINITE_MASK;
  for (int64_t i = (int64_t)blockIdx.x * GTV_NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * GTV_NT) {
    const int q = (int)(i % quads);
    const int64_t vr = i / quads;
    const int oy = (int)(vr % OH), v = (int)(vr / OH);
    const int ox0 = q * GTV_PER, n = min(GTV_PER, OW - ox0);
    const float* src = reinterpret_cast<const float*>(srcs[2 * v]);
    const int64_t pitch = srcs[2 * v + 1];
    const float* cam = cams + (int64_t)v * GTV_CAM;
    // the table holds the intrinsics as the view returns them: rows [1, 0, 2] of K for a portrait group
    const float fu = g.transpose ? cam[3] : cam[0], cu = g.transpose ? cam[5] : cam[2];
    const float fv = g.transpose ? cam[1] : cam[4], cv = g.transpose ? cam[2] : cam[5];
    const float* T = cam + 9;
    float z[GTV_PER] = {}, p[GTV_PER][3] = {};
    uint8_t ok[GTV_PER] = {};
#pragma unroll
    for (int j = 0; j < GTV_PER; ++j) {
      if (j >= n) break;
      int iy, ix;
      image_yx(g, oy, ox0 + j, iy, ix);
      int sy = g.crop_y + iy, sx = g.crop_x + ix;
      if (ny) sy = ny[sy];
      if (nx) sx = nx[sx];
      sy = min(max(sy, 0), g.win_h - 1);   // never beyond the window, whatever the tables hold
      sx = min(max(sx, 0), g.win_w - 1);
      const float d = src[(int64_t)(g.win_y + sy) * pitch + g.win_x + sx];
      z[j] = d;
      if (flag && !isfinite(d)) *flag = 1;
      const double xd = ((double)ix - (double)cu) * (double)d / (double)fu;
      const double yd = ((double)iy - (double)cv) * (double)d / (double)fv;
      float X[3] = {(float)xd, (float)yd, d};
      if (with_pose) {
        const float x = X[0], y = X[1];
#pragma unroll
        for (int r = 0; r < 3; ++r) X[r] = ((T[4 * r] * x + T[4 * r + 1] * y) + T[4 * r + 2] * d) + T[4 * r + 3];
      }
      bool good = d > 0.0f;
      if (finite_mask) good = good && isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]);
      ok[j] = good ? 1 : 0;
#pragma unroll
      for (int r = 0; r < 3; ++r) p[j][r] = X[r];
    }
    const int64_t at = (vr * OW) + ox0;
    if (depth_out) store_f4(depth_out + at, z, n);
    if (pts) {
      float* o = pts + at * 3;
      if (n == GTV_PER && (reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
        float4v* o4 = reinterpret_cast<float4v*>(o);
        o4[0] = float4v{p[0][0], p[0][1], p[0][2], p[1][0]};
        o4[1] = float4v{p[1][1], p[1][2], p[2][0], p[2][1]};
        o4[2] = float4v{p[2][2], p[3][0], p[3][1], p[3][2]};
      } else {
#pragma unroll
        for (int j = 0; j < GTV_PER; ++j)
          if (j < n) {
            o[3 * j] = p[j][0];
            o[3 * j + 1] = p[j][1];
            o[3 * j + 2] = p[j][2];
          }
      }
    }
    if (valid) {
      uint8_t* o = valid + at;
      if (n == GTV_PER && (reinterpret_cast<uintptr_t>(o) & 3u) == 0) {
        *reinterpret_cast<uint32_t*>(o) = (uint32_t)ok[0] | (uint32_t)ok[1] << 8 | (uint32_t)ok[2] << 16 | (uint32_t)ok[3] << 24;
      } else {
#pragma unroll
        for (int j = 0; j < GTV_PER; ++j)
          if (j < n) o[j] = ok[j];
      }
    }
  }
}

inline unsigned gtv_grid(int64_t threads) { return (unsigned)std::min<int64_t>(blocks_of(threads, GTV_NT), GTV_MAX_GRID); }

inline bool gtv_box_ok(int x, int y, int w, int h) { return x >= 0 && y >= 0 && w >= 1 && h >= 1 && (int64_t)x + w <= (1 << 24) && (int64_t)y + h <= (1 << 24); }

}  // namespace

extern "C" size_t f3r_gtview_workspace_bytes(int n_views, int rows, int out_w) {
  if (n_views < 1 || rows < 1 || out_w < 1) return 0;
  return (size_t)((((int64_t)n_views * rows * out_w * 3) + 15) / 16 * 16);
}

extern "C" int f3r_gtview_resample(const int64_t* src_table, int n_views, int win_x, int win_y, int win_w, int win_h, const int32_t* bounds_h,
                                   const int32_t* kk_h, int ksize_h, int res_w, const int32_t* bounds_v, const int32_t* kk_v, int ksize_v,
                                   int res_h, int row0, int rows, int crop_x, int crop_y, int out_w, int out_h, int transpose, uint8_t* img_u8,
                                   float* img, void* workspace, size_t workspace_bytes, f3r_stream_t stream) {
  F3R_REQUIRE(src_table && bounds_h && kk_h && bounds_v && kk_v && img_u8 && img && workspace, "f3r_gtview_resample: null pointer");
  F3R_REQUIRE(n_views >= 1 && n_views <= (1 << 20), "f3r_gtview_resample: n_views = %d; need 1 <= n_views <= 2^20", n_views);
  F3R_REQUIRE(gtv_box_ok(win_x, win_y, win_w, win_h), "f3r_gtview_resample: window (%d, %d) + %d x %d is not a box of a frame", win_x, win_y, win_w, win_h);
  F3R_REQUIRE(res_w >= 1 && res_h >= 1 && res_w <= (1 << 24) && res_h <= (1 << 24) && ksize_h >= 1 && ksize_v >= 1,
              "f3r_gtview_resample: resized size %d x %d or table widths %d, %d out of range", res_w, res_h, ksize_h, ksize_v);
  F3R_REQUIRE(gtv_box_ok(crop_x, crop_y, out_w, out_h) && crop_x + out_w <= res_w && crop_y + out_h <= res_h,
              "f3r_gtview_resample: crop (%d, %d) + %d x %d leaves the resized %d x %d picture", crop_x, crop_y, out_w, out_h, res_w, res_h);
  F3R_REQUIRE(row0 >= 0 && rows >= 1 && (int64_t)row0 + rows <= win_h, "f3r_gtview_resample: rows [%d, %d + %d) leave the window's %d rows", row0,
              row0, rows, win_h);
  F3R_REQUIRE(transpose == 0 || transpose == 1, "f3r_gtview_resample: transpose = %d; need 0 or 1", transpose);
  F3R_REQUIRE((int64_t)n_views * out_w * out_h <= (1ll << 40) && (int64_t)n_views * rows * out_w <= (1ll << 40), "f3r_gtview_resample: group too large");
  F3R_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15u) == 0, "f3r_gtview_resample: workspace must be 16-byte aligned");
  const size_t need = f3r_gtview_workspace_bytes(n_views, rows, out_w);
  F3R_REQUIRE(workspace_bytes >= need, "f3r_gtview_resample: workspace of %zu bytes; need %zu (f3r_gtview_workspace_bytes)", workspace_bytes, need);
  const GtvGeo g{win_x, win_y, win_w, win_h, crop_x, crop_y, out_w, out_h, transpose};
  hipStream_t s = (hipStream_t)stream;
  uint8_t* tmp = (uint8_t*)workspace;
  const int64_t t1 = (int64_t)n_views * rows * ((out_w + GTV_PER - 1) / GTV_PER);
  const int OW = transpose ? out_h : out_w, OH = transpose ? out_w : out_h;
  const int64_t t2 = (int64_t)n_views * OH * ((OW + GTV_PER - 1) / GTV_PER);
  if (win_w <= GTV_HP_MAX_W) {
    const size_t lds = (size_t)(3 * win_w + 3 + 15) / 16 * 16;   // the row, shifted by up to three bytes
    const unsigned grid = (unsigned)std::min<int64_t>((int64_t)n_views * rows, 2 * GTV_MAX_GRID);
    hipLaunchKernelGGL(gtview_hpass_lds_kernel, dim3(grid), dim3(GTV_HP_NT), lds, s, src_table, n_views, g, bounds_h, kk_h, ksize_h, row0, rows, tmp);
  } else {
    hipLaunchKernelGGL(gtview_hpass_kernel, dim3(gtv_grid(t1)), dim3(GTV_NT), 0, s, src_table, n_views, g, bounds_h, kk_h, ksize_h, row0, rows, tmp);
  }
  hipLaunchKernelGGL(gtview_vpass_kernel, dim3(gtv_grid(t2)), dim3(GTV_NT), 0, s, (const uint8_t*)tmp, n_views, g, bounds_v, kk_v, ksize_v, row0, rows,
                     img_u8, img);
  return f3r_check_launch("f3r_gtview_resample");
}

extern "C" int f3r_gtview_unproject(const int64_t* src_table, const float* cams, int n_views, int win_x, int win_y, int win_w, int win_h,
                                    const int32_t* nx, const int32_t* ny, int res_w, int res_h, int crop_x, int crop_y, int out_w, int out_h,
                                    int transpose, int flags, float* depthmap, float* pts3d, uint8_t* valid_mask, int32_t* flag,
                                    f3r_stream_t stream) {
  F3R_REQUIRE(src_table && cams, "f3r_gtview_unproject: null src_table or cams");
  F3R_REQUIRE(depthmap || pts3d || valid_mask, "f3r_gtview_unproject: no output");
  F3R_REQUIRE(n_views >= 1 && n_views <= (1 << 20), "f3r_gtview_unproject: n_views = %d; need 1 <= n_views <= 2^20", n_views);
  F3R_REQUIRE(gtv_box_ok(win_x, win_y, win_w, win_h), "f3r_gtview_unproject: window (%d, %d) + %d x %d is not a box of a frame", win_x, win_y, win_w, win_h);
  F3R_REQUIRE((nx == nullptr) == (ny == nullptr), "f3r_gtview_unproject: nx and ny are given together");
  if (!nx) F3R_REQUIRE(res_w == win_w && res_h == win_h, "f3r_gtview_unproject: without nearest tables the resized size is the window's");
  F3R_REQUIRE(res_w >= 1 && res_h >= 1 && res_w <= (1 << 24) && res_h <= (1 << 24), "f3r_gtview_unproject: resized size %d x %d out of range", res_w, res_h);
  F3R_REQUIRE(gtv_box_ok(crop_x, crop_y, out_w, out_h) && crop_x + out_w <= res_w && crop_y + out_h <= res_h,
              "f3r_gtview_unproject: crop (%d, %d) + %d x %d leaves the resized %d x %d picture", crop_x, crop_y, out_w, out_h, res_w, res_h);
  F3R_REQUIRE(transpose == 0 || transpose == 1, "f3r_gtview_unproject: transpose = %d; need 0 or 1", transpose);
  F3R_REQUIRE((flags & ~(F3R_GTVIEW_POSE | F3R_GTVIEW_FINITE_MASK)) == 0, "f3r_gtview_unproject: unknown flags %d", flags);
  F3R_REQUIRE((int64_t)n_views * out_w * out_h <= (1ll << 40), "f3r_gtview_unproject: group too large");
  const GtvGeo g{win_x, win_y, win_w, win_h, crop_x, crop_y, out_w, out_h, transpose};
  const int OW = transpose ? out_h : out_w, OH = transpose ? out_w : out_h;
  const int64_t t = (int64_t)n_views * OH * ((OW + GTV_PER - 1) / GTV_PER);
  hipLaunchKernelGGL(gtview_unproject_kernel, dim3(gtv_grid(t)), dim3(GTV_NT), 0, (hipStream_t)stream, src_table, cams, n_views, g, nx, ny, flags,
                     depthmap, pts3d, valid_mask, flag);
  return f3r_check_launch("f3r_gtview_unproject");
}
