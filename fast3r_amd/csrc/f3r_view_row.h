// The per-view row of the mesh and point-cloud exports (f3r_mesh.hip, f3r_cloud.hip; include/f3r.h states the layout), and what both
// do with a pixel of it: the keep test, the colour, the stored point.  Header-only inline device functions.
#pragma once

#include "f3r_prims.h"

struct ViewRow {  // one row of the device table, 12 x 8 bytes
  const float* conf;    // (H W) fp32, or null: no threshold test
  const float* pts;     // (H W, 3) fp32
  const void* img;      // fp32 planes (3, H W) in [-1, 1], or with img_u8 the (H W, 3) bytes themselves
  const uint8_t* mask;  // (H W) bytes, nonzero = keep, or null
  int64_t H, W;
  int64_t vbase;        // sum of H W over the views before this one
  int64_t img_u8;
  int64_t k_lo, k_hi;   // f3r_mesh_threshold: the two 0-based ranks np.percentile reads
  int64_t gamma_bits;   // its fp32 interpolation weight, as bits
  int64_t reserved;
};
static_assert(sizeof(ViewRow) == 12 * 8, "include/f3r.h states the row layout");

// pixel i of a view of n pixels is kept: in range, conf > thr (with use_conf), mask nonzero (with a mask)
__device__ __forceinline__ bool view_keep(const ViewRow& r, bool use_conf, float thr, int64_t i, int64_t n) {
  bool v = i < n;
  if (v && use_conf) v = r.conf[i] > thr;
  if (v && r.mask) v = r.mask[i] != 0;
  return v;
}

// the pixel's colour, r | g << 8 | b << 16
__device__ __forceinline__ uint32_t pixel_rgb(const ViewRow& r, int64_t n, int64_t i) {
  uint32_t pk = 0;
  if (r.img_u8) {
    const uint8_t* g = (const uint8_t*)r.img + i * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) pk |= (uint32_t)g[ch] << (8 * ch);
  } else {
    const float* g = (const float*)r.img;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) pk |= (uint32_t)colour_u8(g[(int64_t)ch * n + i]) << (8 * ch);
  }
  return pk;
}

// out[o] = pixel i's point, as it is or with flip as (x, z, -y)
__device__ __forceinline__ void store_point(const ViewRow& r, int64_t i, int flip, float* out, int64_t o) {
  const float x = r.pts[i * 3 + 0], y = r.pts[i * 3 + 1], z = r.pts[i * 3 + 2];
  out[o * 3 + 0] = x;
  out[o * 3 + 1] = flip ? z : y;
  out[o * 3 + 2] = flip ? -y : z;
}
