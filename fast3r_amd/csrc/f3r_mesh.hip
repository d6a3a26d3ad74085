// Mesh export (ABI 410; include/f3r.h "mesh export"): the as_mesh=True branch of the reference's notebooks/demo_multiview.ipynb
// plot_3d_points_with_colors -- per view np.percentile(conf, p), conf > thr, the colour line, fast3r/dust3r/viz.py pts3d_to_trimesh
// (four fancy-indexed (H-1)(W-1) x 3 face arrays and a boolean gather) and cat_meshes -- for all views of a scene in one pass.
//
// * f3r_mesh_threshold: every view is a segment; one workgroup per view finds the two order statistics that np.percentile (method
//   "linear") reads by the exact radix select of f3r_post_common.h, counts the NaNs, and finishes with numpy's fp32 _lerp.
// * f3r_mesh_count: validity (conf > thr, AND the caller's mask) as a bitmap, one 64-bit word per wave step; kept A and B triangles per
//   tile of MESH_TILE quads; one exclusive scan over all tiles for A and one for B (a view's own offsets are differences of that scan);
//   with drop_unreferenced the "used" bitmap of the vertices (from the validity of each vertex's up to six triangles) and its scan.
// * f3r_mesh_write: the vertices (all, or the used ones in order, with the index remap), then the faces in the reference's order: per
//   view kept A, the same wound backward, kept B, the same wound backward; every slot comes from the scan and a ballot rank.
// * f3r_mesh_ply_pack: 12-byte vertex and 16-byte face records.
// A tile never straddles a view.  No atomics except the NaN counter of a workgroup in LDS: two runs give the same bits.  Built with
// -ffp-contract=off: the interpolation and the colour arithmetic round each fp32 operation on its own, as numpy does.
#include "f3r_common.h"
#include "f3r_post_common.h"
#include "f3r_view_row.h"  // the rows of the device table, 12 x 8 bytes: ViewRow

#include <algorithm>

namespace {

constexpr int MESH_TILE = 1024;                // pixels, or quads, of one workgroup (one wave, 16 steps of 64)
constexpr int MESH_STEPS = MESH_TILE / 64;     // = bitmap words per vertex tile
constexpr int THR_NT = 1024;                   // threads of a threshold workgroup
static_assert(MESH_TILE == F3R_MESH_TILE, "include/f3r.h states the tile length");

// ---------------------------------------------------------------------------------------------------------------------------
// thr[v] = np.percentile(conf of view v, p): numpy's _lerp on the order statistics k_lo, k_hi with weight gamma; NaN if any conf is NaN
__global__ __launch_bounds__(THR_NT) void mesh_threshold_kernel(const ViewRow* __restrict__ rows, float* __restrict__ thr,
                                                                uint32_t* __restrict__ nan_count) {
  __shared__ uint32_t hist[2048];
  __shared__ int64_t sh_i64[2];
  __shared__ uint32_t sh_nan;
  const ViewRow r = rows[blockIdx.x];
  const int64_t n = r.H * r.W;
  if (threadIdx.x == 0) sh_nan = 0;
  __syncthreads();
  uint32_t c = 0;
  if (r.conf)
    for (int64_t i = threadIdx.x; i < n; i += THR_NT) c += r.conf[i] != r.conf[i] ? 1u : 0u;
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&sh_nan, c);
  __syncthreads();
  const uint32_t nn = sh_nan;
  float t = __builtin_bit_cast(float, 0x7fc00000u);
  if (r.conf && nn == 0) {  // uniform over the workgroup: select_kth synchronises
    const float vlo = fkey_inv(select_kth<THR_NT>(r.conf, n, r.k_lo, hist, sh_i64));
    float vhi = vlo;
    if (r.k_hi != r.k_lo) vhi = fkey_inv(select_kth<THR_NT>(r.conf, n, r.k_hi, hist, sh_i64));
    const float g = __builtin_bit_cast(float, (uint32_t)r.gamma_bits);
    const float d = vhi - vlo;
    t = vlo + d * g;
    if (g >= 0.5f) t = vhi - d * (1.0f - g);
  }
  if (threadIdx.x == 0) {
    thr[blockIdx.x] = t;
    nan_count[blockIdx.x] = nn;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// validity bitmap: view v's words start at 16 tsv[v]; pixel i = bit i % 64 of word i / 64; bits beyond H W are zero
__global__ __launch_bounds__(64) void mesh_valid_kernel(const ViewRow* __restrict__ rows, const int64_t* __restrict__ tsv, int S,
                                                        const float* __restrict__ thr, uint64_t* __restrict__ bits) {
  const int seg = last_le(tsv, 0, S, blockIdx.x);
  const ViewRow r = rows[seg];
  const int64_t n = r.H * r.W, base = (blockIdx.x - tsv[seg]) * MESH_TILE;
  const bool use_conf = thr && r.conf;
  const float t = use_conf ? thr[seg] : 0.f;
  for (int s = 0; s < MESH_STEPS; ++s) {
    const uint64_t b = __ballot(view_keep(r, use_conf, t, base + s * 64 + threadIdx.x, n));
    if (threadIdx.x == 0) bits[(int64_t)blockIdx.x * MESH_STEPS + s] = b;
  }
}

__device__ __forceinline__ bool vbit(const uint64_t* __restrict__ vb, uint32_t i) { return (vb[i >> 6] >> (i & 63)) & 1ull; }

// quad q of a view of width W: i = its top-left pixel; bit 0 = triangle A (i, i+1, i+W) is kept, bit 1 = triangle B (i+1, i+W, i+W+1)
__device__ __forceinline__ uint32_t quad_keep(const uint64_t* __restrict__ vb, uint32_t q, uint32_t W, uint32_t& i) {
  const uint32_t y = q / (W - 1), x = q - y * (W - 1);
  i = y * W + x;
  const bool v23 = vbit(vb, i + 1) && vbit(vb, i + W);
  return (v23 && vbit(vb, i) ? 1u : 0u) | (v23 && vbit(vb, i + W + 1) ? 2u : 0u);
}

__device__ __forceinline__ int64_t quads_of(const ViewRow& r) { return (r.H - 1) * (r.W - 1); }

// cnt[0][tile] = kept A, cnt[1][tile] = kept B (rows of n_tiles + 1 words; the last word of each row is zeroed for the scan's total)
__global__ __launch_bounds__(64) void mesh_count_kernel(const ViewRow* __restrict__ rows, const int64_t* __restrict__ tsv,
                                                        const int64_t* __restrict__ tsq, int S, const uint64_t* __restrict__ bits,
                                                        uint32_t* __restrict__ cnt, int64_t n_tiles) {
  const int seg = last_le(tsq, 0, S, blockIdx.x);
  const ViewRow r = rows[seg];
  const uint64_t* vb = bits + tsv[seg] * MESH_STEPS;
  uint32_t c[2];
  tile_count<MESH_TILE>(
      (blockIdx.x - tsq[seg]) * MESH_TILE, quads_of(r),
      [&](int64_t q) {
        uint32_t i;
        return quad_keep(vb, (uint32_t)q, (uint32_t)r.W, i);
      },
      c);
  if (threadIdx.x == 0) {
    cnt[blockIdx.x] = c[0];
    cnt[n_tiles + 1 + blockIdx.x] = c[1];
    if (blockIdx.x == 0) cnt[n_tiles] = cnt[2 * n_tiles + 1] = 0;
  }
}

// is pixel (y, x) a vertex of a kept triangle: P and one of the six neighbour pairs that close a triangle with it
__device__ __forceinline__ bool vertex_used(const uint64_t* __restrict__ vb, uint32_t i, uint32_t H, uint32_t W) {
  if (!vbit(vb, i)) return false;
  const uint32_t y = i / W, x = i - y * W;
  const bool up = y > 0, dn = y + 1 < H, lf = x > 0, rt = x + 1 < W;
  const bool U = up && vbit(vb, i - W), D = dn && vbit(vb, i + W), L = lf && vbit(vb, i - 1), R = rt && vbit(vb, i + 1);
  const bool UR = up && rt && vbit(vb, i - W + 1), DL = dn && lf && vbit(vb, i + W - 1);
  return (R && D) || (L && DL) || (DL && D) || (U && UR) || (UR && R) || (U && L);
}

// ubits: the "used" bitmap, laid out like the validity bitmap; cntv[tile] = used vertices of the tile (n_tiles + 1 words, last zeroed)
__global__ __launch_bounds__(64) void mesh_used_kernel(const ViewRow* __restrict__ rows, const int64_t* __restrict__ tsv, int S,
                                                       const uint64_t* __restrict__ bits, uint64_t* __restrict__ ubits,
                                                       uint32_t* __restrict__ cntv, int64_t n_tiles) {
  const int seg = last_le(tsv, 0, S, blockIdx.x);
  const ViewRow r = rows[seg];
  const uint64_t* vb = bits + tsv[seg] * MESH_STEPS;
  const int64_t n = r.H * r.W, base = (blockIdx.x - tsv[seg]) * MESH_TILE;
  uint32_t c = 0;
  for (int s = 0; s < MESH_STEPS; ++s) {
    const int64_t i = base + s * 64 + threadIdx.x;
    const bool u = i < n && vertex_used(vb, (uint32_t)i, (uint32_t)r.H, (uint32_t)r.W);
    const uint64_t b = __ballot(u);
    if (threadIdx.x == 0) ubits[(int64_t)blockIdx.x * MESH_STEPS + s] = b;
    c += (uint32_t)__popcll(b);
  }
  if (threadIdx.x == 0) {
    cntv[blockIdx.x] = c;
    if (blockIdx.x == 0) cntv[n_tiles] = 0;
  }
}

// counts[v] = { kept A, kept B, used vertices (H W without the used scan) } of view v, from the scans
__global__ void mesh_totals_kernel(const ViewRow* __restrict__ rows, const int64_t* __restrict__ tsv, const int64_t* __restrict__ tsq, int S,
                                   const uint32_t* __restrict__ scanf, int64_t n_quad_tiles, const uint32_t* __restrict__ scanv,
                                   uint32_t* __restrict__ counts) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= S) return;
  const uint32_t* sb = scanf + n_quad_tiles + 1;
  counts[v * 3 + 0] = scanf[tsq[v + 1]] - scanf[tsq[v]];
  counts[v * 3 + 1] = sb[tsq[v + 1]] - sb[tsq[v]];
  counts[v * 3 + 2] = scanv ? scanv[tsv[v + 1]] - scanv[tsv[v]] : (uint32_t)(rows[v].H * rows[v].W);
}

// ---------------------------------------------------------------------------------------------------------------------------
// vertices: every pixel at vbase + i, or with DROP the used ones at their rank (and remap[vbase + i] = that rank, -1 if unused)
template <bool DROP>
__global__ __launch_bounds__(64) void mesh_vertex_kernel(const ViewRow* __restrict__ rows, const int64_t* __restrict__ tsv, int S,
                                                         const uint64_t* __restrict__ ubits, const uint32_t* __restrict__ scanv, int flip,
                                                         float* __restrict__ out, int32_t* __restrict__ remap) {
  const int seg = last_le(tsv, 0, S, blockIdx.x);
  const ViewRow r = rows[seg];
  const int64_t n = r.H * r.W, base = (blockIdx.x - tsv[seg]) * MESH_TILE;
  int64_t run = DROP ? (int64_t)scanv[blockIdx.x] : 0;
  for (int s = 0; s < MESH_STEPS; ++s) {
    const int64_t i = base + s * 64 + threadIdx.x;
    const bool ok = i < n;
    bool keep = ok;
    int64_t o = r.vbase + i;
    if (DROP) {
      const uint64_t w = ubits[(int64_t)blockIdx.x * MESH_STEPS + s];
      keep = (w >> threadIdx.x) & 1ull;
      o = run + __popcll(w & lanes_below());
      run += __popcll(w);
      if (ok) remap[r.vbase + i] = keep ? (int32_t)o : -1;
    }
    if (keep) store_point(r, i, flip, out, o);
  }
}

template <class IDX>
__device__ __forceinline__ void put_face(IDX* __restrict__ faces, uint8_t* __restrict__ col, int64_t p, int64_t i0, int64_t i1, int64_t i2,
                                         uint32_t rgb) {
  faces[p * 3 + 0] = (IDX)i0;
  faces[p * 3 + 1] = (IDX)i1;
  faces[p * 3 + 2] = (IDX)i2;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) col[p * 3 + ch] = (uint8_t)(rgb >> (8 * ch));
}

// faces of view v from slot mult (A before + B before): [kept A][A backward][kept B][B backward] (mult = 2), or [kept A][kept B] (mult = 1)
template <class IDX, bool REMAP>
__global__ __launch_bounds__(64) void mesh_face_kernel(const ViewRow* __restrict__ rows, const int64_t* __restrict__ tsv,
                                                       const int64_t* __restrict__ tsq, int S, const uint64_t* __restrict__ bits,
                                                       const uint32_t* __restrict__ scanf, int64_t n_tiles, int mult,
                                                       const int32_t* __restrict__ remap, IDX* __restrict__ faces, uint8_t* __restrict__ col) {
  const int seg = last_le(tsq, 0, S, blockIdx.x);
  const ViewRow r = rows[seg];
  const uint64_t* vb = bits + tsv[seg] * MESH_STEPS;
  const int64_t n = r.H * r.W;
  const uint32_t* sa = scanf;
  const uint32_t* sb = scanf + n_tiles + 1;
  const int64_t t0 = tsq[seg], t1 = tsq[seg + 1];
  const int64_t a0 = sa[t0], b0 = sb[t0], av = (int64_t)sa[t1] - a0, bv = (int64_t)sb[t1] - b0;
  const int64_t fa = (int64_t)mult * (a0 + b0), fb = fa + (int64_t)mult * av;
  int64_t run[2] = {fa + sa[blockIdx.x] - a0, fb + sb[blockIdx.x] - b0};
  uint32_t i = 0;  // the quad's top-left pixel: flags leaves it for emit
  tile_compact<MESH_TILE>(
      (blockIdx.x - tsq[seg]) * MESH_TILE, quads_of(r), run, [&](int64_t q) { return quad_keep(vb, (uint32_t)q, (uint32_t)r.W, i); },
      [&](int64_t, uint32_t ab, const int64_t(&p)[2]) {
        const bool a = ab & 1u, b = ab & 2u;
        int64_t g1 = r.vbase + i, g2 = g1 + 1, g3 = g1 + r.W, g4 = g3 + 1;
        if (REMAP) {  // a kept triangle's vertices are used: their remap entries are >= 0
          g2 = remap[g2];
          g3 = remap[g3];
          if (a) g1 = remap[g1];
          if (b) g4 = remap[g4];
        }
        if (a) {
          const uint32_t rgb = pixel_rgb(r, n, i);  // the quad's top-left pixel
          put_face(faces, col, p[0], g1, g2, g3, rgb);
          if (mult == 2) put_face(faces, col, p[0] + av, g3, g2, g1, rgb);
        }
        if (b) {
          const uint32_t rgb = pixel_rgb(r, n, (int64_t)i + r.W + 1);  // its bottom-right pixel
          put_face(faces, col, p[1], g2, g3, g4, rgb);
          if (mult == 2) put_face(faces, col, p[1] + bv, g4, g3, g2, rgb);
        }
      });
}

// ---------------------------------------------------------------------------------------------------------------------------
// PLY records: 3 nv words of xyz, then per face 16 bytes { 3, three little-endian int32, r, g, b }; thread = one vertex word or one face
template <class IDX>
__global__ void mesh_ply_pack_kernel(const uint32_t* __restrict__ vert, int64_t nv, const IDX* __restrict__ faces,
                                     const uint8_t* __restrict__ col, int64_t nf, uint32_t* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < nv * 3) {
    out[t] = vert[t];
    return;
  }
  const int64_t f = t - nv * 3;
  if (f >= nf) return;
  const uint32_t i0 = (uint32_t)faces[f * 3 + 0], i1 = (uint32_t)faces[f * 3 + 1], i2 = (uint32_t)faces[f * 3 + 2];
  uint32_t* o = out + nv * 3 + f * 4;
  o[0] = 3u | (i0 << 8);
  o[1] = (i0 >> 24) | (i1 << 8);
  o[2] = (i1 >> 24) | (i2 << 8);
  o[3] = (i2 >> 24) | ((uint32_t)col[f * 3 + 0] << 8) | ((uint32_t)col[f * 3 + 1] << 16) | ((uint32_t)col[f * 3 + 2] << 24);
}

// ---- host
struct MeshWs {
  uint64_t *bits, *ubits;
  uint32_t *scanf, *scanv;
  int32_t* remap;
  size_t bytes;
};

MeshWs mesh_ws(void* base, int64_t nvt, int64_t nqt, int64_t total_vertices, int drop) {
  Carve c(base, 256);
  MeshWs m = {};
  m.bits = c.take<uint64_t>((size_t)nvt * MESH_STEPS);
  m.scanf = c.take<uint32_t>((size_t)(nqt + 1) * 2);
  if (drop) {
    m.ubits = c.take<uint64_t>((size_t)nvt * MESH_STEPS);
    m.scanv = c.take<uint32_t>(nvt + 1);
    m.remap = c.take<int32_t>(total_vertices);
  }
  m.bytes = c.bytes();
  return m;
}

// the shapes on the host against the totals the device table was built with; nothing is launched unless they agree
int mesh_check(const char* what, const int64_t* table, const int64_t* host_hw, int n_views, int64_t nvt, int64_t nqt, int64_t total_vertices) {
  F3R_REQUIRE(table && host_hw, "%s: null table or host_hw", what);
  F3R_REQUIRE(n_views >= 1, "%s: n_views = %d; need at least one view", what, n_views);
  F3R_REQUIRE(nvt >= 0 && nqt >= 0 && total_vertices >= 0, "%s: negative count (%lld vertex tiles, %lld quad tiles, %lld vertices)", what,
              (long long)nvt, (long long)nqt, (long long)total_vertices);
  int64_t tv = 0, sv = 0, sq = 0;
  for (int v = 0; v < n_views; ++v) {
    const int64_t H = host_hw[2 * v], W = host_hw[2 * v + 1];
    F3R_REQUIRE(H >= 1 && W >= 1 && H < (1ll << 31) && W < (1ll << 31), "%s: view %d is %lld x %lld; need H, W >= 1", what, v, (long long)H,
                (long long)W);
    tv += H * W;
    F3R_REQUIRE(tv < (1ll << 31), "%s: %lld vertices or more up to view %d; the indices are 32-bit: need fewer than 2^31 in all", what,
                (long long)tv, v);
    sv += (H * W + MESH_TILE - 1) / MESH_TILE;
    sq += std::max<int64_t>(1, ((H - 1) * (W - 1) + MESH_TILE - 1) / MESH_TILE);
  }
  F3R_REQUIRE(tv == total_vertices && sv == nvt && sq == nqt,
              "%s: host_hw gives %lld vertices, %lld vertex tiles, %lld quad tiles; the call states %lld, %lld, %lld", what, (long long)tv,
              (long long)sv, (long long)sq, (long long)total_vertices, (long long)nvt, (long long)nqt);
  return F3R_OK;
}

}  // namespace

extern "C" size_t f3r_mesh_workspace_bytes(int64_t n_vertex_tiles, int64_t n_quad_tiles, int64_t total_vertices, int drop_unreferenced) {
  if (n_vertex_tiles < 1 || n_quad_tiles < 1 || total_vertices < 1 || total_vertices >= (1ll << 31)) return 0;
  return mesh_ws(nullptr, n_vertex_tiles, n_quad_tiles, total_vertices, drop_unreferenced).bytes;
}

extern "C" int f3r_mesh_threshold(const int64_t* table, int n_views, float* thresholds, uint32_t* nan_counts, f3r_stream_t stream) {
  F3R_REQUIRE(table && thresholds && nan_counts, "f3r_mesh_threshold: null pointer");
  F3R_REQUIRE(n_views >= 1, "f3r_mesh_threshold: n_views = %d; need at least one view", n_views);
  hipLaunchKernelGGL(mesh_threshold_kernel, dim3(n_views), dim3(THR_NT), 0, (hipStream_t)stream, (const ViewRow*)table, thresholds, nan_counts);
  return f3r_check_launch("f3r_mesh_threshold");
}

extern "C" int f3r_mesh_count(const int64_t* table, const int64_t* host_hw, int n_views, int64_t n_vertex_tiles, int64_t n_quad_tiles,
                              int64_t total_vertices, const float* thresholds, int drop_unreferenced, void* workspace, size_t workspace_bytes,
                              uint32_t* counts, f3r_stream_t stream) {
  if (int e = mesh_check("f3r_mesh_count", table, host_hw, n_views, n_vertex_tiles, n_quad_tiles, total_vertices)) return e;
  F3R_REQUIRE(workspace && counts, "f3r_mesh_count: null workspace or counts");
  const MeshWs m = mesh_ws(workspace, n_vertex_tiles, n_quad_tiles, total_vertices, drop_unreferenced);
  F3R_REQUIRE(workspace_bytes >= m.bytes, "f3r_mesh_count: workspace too small (%zu bytes; need %zu)", workspace_bytes, m.bytes);
  hipStream_t s = (hipStream_t)stream;
  const ViewRow* rows = (const ViewRow*)table;
  const int64_t* tsv = table + (int64_t)n_views * 12;
  const int64_t* tsq = tsv + n_views + 1;
  const dim3 gv((unsigned)n_vertex_tiles), gq((unsigned)n_quad_tiles), b(64);
  hipLaunchKernelGGL(mesh_valid_kernel, gv, b, 0, s, rows, tsv, n_views, thresholds, m.bits);
  hipLaunchKernelGGL(mesh_count_kernel, gq, b, 0, s, rows, tsv, tsq, n_views, m.bits, m.scanf, n_quad_tiles);
  hipLaunchKernelGGL(exclusive_scan_rows_kernel<SCAN_NT>, dim3(2), dim3(SCAN_NT), 0, s, m.scanf, (const int64_t*)nullptr, n_quad_tiles + 1,
                     (uint32_t*)nullptr);
  if (drop_unreferenced) {
    hipLaunchKernelGGL(mesh_used_kernel, gv, b, 0, s, rows, tsv, n_views, m.bits, m.ubits, m.scanv, n_vertex_tiles);
    hipLaunchKernelGGL(exclusive_scan_rows_kernel<SCAN_NT>, dim3(1), dim3(SCAN_NT), 0, s, m.scanv, (const int64_t*)nullptr, n_vertex_tiles + 1,
                       (uint32_t*)nullptr);
  }
  hipLaunchKernelGGL(mesh_totals_kernel, dim3(blocks_of(n_views, 256)), dim3(256), 0, s, rows, tsv, tsq, n_views, m.scanf, n_quad_tiles,
                     drop_unreferenced ? m.scanv : (const uint32_t*)nullptr, counts);
  return f3r_check_launch("f3r_mesh_count");
}

extern "C" int f3r_mesh_write(const int64_t* table, const int64_t* host_hw, int n_views, int64_t n_vertex_tiles, int64_t n_quad_tiles,
                              int64_t total_vertices, int double_sided, int drop_unreferenced, int flip_axes, int index_dtype,
                              const void* workspace, size_t workspace_bytes, float* vertices, void* faces, uint8_t* face_colors,
                              f3r_stream_t stream) {
  if (int e = mesh_check("f3r_mesh_write", table, host_hw, n_views, n_vertex_tiles, n_quad_tiles, total_vertices)) return e;
  F3R_REQUIRE(index_dtype == F3R_INDEX_I32 || index_dtype == F3R_INDEX_I64, "f3r_mesh_write: index_dtype %d is neither F3R_INDEX_I32 nor F3R_INDEX_I64",
              index_dtype);
  F3R_REQUIRE(workspace, "f3r_mesh_write: null workspace");
  const MeshWs m = mesh_ws((void*)workspace, n_vertex_tiles, n_quad_tiles, total_vertices, drop_unreferenced);
  F3R_REQUIRE(workspace_bytes >= m.bytes, "f3r_mesh_write: workspace too small (%zu bytes; need %zu)", workspace_bytes, m.bytes);
  hipStream_t s = (hipStream_t)stream;
  const ViewRow* rows = (const ViewRow*)table;
  const int64_t* tsv = table + (int64_t)n_views * 12;
  const int64_t* tsq = tsv + n_views + 1;
  const dim3 gv((unsigned)n_vertex_tiles), gq((unsigned)n_quad_tiles), b(64);
  const int mult = double_sided ? 2 : 1, flip = flip_axes ? 1 : 0;
  // vertices may be null when drop_unreferenced kept none, faces when the count found none; the remap is written with the vertices
  F3R_REQUIRE(vertices || !(drop_unreferenced && faces), "f3r_mesh_write: drop_unreferenced with faces needs vertices (the remap is written with them)");
  F3R_REQUIRE(face_colors || !faces, "f3r_mesh_write: faces without face_colors");
  if (vertices) {
    if (drop_unreferenced)
      hipLaunchKernelGGL(mesh_vertex_kernel<true>, gv, b, 0, s, rows, tsv, n_views, m.ubits, m.scanv, flip, vertices, m.remap);
    else
      hipLaunchKernelGGL(mesh_vertex_kernel<false>, gv, b, 0, s, rows, tsv, n_views, m.ubits, m.scanv, flip, vertices, m.remap);
  }
  if (faces) {
#define F3R_MESH_FACES(IDX, REMAP)                                                                                                        \
  hipLaunchKernelGGL((mesh_face_kernel<IDX, REMAP>), gq, b, 0, s, rows, tsv, tsq, n_views, m.bits, m.scanf, n_quad_tiles, mult, m.remap, \
                     (IDX*)faces, face_colors)
    if (index_dtype == F3R_INDEX_I32) {
      if (drop_unreferenced) F3R_MESH_FACES(int32_t, true); else F3R_MESH_FACES(int32_t, false);
    } else {
      if (drop_unreferenced) F3R_MESH_FACES(int64_t, true); else F3R_MESH_FACES(int64_t, false);
    }
#undef F3R_MESH_FACES
  }
  return f3r_check_launch("f3r_mesh_write");
}

extern "C" int f3r_mesh_ply_pack(const float* vertices, int64_t n_vertices, const void* faces, const uint8_t* face_colors, int64_t n_faces,
                                 int index_dtype, void* out, f3r_stream_t stream) {
  F3R_REQUIRE(n_vertices >= 0 && n_faces >= 0, "f3r_mesh_ply_pack: negative count (%lld vertices, %lld faces)", (long long)n_vertices,
              (long long)n_faces);
  F3R_REQUIRE(n_vertices < (1ll << 31), "f3r_mesh_ply_pack: %lld vertices; the file's indices are 32-bit: need fewer than 2^31",
              (long long)n_vertices);
  F3R_REQUIRE(index_dtype == F3R_INDEX_I32 || index_dtype == F3R_INDEX_I64, "f3r_mesh_ply_pack: index_dtype %d is neither F3R_INDEX_I32 nor F3R_INDEX_I64",
              index_dtype);
  if (n_vertices == 0 && n_faces == 0) return F3R_OK;
  F3R_REQUIRE(out && (vertices || n_vertices == 0) && ((faces && face_colors) || n_faces == 0), "f3r_mesh_ply_pack: null pointer");
  F3R_REQUIRE(((uintptr_t)out & 3) == 0, "f3r_mesh_ply_pack: out must be 4-byte aligned (it holds 12 n_vertices + 16 n_faces bytes)");
  const int64_t threads = n_vertices * 3 + n_faces;
  F3R_REQUIRE(threads < (1ll << 39), "f3r_mesh_ply_pack: too many records");
  const dim3 g(blocks_of(threads, 256)), b(256);
  if (index_dtype == F3R_INDEX_I32)
    hipLaunchKernelGGL(mesh_ply_pack_kernel<int32_t>, g, b, 0, (hipStream_t)stream, (const uint32_t*)vertices, n_vertices, (const int32_t*)faces,
                       face_colors, n_faces, (uint32_t*)out);
  else
    hipLaunchKernelGGL(mesh_ply_pack_kernel<int64_t>, g, b, 0, (hipStream_t)stream, (const uint32_t*)vertices, n_vertices, (const int64_t*)faces,
                       face_colors, n_faces, (uint32_t*)out);
  return f3r_check_launch("f3r_mesh_ply_pack");
}
