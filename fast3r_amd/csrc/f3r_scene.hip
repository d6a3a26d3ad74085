// Scene assembly and PLY export (ABI 390; include/f3r.h "scene assembly"): what the reference's viser visualizer does per view and per
// head on the host with numpy -- np.argsort(-conf) and four gathers by that order, three colourings, the per-view extrema, the
// 20th / 80th percentile scene extent, the prefix cut with the sky mask, and generate_ply_bytes -- as integer and byte kernels.
//
// * f3r_scene_sort: every (view, head) is a segment; a segmented stable LSD radix sort (4 passes of 8 bits) of (key, pixel index)
//   pairs.  The key is an order-preserving integer of -conf with the two zeros and every NaN payload made one value each, so the
//   order equals np.argsort(-conf, kind='stable').  A tile of SCENE_TILE keys never straddles a segment.  Per pass: digit counts per
//   (segment, tile); one scan workgroup per segment; then a scatter that first orders the tile by digit in LDS (ballot ranking keeps
//   equal digits in pixel order), so that neighbouring lanes write neighbouring addresses.  The first pass builds the keys from the
//   confidences as it reads them and collects the segment's extrema, NaN count and mask count; the first pass also packs, per pixel, a 16-byte record (xyz, image colour as three bytes, mask
//   byte) while its reads are still streaming; the last pass writes no keys: it writes the order and every gathered output at once from
//   ONE 16-byte gather per key (plus the confidence, which the key itself gives back) and the turbo colour from a table in LDS.
// * f3r_scene_extent: the bracketing order statistics of np.percentile per axis, by exact radix select (11 + 11 + 10 bits).
// * f3r_scene_collect_count / _write: the prefix cut and the stable sky-mask compaction into one packed (points, colours) pair.
// * f3r_ply_pack, f3r_color_range, f3r_color_to_u8: generate_ply_bytes / safe_color_conversion.
// Only integer atomics are used: two runs give the same bits.  Built with -ffp-contract=off: each fp32 operation of the colour
// arithmetic is rounded on its own, as numpy rounds it.
#include "f3r_common.h"
#include "f3r_post_common.h"

#include <algorithm>

namespace {

constexpr int SCENE_NT = 256;                 // threads of a sort workgroup (4 waves)
constexpr int SCENE_PER = 16;                 // keys per thread
constexpr int SCENE_TILE = SCENE_NT * SCENE_PER;  // 4096 = F3R_SCENE_TILE
constexpr int SCENE_SUB = 64 * SCENE_PER;     // keys of one wave: a contiguous quarter of the tile
static_assert(SCENE_TILE == F3R_SCENE_TILE, "include/f3r.h states the tile length");

struct SegRow {  // one row of the device table, 6 x 8 bytes
  const float* conf;
  const float* pts;
  const float* img;
  const int8_t* mask;
  int64_t len;
  int64_t off;
};

struct SceneOut {
  int32_t* order;
  float* pts;
  float* conf;
  uint8_t* rgb;
  uint8_t* ccol;
  int8_t* mask;
};

// ascending in this key = descending in conf; -0.0 == +0.0; every NaN is the one largest key (np.argsort puts NaN last)
__device__ __forceinline__ uint32_t conf_key(float c) {
  if (c != c) return 0xffffffffu;
  if (c == 0.f) c = 0.f;
  return ~fkey(c);
}
__device__ __forceinline__ float conf_of_key(uint32_t k) { return fkey_inv(~k); }

// stats[seg * 4 + {0: smallest key = largest conf, 1: largest non-NaN key = smallest conf, 2: NaN count, 3: count of mask > 0}]
__global__ void scene_stats_init_kernel(uint32_t* __restrict__ stats, int S) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < S * 4) stats[i] = (i & 3) == 0 ? 0xffffffffu : 0u;
}

template <bool FIRST>
__global__ __launch_bounds__(SCENE_NT) void scene_hist_kernel(const SegRow* __restrict__ rows, const int64_t* __restrict__ ts, int S,
                                                              const uint32_t* __restrict__ keys, int shift, uint32_t* __restrict__ hist,
                                                              uint32_t* __restrict__ stats, u32x4* __restrict__ recs) {
  __shared__ uint32_t cnt[256];
  __shared__ uint32_t red[4];
  const int seg = last_le(ts, 0, S, blockIdx.x);  // the segment that owns this tile (every segment has at least one)
  const SegRow r = rows[seg];
  const int64_t t = blockIdx.x - ts[seg], nt = ts[seg + 1] - ts[seg];
  const int64_t base = t * SCENE_TILE, end = min(base + (int64_t)SCENE_TILE, r.len);
  cnt[threadIdx.x] = 0;
  if (FIRST && threadIdx.x < 4) red[threadIdx.x] = threadIdx.x == 0 ? 0xffffffffu : 0u;
  __syncthreads();
  uint32_t kmin = 0xffffffffu, kmax = 0u, nnan = 0u, nmask = 0u;
  for (int64_t i = base + threadIdx.x; i < end; i += SCENE_NT) {
    uint32_t k;
    if (FIRST) {
      k = conf_key(r.conf[i]);
      if (k == 0xffffffffu) {
        ++nnan;
      } else {
        kmin = min(kmin, k);
        kmax = max(kmax, k);
      }
      const int8_t mk = r.mask ? r.mask[i] : (int8_t)1;
      nmask += mk > 0 ? 1u : 0u;
      // the pixel's record for the last pass's single 16-byte gather: xyz and r | g << 8 | b << 16 | mask << 24
      const float* p3 = r.pts + i * 3;
      u32x4 rec;
      rec[0] = __builtin_bit_cast(uint32_t, p3[0]);
      rec[1] = __builtin_bit_cast(uint32_t, p3[1]);
      rec[2] = __builtin_bit_cast(uint32_t, p3[2]);
      uint32_t pk = (uint32_t)(uint8_t)mk << 24;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) pk |= (uint32_t)colour_u8(r.img[(int64_t)ch * r.len + i]) << (8 * ch);
      rec[3] = pk;
      recs[r.off + i] = rec;
    } else {
      k = keys[r.off + i];
    }
    atomicAdd(&cnt[(k >> shift) & 255u], 1u);
  }
  if (FIRST) {
    atomicMin(&red[0], kmin);
    atomicMax(&red[1], kmax);
    if (nnan) atomicAdd(&red[2], nnan);
    if (nmask) atomicAdd(&red[3], nmask);
  }
  __syncthreads();
  hist[ts[seg] * 256 + (int64_t)threadIdx.x * nt + t] = cnt[threadIdx.x];  // digit-major within the segment: its scan gives slot bases
  if (FIRST && threadIdx.x == 0) {
    atomicMin(&stats[seg * 4 + 0], red[0]);
    atomicMax(&stats[seg * 4 + 1], red[1]);
    if (red[2]) atomicAdd(&stats[seg * 4 + 2], red[2]);
    if (red[3]) atomicAdd(&stats[seg * 4 + 3], red[3]);
  }
}

template <bool FIRST, bool FINAL>
__global__ __launch_bounds__(SCENE_NT) void scene_scatter_kernel(const SegRow* __restrict__ rows, const int64_t* __restrict__ ts, int S,
                                                                 const uint32_t* __restrict__ kin, const uint32_t* __restrict__ vin, int shift,
                                                                 const uint32_t* __restrict__ hist, uint32_t* __restrict__ kout,
                                                                 uint32_t* __restrict__ vout, SceneOut o, const uint32_t* __restrict__ stats,
                                                                 const uint8_t* __restrict__ lut, const u32x4* __restrict__ recs) {
  __shared__ uint32_t sk[SCENE_TILE], sv[SCENE_TILE];
  __shared__ uint32_t cnt[4][256];
  __shared__ uint32_t lbase[256], gbase[256], wsum[4];
  __shared__ uint8_t slut[FINAL ? 768 : 4];
  const int seg = last_le(ts, 0, S, blockIdx.x);  // the segment that owns this tile (every segment has at least one)
  const SegRow r = rows[seg];
  const int64_t t = blockIdx.x - ts[seg], nt = ts[seg + 1] - ts[seg];
  const int64_t base = t * SCENE_TILE, end = min(base + (int64_t)SCENE_TILE, r.len);
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  for (int j = 0; j < 4; ++j) cnt[j][tid] = 0;
  if (FINAL)
    for (int j = tid; j < 768; j += SCENE_NT) slut[j] = lut[j];
  gbase[tid] = hist[ts[seg] * 256 + (int64_t)tid * nt + t];
  __syncthreads();

  // wave w owns keys [sub, sub + SCENE_SUB) of the tile; step s ranks the 64 keys at sub + 64 s in lane order
  const int64_t sub = base + (int64_t)w * SCENE_SUB;
  uint32_t k[SCENE_PER], v[SCENE_PER], dr[SCENE_PER];
#pragma unroll
  for (int s = 0; s < SCENE_PER; ++s) {
    const int64_t i = sub + s * 64 + lane;
    const bool ok = i < end;
    if (FIRST) {
      k[s] = ok ? conf_key(r.conf[i]) : 0u;
      v[s] = (uint32_t)i;
    } else {
      k[s] = ok ? kin[r.off + i] : 0u;
      v[s] = ok ? vin[r.off + i] : 0u;
    }
  }
#pragma unroll
  for (int s = 0; s < SCENE_PER; ++s) {
    const bool ok = sub + s * 64 + lane < end;
    const uint32_t d = (k[s] >> shift) & 255u;
    const uint64_t peers = digit_peers(d, ok);
    const uint32_t below = (uint32_t)__popcll(peers & lanes_below());
    // cnt[w] belongs to this wave alone; a wave's LDS accesses execute in program order, so every lane has read before the leader writes
    const uint32_t c = cnt[w][d];
    if (ok && below == 0) cnt[w][d] = c + (uint32_t)__popcll(peers);
    dr[s] = d | ((c + below) << 8);  // rank within (wave, digit) < 1024
  }
  __syncthreads();
  {  // thread = digit: the waves' counts become exclusive prefixes over the waves; lbase = exclusive scan of the tile's digit totals
    const uint32_t c0 = cnt[0][tid], c1 = cnt[1][tid], c2 = cnt[2][tid], c3 = cnt[3][tid];
    cnt[0][tid] = 0;
    cnt[1][tid] = c0;
    cnt[2][tid] = c0 + c1;
    cnt[3][tid] = c0 + c1 + c2;
    const uint32_t tot = c0 + c1 + c2 + c3;
    uint32_t inc = tot;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t up = __shfl_up(inc, off, 64);
      if (lane >= off) inc += up;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint32_t wbase = 0;
    for (int j = 0; j < w; ++j) wbase += wsum[j];
    lbase[tid] = wbase + inc - tot;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < SCENE_PER; ++s) {
    if (sub + s * 64 + lane < end) {
      const uint32_t d = dr[s] & 255u;
      const uint32_t p = lbase[d] + cnt[w][d] + (dr[s] >> 8);
      sk[p] = k[s];
      sv[p] = v[s];
    }
  }
  __syncthreads();
  const int n_here = (int)(end - base);
  float mn = 0.f, den = 1.f;
  bool any_nan = false;
  if (FINAL) {
    any_nan = stats[seg * 4 + 2] != 0u;
    const float mx = conf_of_key(stats[seg * 4 + 0]);
    mn = conf_of_key(stats[seg * 4 + 1]);
    den = (mx - mn) + 1e-8f;
  }
  for (int p = tid; p < n_here; p += SCENE_NT) {
    const uint32_t kk = sk[p];
    const uint32_t d = (kk >> shift) & 255u;
    const int64_t q = r.off + gbase[d] + ((uint32_t)p - lbase[d]);
    if (!FINAL) {
      kout[q] = kk;
      vout[q] = sv[p];
    } else {
      const uint32_t idx = sv[p];
      o.order[q] = (int32_t)idx;
      // the key gives the confidence back exactly, except for a zero (its sign) and a NaN (its payload): those are read
      float c = conf_of_key(kk);
      if (kk == 0xffffffffu || c == 0.f) c = r.conf[idx];
      o.conf[q] = c;
      const u32x4 rec = recs[r.off + idx];  // one 16-byte gather: xyz, packed image colour, mask byte
      const uint32_t wx = rec[0], wy = rec[1], wz = rec[2];  // scalars first: a bit cast straight from a vector element reads element 0
      o.pts[q * 3 + 0] = __builtin_bit_cast(float, wx);
      o.pts[q * 3 + 1] = __builtin_bit_cast(float, wy);
      o.pts[q * 3 + 2] = __builtin_bit_cast(float, wz);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) o.rgb[q * 3 + ch] = (uint8_t)(rec[3] >> (8 * ch));
      o.mask[q] = (int8_t)(rec[3] >> 24);
      // matplotlib's Colormap.__call__ with N = 256 on t = (c - min) / (max - min + 1e-8) in fp32: x = t * 256, x == 256 -> 255,
      // under -> first entry, over -> last entry, NaN -> the "bad" colour (0, 0, 0)
      int li = -1;
      if (!any_nan) {
        const float tt = (c - mn) / den;
        const float xx = tt * 256.f;
        if (xx == xx) li = xx < 0.f ? 0 : (xx >= 256.f ? 255 : (int)xx);
      }
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) o.ccol[q * 3 + ch] = li < 0 ? (uint8_t)0 : slut[li * 3 + ch];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// scene extent: order statistics k[a][r] (axis a, r = 0..3) of p[3 i + a], i < m, by radix select over fkey()
constexpr int EXT_NT = 256;
struct ExtState {
  uint32_t prefix[12];
  uint32_t nan_count[3];
  uint32_t pad;
  int64_t k[12];
};
struct ExtRanks { int64_t k[4]; };

__global__ void ext_init_kernel(ExtState* st, ExtRanks rk) {
  const int i = threadIdx.x;
  if (i < 12) {
    st->prefix[i] = 0;
    st->k[i] = rk.k[i & 3];
  }
  if (i < 3) st->nan_count[i] = 0;
}

template <int PASS>
__global__ __launch_bounds__(EXT_NT) void ext_hist_kernel(const float* __restrict__ p, int64_t m, const ExtState* st,
                                                          uint32_t* __restrict__ hist /*[3][4][2048]*/, ExtState* st_w) {
  constexpr int shift = PASS == 0 ? 21 : (PASS == 1 ? 10 : 0);
  constexpr int nb = PASS == 2 ? 1024 : 2048;
  constexpr uint32_t pmask = PASS == 0 ? 0u : (PASS == 1 ? 0xffe00000u : 0xfffffc00u);
  constexpr int NR = PASS == 0 ? 1 : 4;  // the first pass is the same histogram for the four ranks of an axis
  __shared__ uint32_t lh[NR][2048];
  const int a = blockIdx.y;
  for (int j = threadIdx.x; j < NR * 2048; j += EXT_NT) (&lh[0][0])[j] = 0;
  uint32_t pre[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) pre[r] = st->prefix[a * 4 + r];
  __syncthreads();
  uint32_t nnan = 0;
  for (int64_t i = (int64_t)blockIdx.x * EXT_NT + threadIdx.x; i < m; i += (int64_t)gridDim.x * EXT_NT) {
    const float f = p[i * 3 + a];
    const uint32_t key = fkey(f);
    if (PASS == 0 && f != f) ++nnan;
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if (((key ^ pre[r]) & pmask) == 0u) atomicAdd(&lh[r][(key >> shift) & (nb - 1)], 1u);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < NR * 2048; j += EXT_NT) {
    const uint32_t c = (&lh[0][0])[j];
    if (c) atomicAdd(&hist[(a * 4) * 2048 + j], c);
  }
  if (PASS == 0 && nnan) atomicAdd(&st_w->nan_count[a], nnan);
}

template <int PASS>
__global__ void ext_pick_kernel(ExtState* st, const uint32_t* __restrict__ hist) {
  constexpr int shift = PASS == 0 ? 21 : (PASS == 1 ? 10 : 0);
  constexpr int nb = PASS == 2 ? 1024 : 2048;
  const int tg = threadIdx.x;
  if (tg >= 12) return;
  const uint32_t* h = hist + (PASS == 0 ? (tg & ~3) : tg) * 2048;
  int64_t k = st->k[tg], acc = 0;
  int b = 0;
  for (; b < nb - 1; ++b) {
    if (acc + h[b] > k) break;
    acc += h[b];
  }
  st->prefix[tg] |= (uint32_t)b << shift;
  st->k[tg] = k - acc;
}

__global__ void ext_final_kernel(const ExtState* st, uint32_t* out /*12 values as bits, 3 NaN counts*/) {
  const int i = threadIdx.x;
  if (i < 12) out[i] = __builtin_bit_cast(uint32_t, fkey_inv(st->prefix[i]));
  if (i < 3) out[12 + i] = st->nan_count[i];
}

// ---------------------------------------------------------------------------------------------------------------------------
// collect_points: per (view, head) the first `num` sorted entries, those with mask > 0 when there is a mask; tiles of 1024, one wave
constexpr int COL_TILE = 1024;
struct ColRow {  // 5 x 8 bytes
  const float* pts;
  const uint8_t* col;   // sorted colours, or null: the constant colour
  const int8_t* mask;   // sorted mask, or null: keep all
  int64_t num;
  int64_t const_col;    // r | g << 8 | b << 16
};

__global__ __launch_bounds__(64) void collect_count_kernel(const ColRow* __restrict__ rows, const int64_t* __restrict__ ts, int S,
                                                           uint32_t* __restrict__ counts) {
  const int seg = last_le(ts, 0, S, blockIdx.x);  // the segment that owns this tile (every segment has at least one)
  const ColRow r = rows[seg];
  uint32_t c[1];
  tile_count<COL_TILE>((blockIdx.x - ts[seg]) * COL_TILE, r.num, [&](int64_t i) { return !r.mask || r.mask[i] > 0; }, c);
  if (threadIdx.x == 0) counts[blockIdx.x] = c[0];
}

__global__ __launch_bounds__(64) void collect_write_kernel(const ColRow* __restrict__ rows, const int64_t* __restrict__ ts, int S,
                                                           const uint32_t* __restrict__ scan, float* __restrict__ out_pts,
                                                           uint8_t* __restrict__ out_col) {
  const int seg = last_le(ts, 0, S, blockIdx.x);  // the segment that owns this tile (every segment has at least one)
  const ColRow r = rows[seg];
  int64_t run[1] = {scan[blockIdx.x]};
  tile_compact<COL_TILE>(
      (blockIdx.x - ts[seg]) * COL_TILE, r.num, run, [&](int64_t i) { return !r.mask || r.mask[i] > 0; },
      [&](int64_t i, uint32_t, const int64_t(&q)[1]) {
        float p[3];  // every load before the first store: the compiler cannot tell that the outputs do not overlap the inputs
        uint8_t c[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          p[ch] = r.pts[i * 3 + ch];
          c[ch] = r.col ? r.col[i * 3 + ch] : (uint8_t)((r.const_col >> (8 * ch)) & 255);
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          out_pts[q[0] * 3 + ch] = p[ch];
          out_col[q[0] * 3 + ch] = c[ch];
        }
      });
}

// ---------------------------------------------------------------------------------------------------------------------------
// PLY records: 12 bytes of xyz (little-endian fp32) + 3 bytes of rgb; thread = one aligned output word
__global__ void ply_pack_kernel(const uint8_t* __restrict__ pts, const uint8_t* __restrict__ col, int64_t n, uint32_t* __restrict__ out) {
  const int64_t wi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nbytes = n * 15;
  if (wi * 4 >= nbytes) return;
  uint32_t word = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t b = wi * 4 + j;
    if (b < nbytes) {
      const int64_t rec = b / 15;
      const int off = (int)(b - rec * 15);
      const uint32_t byte = off < 12 ? pts[rec * 12 + off] : col[rec * 3 + (off - 12)];
      word |= byte << (8 * j);
    }
  }
  out[wi] = word;
}

__global__ void color_range_init_kernel(unsigned long long* out) {
  out[0] = ~0ull;
  out[1] = 0ull;
  out[2] = 0ull;
}

// out = {key of the minimum, key of the maximum, NaN count} over the values widened (exactly) to fp64
template <class T>
__global__ __launch_bounds__(256) void color_range_kernel(const T* __restrict__ c, int64_t n, unsigned long long* __restrict__ out) {
  unsigned long long kmin = ~0ull, kmax = 0ull, nnan = 0ull;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double f = (double)c[i];
    if (f != f) {
      ++nnan;
    } else {
      const uint64_t k = dkey(f);
      kmin = min(kmin, (unsigned long long)k);
      kmax = max(kmax, (unsigned long long)k);
    }
  }
  if (kmin != ~0ull) {
    atomicMin(&out[0], kmin);
    atomicMax(&out[1], kmax);
  }
  if (nnan) atomicAdd(&out[2], nnan);
}

// safe_color_conversion in the input's own type T: rule 0: c * 255; 1: (c + 1) * 127.5; 2: ((c - mn) / (mx - mn)) * 255; clip, truncate
template <class T>
__global__ void color_to_u8_kernel(const T* __restrict__ c, int64_t n, int rule, T mn, T mx, uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const T x = c[i];
  T y;
  if (rule == 0) y = x * (T)255;
  else if (rule == 1) y = (x + (T)1) * (T)127.5;
  else y = ((x - mn) / (mx - mn)) * (T)255;
  out[i] = !(y > (T)0) ? (uint8_t)0 : (y >= (T)255 ? (uint8_t)255 : (uint8_t)(int)y);
}

constexpr size_t EXT_HIST_BYTES = 3 * 4 * 2048 * sizeof(uint32_t);

// the workspaces, sized on a null base and carved on the caller's (a braced list is evaluated left to right: the regions lie in that order)
struct SortWs {
  uint32_t *k0, *v0, *k1, *v1, *hist;
  u32x4* recs;
  size_t bytes;
};
SortWs sort_ws(void* base, int64_t n, int64_t n_tiles) {
  Carve c(base, 256);
  return {c.take<uint32_t>(n), c.take<uint32_t>(n), c.take<uint32_t>(n), c.take<uint32_t>(n), c.take<uint32_t>(n_tiles * 256), c.take<u32x4>(n), c.bytes()};
}
struct ExtWs {
  uint32_t* hist;
  ExtState* st;
  size_t bytes;
};
ExtWs ext_ws(void* base) {
  Carve c(base, 256);
  return {c.take<uint32_t>(EXT_HIST_BYTES / sizeof(uint32_t)), c.take<ExtState>(1), c.bytes()};
}

}  // namespace

extern "C" size_t f3r_scene_sort_workspace_bytes(int64_t total_keys, int64_t n_tiles) {
  if (total_keys < 1 || n_tiles < 1) return 0;
  return sort_ws(nullptr, total_keys, n_tiles).bytes;
}

extern "C" int f3r_scene_sort(const int64_t* table, int n_segments, int64_t n_tiles, int64_t total_keys, const uint8_t* lut, void* workspace,
                              size_t workspace_bytes, int32_t* order, float* pts, float* conf, uint8_t* rgb, uint8_t* conf_rgb, int8_t* mask,
                              uint32_t* stats, f3r_stream_t stream) {
  F3R_REQUIRE(table && lut && workspace && order && pts && conf && rgb && conf_rgb && mask && stats, "f3r_scene_sort: null pointer");
  F3R_REQUIRE(n_segments >= 1 && n_tiles >= n_segments && n_tiles < (1ll << 31) && total_keys >= n_segments,
              "f3r_scene_sort: need n_segments >= 1, one tile or more per segment and fewer than 2^31 tiles (got %d segments, %lld tiles, %lld keys)",
              n_segments, (long long)n_tiles, (long long)total_keys);
  F3R_REQUIRE(workspace_bytes >= f3r_scene_sort_workspace_bytes(total_keys, n_tiles), "f3r_scene_sort: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const SegRow* rows = (const SegRow*)table;
  const int64_t* ts = table + (int64_t)n_segments * 6;
  const auto [k0, v0, k1, v1, hist, recs, ws_bytes] = sort_ws(workspace, total_keys, n_tiles);
  const SceneOut o = {order, pts, conf, rgb, conf_rgb, mask};
  const dim3 g((unsigned)n_tiles), b(SCENE_NT);
  hipLaunchKernelGGL(scene_stats_init_kernel, dim3((n_segments * 4 + 255) / 256), dim3(256), 0, s, stats, n_segments);
  // pass 0: conf -> (k0, v0)
  hipLaunchKernelGGL(scene_hist_kernel<true>, g, b, 0, s, rows, ts, n_segments, (const uint32_t*)nullptr, 0, hist, stats, recs);
  hipLaunchKernelGGL(exclusive_scan_rows_kernel<SCAN_NT>, dim3(n_segments), dim3(SCAN_NT), 0, s, hist, ts, (int64_t)0, (uint32_t*)nullptr);
  hipLaunchKernelGGL((scene_scatter_kernel<true, false>), g, b, 0, s, rows, ts, n_segments, (const uint32_t*)nullptr, (const uint32_t*)nullptr, 0,
                     hist, k0, v0, o, stats, lut, recs);
  // passes 1, 2: (k0, v0) -> (k1, v1) -> (k0, v0)
  for (int pass = 1; pass <= 2; ++pass) {
    uint32_t *ki = pass == 1 ? k0 : k1, *vi = pass == 1 ? v0 : v1, *ko = pass == 1 ? k1 : k0, *vo = pass == 1 ? v1 : v0;
    hipLaunchKernelGGL(scene_hist_kernel<false>, g, b, 0, s, rows, ts, n_segments, ki, 8 * pass, hist, stats, recs);
    hipLaunchKernelGGL(exclusive_scan_rows_kernel<SCAN_NT>, dim3(n_segments), dim3(SCAN_NT), 0, s, hist, ts, (int64_t)0, (uint32_t*)nullptr);
    hipLaunchKernelGGL((scene_scatter_kernel<false, false>), g, b, 0, s, rows, ts, n_segments, ki, vi, 8 * pass, hist, ko, vo, o, stats, lut, recs);
  }
  // pass 3: (k0, v0) -> the order and every gathered output
  hipLaunchKernelGGL(scene_hist_kernel<false>, g, b, 0, s, rows, ts, n_segments, k0, 24, hist, stats, recs);
  hipLaunchKernelGGL(exclusive_scan_rows_kernel<SCAN_NT>, dim3(n_segments), dim3(SCAN_NT), 0, s, hist, ts, (int64_t)0, (uint32_t*)nullptr);
  hipLaunchKernelGGL((scene_scatter_kernel<false, true>), g, b, 0, s, rows, ts, n_segments, k0, v0, 24, hist, (uint32_t*)nullptr,
                     (uint32_t*)nullptr, o, stats, lut, recs);
  return f3r_check_launch("f3r_scene_sort");
}

extern "C" size_t f3r_scene_extent_workspace_bytes(void) { return ext_ws(nullptr).bytes; }

extern "C" int f3r_scene_extent(const float* pts, int64_t m, const int64_t* ranks, void* workspace, size_t workspace_bytes, uint32_t* out,
                                f3r_stream_t stream) {
  F3R_REQUIRE(pts && ranks && workspace && out, "f3r_scene_extent: null pointer");
  F3R_REQUIRE(m >= 1, "f3r_scene_extent: no points");
  F3R_REQUIRE(workspace_bytes >= f3r_scene_extent_workspace_bytes(), "f3r_scene_extent: workspace too small");
  ExtRanks rk;
  for (int r = 0; r < 4; ++r) {
    F3R_REQUIRE(ranks[r] >= 0 && ranks[r] < m, "f3r_scene_extent: rank %d = %lld outside [0, %lld)", r, (long long)ranks[r], (long long)m);
    rk.k[r] = ranks[r];
  }
  hipStream_t s = (hipStream_t)stream;
  const auto [hist, st, ws_bytes] = ext_ws(workspace);
  const unsigned nb = (unsigned)std::min<int64_t>(1024, (m + EXT_NT - 1) / EXT_NT);
  hipLaunchKernelGGL(ext_init_kernel, dim3(1), dim3(64), 0, s, st, rk);
  if (hipMemsetAsync(hist, 0, EXT_HIST_BYTES, s) != hipSuccess) return f3r_check_launch("f3r_scene_extent");
  hipLaunchKernelGGL(ext_hist_kernel<0>, dim3(nb, 3), dim3(EXT_NT), 0, s, pts, m, st, hist, st);
  hipLaunchKernelGGL(ext_pick_kernel<0>, dim3(1), dim3(64), 0, s, st, hist);
  if (hipMemsetAsync(hist, 0, EXT_HIST_BYTES, s) != hipSuccess) return f3r_check_launch("f3r_scene_extent");
  hipLaunchKernelGGL(ext_hist_kernel<1>, dim3(nb, 3), dim3(EXT_NT), 0, s, pts, m, st, hist, st);
  hipLaunchKernelGGL(ext_pick_kernel<1>, dim3(1), dim3(64), 0, s, st, hist);
  if (hipMemsetAsync(hist, 0, EXT_HIST_BYTES, s) != hipSuccess) return f3r_check_launch("f3r_scene_extent");
  hipLaunchKernelGGL(ext_hist_kernel<2>, dim3(nb, 3), dim3(EXT_NT), 0, s, pts, m, st, hist, st);
  hipLaunchKernelGGL(ext_pick_kernel<2>, dim3(1), dim3(64), 0, s, st, hist);
  hipLaunchKernelGGL(ext_final_kernel, dim3(1), dim3(64), 0, s, st, out);
  return f3r_check_launch("f3r_scene_extent");
}

extern "C" int f3r_scene_collect_count(const int64_t* table, int n_segments, int64_t n_tiles, uint32_t* scan, f3r_stream_t stream) {
  F3R_REQUIRE(table && scan, "f3r_scene_collect_count: null pointer");
  F3R_REQUIRE(n_segments >= 1 && n_tiles >= n_segments && n_tiles < (1ll << 22),
              "f3r_scene_collect_count: need one tile or more per segment and fewer than 2^22 tiles (got %d segments, %lld tiles)", n_segments,
              (long long)n_tiles);
  hipStream_t s = (hipStream_t)stream;
  const int64_t* ts = table + (int64_t)n_segments * 5;
  hipLaunchKernelGGL(collect_count_kernel, dim3((unsigned)n_tiles), dim3(64), 0, s, (const ColRow*)table, ts, n_segments, scan);
  hipLaunchKernelGGL(exclusive_scan_rows_kernel<SCAN_NT>, dim3(1), dim3(SCAN_NT), 0, s, scan, (const int64_t*)nullptr, n_tiles, scan + n_tiles);
  return f3r_check_launch("f3r_scene_collect_count");
}

extern "C" int f3r_scene_collect_write(const int64_t* table, int n_segments, int64_t n_tiles, const uint32_t* scan, float* out_pts, uint8_t* out_rgb,
                                       f3r_stream_t stream) {
  F3R_REQUIRE(table && scan && out_pts && out_rgb, "f3r_scene_collect_write: null pointer");
  F3R_REQUIRE(n_segments >= 1 && n_tiles >= n_segments && n_tiles < (1ll << 22), "f3r_scene_collect_write: bad tile count");
  hipStream_t s = (hipStream_t)stream;
  const int64_t* ts = table + (int64_t)n_segments * 5;
  hipLaunchKernelGGL(collect_write_kernel, dim3((unsigned)n_tiles), dim3(64), 0, s, (const ColRow*)table, ts, n_segments, scan, out_pts, out_rgb);
  return f3r_check_launch("f3r_scene_collect_write");
}

extern "C" int f3r_ply_pack(const float* pts, const uint8_t* rgb, int64_t n, void* out, f3r_stream_t stream) {
  F3R_REQUIRE(n >= 0, "f3r_ply_pack: n < 0");
  if (n == 0) return F3R_OK;
  F3R_REQUIRE(pts && rgb && out, "f3r_ply_pack: null pointer");
  F3R_REQUIRE(((uintptr_t)out & 3) == 0, "f3r_ply_pack: out must be 4-byte aligned (and hold 15 n bytes rounded up to 4)");
  const int64_t words = (n * 15 + 3) / 4;
  F3R_REQUIRE(words < (1ll << 39), "f3r_ply_pack: too many points");
  hipLaunchKernelGGL(ply_pack_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)pts, rgb, n,
                     (uint32_t*)out);
  return f3r_check_launch("f3r_ply_pack");
}

extern "C" int f3r_color_range(const void* colors, int64_t n, int dtype, uint64_t* out, f3r_stream_t stream) {
  F3R_REQUIRE(colors && out && n >= 1, "f3r_color_range: null pointer or no values");
  F3R_REQUIRE(dtype == F3R_REAL_F32 || dtype == F3R_REAL_F64, "f3r_color_range: dtype %d", dtype);
  hipStream_t s = (hipStream_t)stream;
  const unsigned nb = (unsigned)std::min<int64_t>(2048, (n + 255) / 256);
  hipLaunchKernelGGL(color_range_init_kernel, dim3(1), dim3(1), 0, s, (unsigned long long*)out);
  if (dtype == F3R_REAL_F32)
    hipLaunchKernelGGL(color_range_kernel<float>, dim3(nb), dim3(256), 0, s, (const float*)colors, n, (unsigned long long*)out);
  else
    hipLaunchKernelGGL(color_range_kernel<double>, dim3(nb), dim3(256), 0, s, (const double*)colors, n, (unsigned long long*)out);
  return f3r_check_launch("f3r_color_range");
}

extern "C" int f3r_color_to_u8(const void* colors, int64_t n, int dtype, int rule, double lo, double hi, uint8_t* out, f3r_stream_t stream) {
  F3R_REQUIRE(colors && out && n >= 1, "f3r_color_to_u8: null pointer or no values");
  F3R_REQUIRE(dtype == F3R_REAL_F32 || dtype == F3R_REAL_F64, "f3r_color_to_u8: dtype %d", dtype);
  F3R_REQUIRE(rule >= 0 && rule <= 2, "f3r_color_to_u8: rule %d", rule);
  F3R_REQUIRE(rule != 2 || hi != lo, "f3r_color_to_u8: rule 2 with hi == lo divides by zero");
  hipStream_t s = (hipStream_t)stream;
  const dim3 g((unsigned)((n + 255) / 256)), b(256);
  F3R_REQUIRE((n + 255) / 256 < (1ll << 31), "f3r_color_to_u8: too many values");
  if (dtype == F3R_REAL_F32)
    hipLaunchKernelGGL(color_to_u8_kernel<float>, g, b, 0, s, (const float*)colors, n, rule, (float)lo, (float)hi, out);
  else
    hipLaunchKernelGGL(color_to_u8_kernel<double>, g, b, 0, s, (const double*)colors, n, rule, lo, hi, out);
  return f3r_check_launch("f3r_color_to_u8");
}
