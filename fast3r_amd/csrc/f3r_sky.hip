// Sky detection (ABI 400; include/f3r.h "sky detection"): the reference's detect_sky_mask (fast3r/viz/viser_visualizer.py:24-72) for all
// views of a scene at once -- OpenCV's 8-bit HSV, three colour ranges and the upper-region rule, a 7 x 7 dilation and a 7 x 7 opening,
// scipy's 4-connected labelling, and the top-row / 1 % rule -- as integer kernels on a bit-packed bitmap (one 64-bit word per 64 pixels
// of a row, f3r_ccl.h).  Views differ in H x W; one device table describes them, as in f3r_scene_sort.
//
// * sky_pack_kernel: a wave reads 64 pixels of a row (the three fp32 planes as stored, or a caller's int8 bitmap) and ballots the word.
// * sky_morph_kernel: one 7 x 7 box pass (OR or AND), thread = output word: 7 rows x 3 words, shifts across the word borders.  Pixels
//   outside the image are ignored (OpenCV's default morphology border), so the fill is 0 for OR and 1 for AND; nothing is tiled, so
//   there is no halo: the 21 words come from the bitmap itself, which is 1 / 96 of the image's bytes and stays in cache.
// * sky_init_kernel / sky_merge_kernel / sky_flatten_kernel: union-find over the set pixels (f3r_ccl.h): run starts, one union per
//   vertical run-to-run contact, then every pixel stores its root = the smallest pixel index of its component.  A component touches
//   row 0 exactly when its root is < W, so sizes are only kept for those (W counters per view), one atomic per run and word.
// * sky_apply_kernel: the rule, not_sky as int8, the optional root image, the kept count and the branch.
// Only integer atomics are used, and every output is a function of the partition alone: two runs give the same bits.  Built with
// -ffp-contract=off: (img + 1) * 127.5 is an fp32 add and an fp32 multiply, each rounded, as numpy computes it.
#include "f3r_ccl.h"
#include "f3r_common.h"
#include "f3r_prims.h"

#include <utility>

namespace {

constexpr int SKY_NT = 256;          // threads of a workgroup (4 waves)
constexpr int SKY_PIX_TILE = 16;     // words per workgroup of the wave-per-word kernels: 4 per wave
constexpr int SKY_WORD_TILE = 256;   // words per workgroup of the thread-per-word kernels
static_assert(SKY_PIX_TILE == F3R_SKY_PIX_TILE && SKY_WORD_TILE == F3R_SKY_WORD_TILE, "include/f3r.h states the tile lengths");
constexpr int SKY_ROW = 10;          // int64 per table row

struct SkyRow {  // one row of the device table, 10 x 8 bytes
  const void* src;     // fp32 planes (3, H * W), or an int8 (H, W) bitmap
  int8_t* not_sky;     // (H, W) out, or null
  int32_t* roots;      // (H, W) out, or null
  int64_t H, W;
  int64_t word_off;    // the view's first word in the bitmaps
  int64_t pix_off;     // its first entry in the parent array
  int64_t width_off;   // its first entry in the top-row size counters
  int64_t thr;         // floor(H * W * 0.01), formed in double on the host
  int64_t upper;       // int(H * 0.4)
};
static_assert(sizeof(SkyRow) == SKY_ROW * 8, "table row layout");

// OpenCV's 12-bit fixed-point HSV tables: sdiv[i] = rint((255 << 12) / i), hdiv[i] = rint((180 << 12) / (6 i)), rint = to nearest even
struct HsvTab {
  int32_t sdiv[256], hdiv[256];
};
constexpr int32_t rint_div(int32_t n, int32_t i) {
  const int32_t q = n / i, r = n % i;
  return 2 * r > i ? q + 1 : (2 * r == i ? q + (q & 1) : q);
}
constexpr HsvTab make_hsv_tab() {
  HsvTab t{};
  for (int i = 1; i < 256; ++i) {
    t.sdiv[i] = rint_div(255 << 12, i);
    t.hdiv[i] = rint_div((180 << 12) / 6, i);  // (180 << 12) / 6 = 122880 exactly, so the quotient by i is the same real number
  }
  return t;
}
__constant__ HsvTab kHsvTab = make_hsv_tab();

// steps 1-3 for one pixel: is it sky-coloured?
__device__ __forceinline__ bool sky_colour(float fr, float fg, float fb, bool in_upper, const int32_t* sdiv, const int32_t* hdiv) {
  const int r = colour_u8(fr), g = colour_u8(fg), b = colour_u8(fb);
  const int v = max(r, max(g, b)), mn = min(r, min(g, b)), d = v - mn;
  const int s = (d * sdiv[v] + 2048) >> 12;
  const int h0 = v == r ? g - b : (v == g ? b - r + 2 * d : r - g + 4 * d);
  int h = (h0 * hdiv[d] + 2048) >> 12;  // arithmetic shift
  if (h < 0) h += 180;
  const bool blue = h >= 105 && h <= 135 && s >= 50 && v >= 140;
  const bool light = h >= 95 && h <= 145 && s >= 5 && s <= 100 && v >= 150;
  const bool white = s <= 10 && v >= 235;  // h <= 180 always
  return blue || light || white || (in_upper && s < 50 && v > 150);
}

__device__ __forceinline__ int64_t words_per_row(int64_t W) { return (W + 63) >> 6; }
__device__ __forceinline__ uint64_t valid_bits(int64_t xw, int64_t WW, int64_t W) {
  const int rem = (int)(W & 63);
  return (xw == WW - 1 && rem) ? ((1ull << rem) - 1ull) : ~0ull;
}

// the view that owns this workgroup's tile and the tile's first word within the view
struct TileAt {
  int seg;
  int64_t word0;
};
__device__ __forceinline__ TileAt tile_at(const int64_t* __restrict__ ts, int S, int tile_words) {
  const int seg = last_le(ts, 0, S, (int64_t)blockIdx.x);
  return {seg, ((int64_t)blockIdx.x - ts[seg]) * tile_words};
}

// ---- wave = word: bits[word] = ballot over its 64 pixels
template <bool FROM_IMG>
__global__ __launch_bounds__(SKY_NT) void sky_pack_kernel(const SkyRow* __restrict__ rows, const int64_t* __restrict__ ts, int S,
                                                          uint64_t* __restrict__ bits) {
  __shared__ int32_t sdiv[256], hdiv[256];
  if (FROM_IMG) {
    sdiv[threadIdx.x] = kHsvTab.sdiv[threadIdx.x];
    hdiv[threadIdx.x] = kHsvTab.hdiv[threadIdx.x];
    __syncthreads();
  }
  const TileAt t = tile_at(ts, S, SKY_PIX_TILE);
  const SkyRow r = rows[t.seg];
  const int64_t WW = words_per_row(r.W), n_words = r.H * WW, HW = r.H * r.W;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int j = 0; j < SKY_PIX_TILE / 4; ++j) {
    const int64_t wi = t.word0 + wv * (SKY_PIX_TILE / 4) + j;  // uniform over the wave
    if (wi >= n_words) break;
    const int64_t y = wi / WW, x = (wi - y * WW) * 64 + lane;
    bool set = false;
    if (x < r.W) {
      const int64_t p = y * r.W + x;
      if (FROM_IMG) {
        const float* img = (const float*)r.src;
        set = sky_colour(img[p], img[HW + p], img[2 * HW + p], y < r.upper, sdiv, hdiv);
      } else {
        set = ((const int8_t*)r.src)[p] != 0;
      }
    }
    const uint64_t w = __ballot(set);
    if (lane == 0) bits[r.word_off + wi] = w;
  }
}

// ---- thread = output word: one 7 x 7 box pass
template <bool AND>
__global__ __launch_bounds__(SKY_NT) void sky_morph_kernel(const SkyRow* __restrict__ rows, const int64_t* __restrict__ ts, int S,
                                                           const uint64_t* __restrict__ in, uint64_t* __restrict__ out) {
  const TileAt t = tile_at(ts, S, SKY_WORD_TILE);
  const SkyRow r = rows[t.seg];
  const int64_t WW = words_per_row(r.W), n_words = r.H * WW;
  const int64_t wi = t.word0 + threadIdx.x;
  if (wi >= n_words) return;
  const int64_t y = wi / WW, xw = wi - y * WW;
  const uint64_t* b = in + r.word_off;
  constexpr uint64_t FILL = AND ? ~0ull : 0ull;  // what a pixel outside the image contributes: nothing
  // for AND the bits of the last word beyond W are outside the image too
  const uint64_t pad_c = AND ? ~valid_bits(xw, WW, r.W) : 0ull;
  const uint64_t pad_r = (AND && xw + 1 < WW) ? ~valid_bits(xw + 1, WW, r.W) : 0ull;
  uint64_t acc = FILL;
  for (int dy = -3; dy <= 3; ++dy) {
    const int64_t yy = y + dy;
    if (yy < 0 || yy >= r.H) continue;
    const uint64_t* row = b + yy * WW;
    const uint64_t c = row[xw] | pad_c;
    const uint64_t l = xw > 0 ? row[xw - 1] : FILL;  // a word left of the last one is full: no padding bits
    const uint64_t rt = xw + 1 < WW ? (row[xw + 1] | pad_r) : FILL;
    uint64_t h = c;
#pragma unroll
    for (int k = 1; k <= 3; ++k) {
      const uint64_t from_left = (c << k) | (l >> (64 - k));    // bit i = pixel x - k
      const uint64_t from_right = (c >> k) | (rt << (64 - k));  // bit i = pixel x + k
      if (AND) h &= from_left & from_right; else h |= from_left | from_right;
    }
    if (AND) acc &= h; else acc |= h;
  }
  out[r.word_off + wi] = acc & valid_bits(xw, WW, r.W);
}

// ---- wave = word: parent of every set pixel = its run start (f3r_ccl.h)
__global__ __launch_bounds__(SKY_NT) void sky_init_kernel(const SkyRow* __restrict__ rows, const int64_t* __restrict__ ts, int S,
                                                          const uint64_t* __restrict__ bits, int32_t* __restrict__ parent) {
  const TileAt t = tile_at(ts, S, SKY_PIX_TILE);
  const SkyRow r = rows[t.seg];
  const int64_t WW = words_per_row(r.W), n_words = r.H * WW;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int j = 0; j < SKY_PIX_TILE / 4; ++j) {
    const int64_t wi = t.word0 + wv * (SKY_PIX_TILE / 4) + j;
    if (wi >= n_words) break;
    const uint64_t w = bits[r.word_off + wi];
    if (!((w >> lane) & 1ull)) continue;  // bits at x >= W are 0
    const int64_t y = wi / WW, xw = wi - y * WW;
    const bool prev_last = xw > 0 && (bits[r.word_off + wi - 1] >> 63);
    const int32_t p = (int32_t)(y * r.W + xw * 64 + lane);
    parent[r.pix_off + p] = f3r_ccl::initial_parent(w, lane, prev_last, p);
  }
}

// ---- thread = word: one union per run of vertical contacts with the row above
__global__ __launch_bounds__(SKY_NT) void sky_merge_kernel(const SkyRow* __restrict__ rows, const int64_t* __restrict__ ts, int S,
                                                           const uint64_t* __restrict__ bits, int32_t* __restrict__ parent) {
  const TileAt t = tile_at(ts, S, SKY_WORD_TILE);
  const SkyRow r = rows[t.seg];
  const int64_t WW = words_per_row(r.W), n_words = r.H * WW;
  const int64_t wi = t.word0 + threadIdx.x;
  if (wi < WW || wi >= n_words) return;  // row 0 has no row above
  const uint64_t* b = bits + r.word_off;
  const uint64_t w = b[wi], up = b[wi - WW];
  if (!(w & up)) return;
  const int64_t y = wi / WW, xw = wi - y * WW;
  const bool prev_link = xw > 0 && ((b[wi - 1] & b[wi - 1 - WW]) >> 63);
  uint64_t starts = f3r_ccl::link_starts(w, up, prev_link);
  int32_t* par = parent + r.pix_off;
  const int32_t p0 = (int32_t)(y * r.W + xw * 64);
  while (starts) {  // at most 32 rounds: each clears one bit
    const int bit = f3r_ccl::ctz64(starts);
    starts &= starts - 1ull;
    f3r_ccl::unite(par, p0 + bit, p0 + bit - (int32_t)r.W);  // loops bounded by construction: f3r_ccl.h
  }
}

// stats[view * 5 + {0: set pixels, 1: components, 2: components touching row 0, 3: components kept, 4: branch}]
// ---- wave = word: every set pixel stores its root; counts; the sizes of the components that touch row 0
__global__ __launch_bounds__(SKY_NT) void sky_flatten_kernel(const SkyRow* __restrict__ rows, const int64_t* __restrict__ ts, int S,
                                                             const uint64_t* __restrict__ bits, int32_t* __restrict__ parent,
                                                             int32_t* __restrict__ top_size, int32_t* __restrict__ stats) {
  const TileAt t = tile_at(ts, S, SKY_PIX_TILE);
  const SkyRow r = rows[t.seg];
  const int64_t WW = words_per_row(r.W), n_words = r.H * WW;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int32_t* par = parent + r.pix_off;
  int32_t n_set = 0, n_root = 0, n_top = 0;  // the wave's counts (uniform)
  for (int j = 0; j < SKY_PIX_TILE / 4; ++j) {
    const int64_t wi = t.word0 + wv * (SKY_PIX_TILE / 4) + j;
    if (wi >= n_words) break;
    const uint64_t w = bits[r.word_off + wi];
    if (!w) continue;
    const bool set = (w >> lane) & 1ull;
    const int64_t y = wi / WW, xw = wi - y * WW;
    const int32_t p = (int32_t)(y * r.W + xw * 64 + lane);
    int32_t root = -1;
    if (set) {
      root = f3r_ccl::find_root(par, p);  // the merge kernel has finished: this is the component's final root
      f3r_ccl::store(par + p, root);      // a root keeps pointing at itself; a concurrent find reads the old or the new ancestor
      if (root < r.W && (lane == 0 || !((w >> (lane - 1)) & 1ull))) atomicAdd(top_size + r.width_off + root, f3r_ccl::run_length(w, lane));
    }
    n_set += __popcll(w);
    n_root += (int32_t)wave_flag_count(set && root == p);
    n_top += (int32_t)wave_flag_count(set && root == p && p < r.W);
  }
  if (lane == 0) {
    if (n_set) atomicAdd(stats + t.seg * 5 + 0, n_set);
    if (n_root) atomicAdd(stats + t.seg * 5 + 1, n_root);
    if (n_top) atomicAdd(stats + t.seg * 5 + 2, n_top);
  }
}

// ---- wave = word: the rule of step 5 and the outputs
__global__ __launch_bounds__(SKY_NT) void sky_apply_kernel(const SkyRow* __restrict__ rows, const int64_t* __restrict__ ts, int S,
                                                           const uint64_t* __restrict__ bits, const int32_t* __restrict__ parent,
                                                           const int32_t* __restrict__ top_size, int32_t* __restrict__ stats) {
  const TileAt t = tile_at(ts, S, SKY_PIX_TILE);
  const SkyRow r = rows[t.seg];
  const int64_t WW = words_per_row(r.W), n_words = r.H * WW;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int32_t* par = parent + r.pix_off;
  const int32_t* size = top_size + r.width_off;
  // written by the flatten kernel, complete at this kernel's start; this kernel writes words 3 and 4 only
  const int32_t n_set = stats[t.seg * 5 + 0], n_comp = stats[t.seg * 5 + 1], n_top = stats[t.seg * 5 + 2];
  const int branch = n_set == 0 ? F3R_SKY_EMPTY : (n_top == 0 ? F3R_SKY_NO_TOP : F3R_SKY_TOP);
  int32_t n_kept = 0;
  for (int j = 0; j < SKY_PIX_TILE / 4; ++j) {
    const int64_t wi = t.word0 + wv * (SKY_PIX_TILE / 4) + j;
    if (wi >= n_words) break;
    const uint64_t w = bits[r.word_off + wi];
    const int64_t y = wi / WW, x = (wi - y * WW) * 64 + lane;
    if (wi == 0 && lane == 0) {
      stats[t.seg * 5 + 4] = branch;
      if (branch == F3R_SKY_NO_TOP) stats[t.seg * 5 + 3] = n_comp;  // the mask is left as it is: every component stays
    }
    const bool inside = x < r.W;
    const bool set = inside && ((w >> lane) & 1ull);
    const int64_t p = y * r.W + x;
    int32_t root = -1;
    bool sky = false;
    if (set) {
      root = par[p];
      sky = branch != F3R_SKY_TOP || (root < r.W && (int64_t)size[root] > r.thr);
    }
    if (inside) {
      if (r.not_sky) r.not_sky[p] = sky ? (int8_t)0 : (int8_t)1;
      if (r.roots) r.roots[p] = root;
    }
    if (branch == F3R_SKY_TOP && y == 0) n_kept += (int32_t)wave_flag_count(set && root == (int32_t)p && sky);
  }
  if (lane == 0 && n_kept) atomicAdd(stats + t.seg * 5 + 3, n_kept);
}

// the workspace, sized on a null base and carved on the caller's (a braced list is evaluated left to right: the regions lie in that order)
struct SkyWs {
  uint64_t *cur, *other;
  int32_t *parent, *top_size;  // empty without F3R_SKY_LABEL
  size_t bytes;
};
SkyWs sky_ws(void* base, int64_t total_words, int64_t total_pixels, int64_t total_width, int stages) {
  const bool label = stages & F3R_SKY_LABEL;
  Carve c(base, 256);
  return {c.take<uint64_t>(total_words), c.take<uint64_t>(total_words), c.take<int32_t>(label ? total_pixels : 0),
          c.take<int32_t>(label ? total_width : 0), c.bytes()};
}

}  // namespace

extern "C" size_t f3r_sky_workspace_bytes(int64_t total_words, int64_t total_pixels, int64_t total_width, int stages) {
  if (total_words < 1 || total_pixels < 1 || total_width < 1) return 0;
  return sky_ws(nullptr, total_words, total_pixels, total_width, stages).bytes;
}

extern "C" int f3r_sky_detect(const int64_t* table, const int64_t* host_hw, int n_views, int64_t n_pix_tiles, int64_t n_word_tiles,
                              int64_t total_words, int64_t total_pixels, int64_t total_width, int stages, void* workspace,
                              size_t workspace_bytes, int32_t* stats, uint64_t* bits_out, f3r_stream_t stream) {
  F3R_REQUIRE(table && host_hw && workspace, "f3r_sky_detect: null pointer");
  F3R_REQUIRE(n_views >= 1, "f3r_sky_detect: n_views = %d < 1", n_views);
  constexpr int ALL = F3R_SKY_CLASSIFY | F3R_SKY_MORPH | F3R_SKY_LABEL;
  F3R_REQUIRE(stages > 0 && (stages & ~ALL) == 0, "f3r_sky_detect: stages = %d is no combination of F3R_SKY_CLASSIFY | _MORPH | _LABEL", stages);
  F3R_REQUIRE(!(stages & F3R_SKY_LABEL) || stats, "f3r_sky_detect: F3R_SKY_LABEL needs stats");
  F3R_REQUIRE((stages & F3R_SKY_LABEL) || bits_out, "f3r_sky_detect: without F3R_SKY_LABEL the bitmap is the only output: bits_out is null");
  // the host's copy of the shapes must add up to the totals the launches are sized by: a mismatch is an argument error, not a wild write
  int64_t words = 0, pixels = 0, width = 0, ptiles = 0, wtiles = 0;
  for (int i = 0; i < n_views; ++i) {
    const int64_t H = host_hw[2 * i], W = host_hw[2 * i + 1];
    F3R_REQUIRE(H >= 1 && W >= 1 && H < (1ll << 31) && W < (1ll << 31) && H * W < (1ll << 31),
                "f3r_sky_detect: view %d is %lld x %lld; need H, W >= 1 and H * W < 2^31", i, (long long)H, (long long)W);
    const int64_t nw = H * ((W + 63) / 64);
    words += nw;
    pixels += H * W;
    width += W;
    ptiles += (nw + SKY_PIX_TILE - 1) / SKY_PIX_TILE;
    wtiles += (nw + SKY_WORD_TILE - 1) / SKY_WORD_TILE;
  }
  F3R_REQUIRE(words == total_words && pixels == total_pixels && width == total_width && ptiles == n_pix_tiles && wtiles == n_word_tiles,
              "f3r_sky_detect: the totals do not match the shapes (words %lld / %lld, pixels %lld / %lld, widths %lld / %lld, tiles %lld / %lld and "
              "%lld / %lld)", (long long)total_words, (long long)words, (long long)total_pixels, (long long)pixels, (long long)total_width,
              (long long)width, (long long)n_pix_tiles, (long long)ptiles, (long long)n_word_tiles, (long long)wtiles);
  F3R_REQUIRE(n_pix_tiles < (1ll << 31), "f3r_sky_detect: too many tiles");
  F3R_REQUIRE(workspace_bytes >= f3r_sky_workspace_bytes(total_words, total_pixels, total_width, stages), "f3r_sky_detect: workspace too small");

  hipStream_t s = (hipStream_t)stream;
  const SkyRow* rows = (const SkyRow*)table;
  const int64_t* ts_pix = table + (int64_t)n_views * SKY_ROW;
  const int64_t* ts_word = ts_pix + n_views + 1;
  auto [cur, other, parent, top_size, ws_bytes] = sky_ws(workspace, total_words, total_pixels, total_width, stages);
  const dim3 gp((unsigned)n_pix_tiles), gw((unsigned)n_word_tiles), b(SKY_NT);

  if (stages & F3R_SKY_CLASSIFY)
    hipLaunchKernelGGL(sky_pack_kernel<true>, gp, b, 0, s, rows, ts_pix, n_views, cur);
  else
    hipLaunchKernelGGL(sky_pack_kernel<false>, gp, b, 0, s, rows, ts_pix, n_views, cur);
  if (stages & F3R_SKY_MORPH) {  // dilate, then open = erode, dilate
    hipLaunchKernelGGL(sky_morph_kernel<false>, gw, b, 0, s, rows, ts_word, n_views, (const uint64_t*)cur, other);
    hipLaunchKernelGGL(sky_morph_kernel<true>, gw, b, 0, s, rows, ts_word, n_views, (const uint64_t*)other, cur);
    hipLaunchKernelGGL(sky_morph_kernel<false>, gw, b, 0, s, rows, ts_word, n_views, (const uint64_t*)cur, other);
    std::swap(cur, other);
  }
  if (bits_out && hipMemcpyAsync(bits_out, cur, (size_t)total_words * 8, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return f3r_check_launch("f3r_sky_detect");
  if (stages & F3R_SKY_LABEL) {
    if (hipMemsetAsync(stats, 0, (size_t)n_views * 5 * sizeof(int32_t), s) != hipSuccess) return f3r_check_launch("f3r_sky_detect");
    if (hipMemsetAsync(top_size, 0, (size_t)total_width * sizeof(int32_t), s) != hipSuccess) return f3r_check_launch("f3r_sky_detect");
    hipLaunchKernelGGL(sky_init_kernel, gp, b, 0, s, rows, ts_pix, n_views, (const uint64_t*)cur, parent);
    hipLaunchKernelGGL(sky_merge_kernel, gw, b, 0, s, rows, ts_word, n_views, (const uint64_t*)cur, parent);
    hipLaunchKernelGGL(sky_flatten_kernel, gp, b, 0, s, rows, ts_pix, n_views, (const uint64_t*)cur, parent, top_size, stats);
    hipLaunchKernelGGL(sky_apply_kernel, gp, b, 0, s, rows, ts_pix, n_views, (const uint64_t*)cur, (const int32_t*)parent,
                       (const int32_t*)top_size, stats);
  }
  return f3r_check_launch("f3r_sky_detect");
}
