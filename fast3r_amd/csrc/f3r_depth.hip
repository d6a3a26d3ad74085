// Multi-view depth metrics (include/f3r.h "multi-view depth metrics"): what the reference's scripts/robustmvd_eval.py obtains from an
// external benchmark library per sample on the host -- median alignment, absolute relative error, inlier ratios, sparsification curves and
// their area -- for all (view, sample) segments of a forward pass at once, on tensors that stay where they lie.
//   medians   one workgroup per segment: the confidence threshold (block_quantile), the count of valid pixels, and the medians of the
//             ground truth and of the prediction over the valid pixels by radix select over masked keys; the scale
//   errors    one workgroup per tile of 1024 pixels: 16-byte loads where the segment's pointers allow them, fp64 terms, one partial per
//             tile; finish: one workgroup per segment adds its tiles' partials in a fixed order
//   sparsify  valid pixels per tile, one scan, a ballot compaction of (segment << 32 | key, pixel) in pixel order, the stable LSD sort of
//             f3r_sort.h, once by confidence and once by descending error; per (segment, order, bin) one workgroup sums its bin; one
//             workgroup per segment turns the bin sums into the two curves (suffix sums of bin sums, never total - prefix) and their area
// All arithmetic is fp64 on exactly widened fp32 inputs.  Sums follow the order contract of f3r_prims.h: accumulators start at +0.0, no
// floating-point atomics, so two runs give the same bits.  Inputs are never written to.  Built with -ffp-contract=off.
#include <math.h>

#include "f3r_common.h"
#include "f3r_post_common.h"
#include "f3r_sort.h"

namespace {

constexpr int TILE = 1024;          // pixels of one workgroup of the error and compaction kernels
constexpr int ERR_NT = 256;
constexpr int PX = TILE / ERR_NT;   // consecutive pixels of one thread of the error kernel: 16 bytes of depth, 48 of pointmap
constexpr int MED_NT = 1024;
constexpr int NP = 6;               // partials of a tile: sum e, sum (sp - g)^2, the four inlier counts
constexpr int ROW = 8;              // words of a table row
constexpr int COLS = 16;            // fixed columns of a result row; the curves follow
constexpr int MAX_BINS = 1 << 16;
static_assert(TILE == F3R_DEPTH_TILE && ROW == F3R_DEPTH_ROW_WORDS && COLS == F3R_DEPTH_OUT_WORDS && PX == 4 && NP == 2 + F3R_DEPTH_MAX_THRESHOLDS,
              "include/f3r.h states the layout");
enum { C_N = 0, C_THR = 1, C_MED_G = 2, C_MED_P = 3, C_SCALE = 4, C_ABSREL = 5, C_RMSE = 6, C_INL = 7, C_CNT = 11, C_AUSE = 15 };

struct DepthRow {  // one row of the device table, 8 x 8 bytes
  const float* g;       // ground-truth depth, n fp32
  const float* p;       // prediction: a depth map (stride 1) or a pointmap (stride 3, channel 2)
  int64_t p_stride, p_chan;
  const float* conf;    // n fp32, or null
  const uint8_t* mask;  // n bytes, nonzero = valid, or null
  int64_t n;            // pixels
  int64_t base;         // pixels of the segments before
};
static_assert(sizeof(DepthRow) == ROW * 8, "include/f3r.h states the row layout");

struct Params {
  int n_seg, use_thr, clip, n_thr, n_bins, median;
  float q;
  int64_t out_ld;
  double lo, hi, t[F3R_DEPTH_MAX_THRESHOLDS];
};

__device__ __forceinline__ bool finite_f(float v) { return (__builtin_bit_cast(uint32_t, v) & 0x7f800000u) != 0x7f800000u; }

// the one statement of "valid": g > 0, g and p finite, the mask, conf >= thr (a NaN confidence fails)
__device__ __forceinline__ bool valid_values(float g, float p, bool m, bool use_thr, float c, float thr) {
  return g > 0.f && finite_f(g) && finite_f(p) && m && (!use_thr || c >= thr);
}

__device__ __forceinline__ bool valid_at(const DepthRow& r, bool use_thr, float thr, int64_t i) {
  return valid_values(r.g[i], r.p[i * r.p_stride + r.p_chan], !r.mask || r.mask[i] != 0, use_thr, use_thr ? r.conf[i] : 0.f, thr);
}

// e = |sp - g| / g and the aligned, clipped prediction sp
__device__ __forceinline__ double rel_error(const Params& P, double s, float g, float p, double& sp, double& d) {
  sp = s * (double)p;
  if (P.clip) sp = fmin(fmax(sp, P.lo), P.hi);
  d = sp - (double)g;
  return fabs(d) / (double)g;
}

// ---------------------------------------------------------------------------------------------------------------------------
// medians
__global__ __launch_bounds__(MED_NT) void depth_median_kernel(const DepthRow* __restrict__ rows, Params P, double* __restrict__ out) {
  __shared__ uint32_t hist[2048];
  __shared__ int64_t sh_i64[2];
  __shared__ float sh_thr;
  __shared__ uint32_t sh_cnt;
  const DepthRow r = rows[blockIdx.x];
  const bool use_thr = P.use_thr && r.conf;
  float thr = __builtin_nanf("");
  if (use_thr) thr = block_quantile<MED_NT>(r.conf, r.n, P.q, hist, sh_i64, &sh_thr);
  if (threadIdx.x == 0) sh_cnt = 0;
  __syncthreads();
  uint32_t c = 0;
  for (int64_t i = threadIdx.x; i < r.n; i += MED_NT) c += valid_at(r, use_thr, thr, i) ? 1u : 0u;
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&sh_cnt, c);
  __syncthreads();
  const int64_t n = sh_cnt;
  double med_g = __builtin_nan(""), med_p = med_g, s = med_g;
  if (n > 0) {
    // invalid pixels read as the largest key (a valid value is finite: its key is smaller), and the ranks come from n
    const auto key_g = [&](int64_t i) { return valid_at(r, use_thr, thr, i) ? fkey(r.g[i]) : 0xffffffffu; };
    const auto key_p = [&](int64_t i) { return valid_at(r, use_thr, thr, i) ? fkey(r.p[i * r.p_stride + r.p_chan]) : 0xffffffffu; };
    const int64_t k_lo = (n - 1) / 2, k_hi = n / 2;
    float a = fkey_inv(select_kth_key<MED_NT>(key_g, r.n, k_lo, hist, sh_i64)), b = a;
    if (k_hi != k_lo) b = fkey_inv(select_kth_key<MED_NT>(key_g, r.n, k_hi, hist, sh_i64));
    med_g = ((double)a + (double)b) / 2.0;
    a = b = fkey_inv(select_kth_key<MED_NT>(key_p, r.n, k_lo, hist, sh_i64));
    if (k_hi != k_lo) b = fkey_inv(select_kth_key<MED_NT>(key_p, r.n, k_hi, hist, sh_i64));
    med_p = ((double)a + (double)b) / 2.0;
    s = 1.0;
    if (P.median) {
      s = med_g / med_p;
      if (!(fabs(s) < __builtin_inf())) s = 1.0;  // 0 / 0, x / 0
    }
  }
  if (threadIdx.x == 0) {
    double* o = out + (int64_t)blockIdx.x * P.out_ld;
    o[C_N] = (double)n;
    o[C_THR] = (double)thr;
    o[C_MED_G] = med_g;
    o[C_MED_P] = med_p;
    o[C_SCALE] = s;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// errors
__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

__global__ __launch_bounds__(ERR_NT) void depth_error_kernel(const DepthRow* __restrict__ rows, const int64_t* __restrict__ ts, Params P,
                                                             const double* __restrict__ out, double* __restrict__ part) {
  __shared__ double red[ERR_NT / 64][NP];
  const int seg = last_le(ts, 0, P.n_seg, (int64_t)blockIdx.x);
  const DepthRow r = rows[seg];
  const double* o = out + (int64_t)seg * P.out_ld;
  const bool use_thr = P.use_thr && r.conf;
  const float thr = (float)o[C_THR];
  const double s = o[C_SCALE];
  const int64_t i0 = ((int64_t)blockIdx.x - ts[seg]) * TILE + (int64_t)threadIdx.x * PX;
  float g[PX], p[PX], c[PX];
  bool m[PX], in[PX];
  const bool full = i0 + PX <= r.n;
#pragma unroll
  for (int j = 0; j < PX; ++j) {
    in[j] = i0 + j < r.n;
    c[j] = 0.f;
    m[j] = true;
  }
  // a tile starts 4096 bytes into its segment, so the segment's base pointers decide: 16-byte loads, or scalar ones at odd bases and ends
  if (full && aligned16(r.g)) {
    const float4v v = *(const float4v*)(r.g + i0);
#pragma unroll
    for (int j = 0; j < PX; ++j) g[j] = v[j];
  } else {
#pragma unroll
    for (int j = 0; j < PX; ++j) g[j] = in[j] ? r.g[i0 + j] : 0.f;
  }
  if (full && aligned16(r.p) && r.p_stride == 3) {  // twelve floats: the pixels' channel p_chan sits at 3 j + p_chan
    const float4v* q = (const float4v*)(r.p + i0 * 3);
    const float4v v0 = q[0], v1 = q[1], v2 = q[2];
    float w[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      w[j] = v0[j];
      w[4 + j] = v1[j];
      w[8 + j] = v2[j];
    }
#pragma unroll
    for (int j = 0; j < PX; ++j) p[j] = r.p_chan == 2 ? w[3 * j + 2] : r.p_chan == 1 ? w[3 * j + 1] : w[3 * j];
  } else if (full && aligned16(r.p) && r.p_stride == 1) {
    const float4v v = *(const float4v*)(r.p + i0);
#pragma unroll
    for (int j = 0; j < PX; ++j) p[j] = v[j];
  } else {
#pragma unroll
    for (int j = 0; j < PX; ++j) p[j] = in[j] ? r.p[(i0 + j) * r.p_stride + r.p_chan] : 0.f;
  }
  if (use_thr) {
    if (full && aligned16(r.conf)) {
      const float4v v = *(const float4v*)(r.conf + i0);
#pragma unroll
      for (int j = 0; j < PX; ++j) c[j] = v[j];
    } else {
#pragma unroll
      for (int j = 0; j < PX; ++j) c[j] = in[j] ? r.conf[i0 + j] : 0.f;
    }
  }
  if (r.mask) {
    if (full && ((uintptr_t)r.mask & 3u) == 0) {
      const uint32_t v = *(const uint32_t*)(r.mask + i0);
#pragma unroll
      for (int j = 0; j < PX; ++j) m[j] = ((v >> (8 * j)) & 255u) != 0;
    } else {
#pragma unroll
      for (int j = 0; j < PX; ++j) m[j] = in[j] && r.mask[i0 + j] != 0;
    }
  }
  double acc[NP] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int j = 0; j < PX; ++j) {
    if (in[j] && valid_values(g[j], p[j], m[j], use_thr, c[j], thr)) {
      double sp, d;
      const double e = rel_error(P, s, g[j], p[j], sp, d);
      const double ra = (double)g[j] / sp, rb = sp / (double)g[j];
      const double ratio = (ra >= rb || ra != ra) ? ra : rb;  // the maximum that keeps a NaN, as numpy's
      acc[0] += e;
      acc[1] += d * d;
#pragma unroll
      for (int t = 0; t < F3R_DEPTH_MAX_THRESHOLDS; ++t)
        if (t < P.n_thr && ratio < P.t[t]) acc[2 + t] += 1.0;
    }
  }
  block_sum<NP, ERR_NT, NP>(acc, red, part + (int64_t)blockIdx.x * NP);
}

__global__ __launch_bounds__(ERR_NT) void depth_finish_kernel(const int64_t* __restrict__ ts, Params P, const double* __restrict__ part,
                                                              double* __restrict__ out) {
  __shared__ double red[ERR_NT / 64][NP];
  __shared__ double tot[NP];
  const int64_t t0 = ts[blockIdx.x], t1 = ts[blockIdx.x + 1];
  double acc[NP] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t t = t0 + threadIdx.x; t < t1; t += ERR_NT) {
#pragma unroll
    for (int j = 0; j < NP; ++j) acc[j] += part[t * NP + j];
  }
  block_sum<NP, ERR_NT, NP>(acc, red, tot);
  if (threadIdx.x == 0) {
    double* o = out + (int64_t)blockIdx.x * P.out_ld;
    const double n = o[C_N], nan = __builtin_nan("");
    o[C_ABSREL] = n > 0 ? 100.0 * tot[0] / n : nan;
    o[C_RMSE] = n > 0 ? sqrt(tot[1] / n) : nan;
    for (int t = 0; t < F3R_DEPTH_MAX_THRESHOLDS; ++t) {
      o[C_INL + t] = (n > 0 && t < P.n_thr) ? 100.0 * tot[2 + t] / n : nan;
      o[C_CNT + t] = t < P.n_thr ? tot[2 + t] : nan;
    }
    o[C_AUSE] = nan;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// sparsification
// cnt[tile] = valid pixels of the tile (n_tiles + 1 words; the last is zeroed for the scan's total)
__global__ __launch_bounds__(64) void depth_count_kernel(const DepthRow* __restrict__ rows, const int64_t* __restrict__ ts, Params P,
                                                         const double* __restrict__ out, uint32_t* __restrict__ cnt, int64_t n_tiles) {
  const int seg = last_le(ts, 0, P.n_seg, (int64_t)blockIdx.x);
  const DepthRow r = rows[seg];
  const bool use_thr = P.use_thr && r.conf;
  const float thr = (float)out[(int64_t)seg * P.out_ld + C_THR];
  uint32_t c[1];
  tile_count<TILE>(((int64_t)blockIdx.x - ts[seg]) * TILE, r.n, [&](int64_t i) { return valid_at(r, use_thr, thr, i); }, c);
  if (threadIdx.x == 0) {
    cnt[blockIdx.x] = c[0];
    if (blockIdx.x == 0) cnt[n_tiles] = 0;
  }
}

// the valid pixels of the tile, in pixel order, at the scanned slots: key = segment << 32 | (by_error ? the inverted key of e rounded to fp32
// : the key of the confidence), value = the pixel's index in its segment.  by_error also leaves e at err[base + pixel].
__global__ __launch_bounds__(64) void depth_compact_kernel(const DepthRow* __restrict__ rows, const int64_t* __restrict__ ts, Params P,
                                                           const double* __restrict__ out, const uint32_t* __restrict__ scan, int by_error,
                                                           double* __restrict__ err, uint64_t* __restrict__ keys, uint32_t* __restrict__ idx) {
  const int seg = last_le(ts, 0, P.n_seg, (int64_t)blockIdx.x);
  const DepthRow r = rows[seg];
  const double* o = out + (int64_t)seg * P.out_ld;
  const bool use_thr = P.use_thr && r.conf;
  const float thr = (float)o[C_THR];
  const double s = o[C_SCALE];
  uint32_t run[1] = {scan[blockIdx.x]};
  tile_compact<TILE>(
      ((int64_t)blockIdx.x - ts[seg]) * TILE, r.n, run, [&](int64_t i) { return valid_at(r, use_thr, thr, i); },
      [&](int64_t i, uint32_t, const uint32_t(&slot)[1]) {
        uint32_t key;
        if (by_error) {
          double sp, d;
          const double e = rel_error(P, s, r.g[i], r.p[i * r.p_stride + r.p_chan], sp, d);
          err[r.base + i] = e;
          key = ~fkey((float)e);  // descending e
        } else {
          key = r.conf ? fkey(r.conf[i]) : 0u;
        }
        keys[slot[0]] = ((uint64_t)seg << 32) | key;
        idx[slot[0]] = (uint32_t)i;
      });
}

// the slots past the valid pixels hold the largest key: a stable sort leaves them where they are, after every segment
__global__ __launch_bounds__(256) void depth_pad_kernel(const uint32_t* __restrict__ scan, int64_t n_tiles, int64_t total, uint64_t* __restrict__ keys,
                                                        uint32_t* __restrict__ idx) {
  for (int64_t i = (int64_t)scan[n_tiles] + (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    keys[i] = ~0ull;
    idx[i] = 0u;
  }
}

__global__ __launch_bounds__(256) void depth_starts_kernel(const int64_t* __restrict__ ts, int n_seg, const uint32_t* __restrict__ scan,
                                                           uint32_t* __restrict__ starts) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s <= n_seg) starts[s] = scan[ts[s]];
}

// workgroup (segment, order, bin): the sum of e over the bin's run [n k / K, n (k + 1) / K) of the order
__global__ __launch_bounds__(ERR_NT) void depth_bin_kernel(const DepthRow* __restrict__ rows, Params P, const uint32_t* __restrict__ starts,
                                                           const uint32_t* __restrict__ order_conf, const uint32_t* __restrict__ order_err,
                                                           const double* __restrict__ err, double* __restrict__ bins) {
  __shared__ double red[ERR_NT / 64][1];
  const int64_t K = P.n_bins;
  const int64_t k = blockIdx.x % K, so = blockIdx.x / K, seg = so >> 1;
  const uint32_t* order = (so & 1) ? order_err : order_conf;
  const int64_t start = starts[seg], n = (int64_t)starts[seg + 1] - start;
  const int64_t r0 = n * k / K, r1 = n * (k + 1) / K;
  const double* e = err + rows[seg].base;
  double acc = 0.0;
  for (int64_t q = r0 + threadIdx.x; q < r1; q += ERR_NT) acc += e[order[start + q]];
  block_sum<1, ERR_NT, 1>(&acc, red, bins + blockIdx.x);
}

// one workgroup per segment: thread 0 the sparsification curve, thread 1 the oracle curve (means of the kept pixels from suffix sums of the
// bin sums, last bin first), then thread 0 the area between them
__global__ __launch_bounds__(64) void depth_curve_kernel(Params P, const uint32_t* __restrict__ starts, const double* __restrict__ bins,
                                                         double* __restrict__ out) {
  const int64_t K = P.n_bins;
  const int seg = blockIdx.x;
  double* o = out + (int64_t)seg * P.out_ld;
  const int64_t n = (int64_t)starts[seg + 1] - (int64_t)starts[seg];
  const double nan = __builtin_nan("");
  if (threadIdx.x < 2) {
    const double* b = bins + ((int64_t)seg * 2 + threadIdx.x) * K;
    double* curve = o + COLS + threadIdx.x * K;
    double acc = 0.0;
    for (int64_t k = K - 1; k >= 0; --k) {
      acc += b[k];
      curve[k] = n > 0 ? acc / (double)(n - n * k / K) : nan;
    }
  }
  __threadfence_block();
  __syncthreads();
  if (threadIdx.x == 0) {
    const double* sc = o + COLS;
    const double* oc = sc + K;
    double a = nan;
    if (n > 0) {
      a = 0.0;
      const double s0 = sc[0];
      if (s0 != 0.0)
        for (int64_t k = 0; k + 1 < K; ++k) a += ((sc[k] - oc[k]) / s0 + (sc[k + 1] - oc[k + 1]) / s0) / (2.0 * (double)K);
    }
    o[C_AUSE] = a;
  }
}

// ---- host
struct DepthWs {
  double *part, *err, *bins;
  uint32_t* scan;
  SortWs<> sort;
  size_t bytes;
};

DepthWs depth_ws(void* base, int n_seg, int64_t n_tiles, int64_t total, int uncertainty, int n_bins) {
  Carve c(base, 256);
  DepthWs w = {};
  w.part = c.take<double>((size_t)n_tiles * NP);
  if (uncertainty) {
    w.scan = c.take<uint32_t>((size_t)n_tiles + 1);
    w.err = c.take<double>((size_t)total);
    w.bins = c.take<double>((size_t)n_seg * 2 * (size_t)n_bins);
    w.sort = sort_ws(c, total);
  }
  w.bytes = c.bytes();
  return w;
}

// the host copy of the table says what the device copy holds: rows, then the n_seg + 1 tile starts
const char* table_fault(const int64_t* host, int n_seg, int64_t n_tiles, int64_t* total) {
  int64_t base = 0, tiles = 0;
  for (int s = 0; s < n_seg; ++s) {
    const int64_t* r = host + (int64_t)s * ROW;
    if (!r[0] || !r[1]) return "a null depth or prediction pointer";
    if (!((r[2] == 1 && r[3] == 0) || (r[2] == 3 && r[3] >= 0 && r[3] < 3))) return "a prediction stride that is neither 1 nor 3";
    if ((r[0] | r[1] | r[4]) & 3) return "a pointer that is not a multiple of 4 bytes";
    if (r[6] < 1 || r[6] >= (1ll << 31)) return "a segment of fewer than 1 or of 2^31 pixels or more";
    if (r[7] != base) return "a pixel base that is not the sum of the sizes before";
    if (host[(int64_t)n_seg * ROW + s] != tiles) return "tile starts that are not the segments' tile counts";
    base += r[6];
    tiles += (r[6] + TILE - 1) / TILE;
  }
  if (host[(int64_t)n_seg * ROW + n_seg] != tiles || tiles != n_tiles) return "tile starts that are not the segments' tile counts";
  *total = base;
  return nullptr;
}

bool fill_params(Params* P, int n_seg, int use_thr, int clip, double lo, double hi, const double* thresholds, int n_thr, int n_bins, int64_t out_ld) {
  *P = Params{};
  P->n_seg = n_seg;
  P->use_thr = use_thr ? 1 : 0;
  P->clip = clip ? 1 : 0;
  P->lo = lo;
  P->hi = hi;
  P->n_thr = n_thr;
  for (int t = 0; t < n_thr; ++t) P->t[t] = thresholds[t];
  P->n_bins = n_bins;
  P->out_ld = out_ld;
  return !clip || lo <= hi;  // false for a NaN bound too
}

}  // namespace

extern "C" size_t f3r_depth_workspace_bytes(int n_seg, int64_t n_tiles, int64_t total_pixels, int eval_uncertainty, int n_bins) {
  if (n_seg < 1 || n_tiles < n_seg || n_tiles >= (1ll << 31) || total_pixels < n_seg) return 0;
  if (eval_uncertainty && (n_bins < 1 || n_bins > MAX_BINS || total_pixels >= (1ll << 31))) return 0;
  return depth_ws(nullptr, n_seg, n_tiles, total_pixels, eval_uncertainty, n_bins).bytes;
}

#define DEPTH_COMMON(who)                                                                                                                  \
  F3R_REQUIRE(table && host_table, who ": null table or host_table");                                                                      \
  F3R_REQUIRE(out, who ": null out");                                                                                                      \
  F3R_REQUIRE(n_seg >= 1 && n_seg <= (1 << 24) && n_tiles >= n_seg && n_tiles < (1ll << 31),                                               \
              who ": %d segments, %lld tiles; need 1 <= segments <= 2^24 and one tile per segment at least", n_seg, (long long)n_tiles);  \
  int64_t total = 0;                                                                                                                       \
  {                                                                                                                                        \
    const char* fault = table_fault(host_table, n_seg, n_tiles, &total);                                                                   \
    F3R_REQUIRE(!fault, who ": the table holds %s", fault);                                                                                \
  }

extern "C" int f3r_depth_medians(const int64_t* table, const int64_t* host_table, int n_seg, int64_t n_tiles, int alignment, int use_thr, float q,
                                 double* out, int64_t out_ld, f3r_stream_t stream) {
  DEPTH_COMMON("f3r_depth_medians")
  F3R_REQUIRE(out_ld >= COLS, "f3r_depth_medians: out_ld = %lld; a result row has %d words at least", (long long)out_ld, COLS);
  F3R_REQUIRE(alignment == F3R_DEPTH_ALIGN_NONE || alignment == F3R_DEPTH_ALIGN_MEDIAN, "f3r_depth_medians: unknown alignment %d", alignment);
  F3R_REQUIRE(!use_thr || (q >= 0.f && q <= 1.f), "f3r_depth_medians: q = %g outside [0, 1]", (double)q);
  Params P;
  fill_params(&P, n_seg, use_thr, 0, 0.0, 0.0, nullptr, 0, 0, out_ld);
  P.median = alignment == F3R_DEPTH_ALIGN_MEDIAN;
  P.q = q;
  hipLaunchKernelGGL(depth_median_kernel, dim3((unsigned)n_seg), dim3(MED_NT), 0, (hipStream_t)stream, (const DepthRow*)table, P, out);
  return f3r_check_launch("f3r_depth_medians");
}

extern "C" int f3r_depth_errors(const int64_t* table, const int64_t* host_table, int n_seg, int64_t n_tiles, int use_thr, int clip, double clip_lo,
                                double clip_hi, const double* thresholds, int n_thresholds, void* workspace, size_t workspace_bytes, double* out,
                                int64_t out_ld, f3r_stream_t stream) {
  DEPTH_COMMON("f3r_depth_errors")
  F3R_REQUIRE(workspace, "f3r_depth_errors: null workspace");
  F3R_REQUIRE(out_ld >= COLS, "f3r_depth_errors: out_ld = %lld; a result row has %d words at least", (long long)out_ld, COLS);
  F3R_REQUIRE(n_thresholds >= 0 && n_thresholds <= F3R_DEPTH_MAX_THRESHOLDS && (thresholds || !n_thresholds),
              "f3r_depth_errors: %d thresholds; at most %d, with their array", n_thresholds, F3R_DEPTH_MAX_THRESHOLDS);
  Params P;
  F3R_REQUIRE(fill_params(&P, n_seg, use_thr, clip, clip_lo, clip_hi, thresholds, n_thresholds, 0, out_ld),
              "f3r_depth_errors: clip bounds (%g, %g) are not an interval", clip_lo, clip_hi);
  const DepthWs w = depth_ws(workspace, n_seg, n_tiles, total, 0, 0);
  F3R_REQUIRE(workspace_bytes >= w.bytes, "f3r_depth_errors: workspace too small (%zu bytes; need %zu)", workspace_bytes, w.bytes);
  hipStream_t s = (hipStream_t)stream;
  const DepthRow* rows = (const DepthRow*)table;
  const int64_t* ts = table + (int64_t)n_seg * ROW;
  hipLaunchKernelGGL(depth_error_kernel, dim3((unsigned)n_tiles), dim3(ERR_NT), 0, s, rows, ts, P, (const double*)out, w.part);
  hipLaunchKernelGGL(depth_finish_kernel, dim3((unsigned)n_seg), dim3(ERR_NT), 0, s, ts, P, (const double*)w.part, out);
  return f3r_check_launch("f3r_depth_errors");
}

extern "C" int f3r_depth_sparsify(const int64_t* table, const int64_t* host_table, int n_seg, int64_t n_tiles, int use_thr, int clip, double clip_lo,
                                  double clip_hi, int n_bins, void* workspace, size_t workspace_bytes, uint32_t* order_conf, uint32_t* order_err,
                                  uint32_t* starts, double* out, int64_t out_ld, f3r_stream_t stream) {
  DEPTH_COMMON("f3r_depth_sparsify")
  F3R_REQUIRE(workspace && order_conf && order_err && starts, "f3r_depth_sparsify: null workspace, order or starts");
  F3R_REQUIRE(n_bins >= 1 && n_bins <= MAX_BINS, "f3r_depth_sparsify: n_bins = %d outside [1, %d]", n_bins, MAX_BINS);
  F3R_REQUIRE(total < (1ll << 31), "f3r_depth_sparsify: %lld pixels in all; the sort takes fewer than 2^31", (long long)total);
  F3R_REQUIRE((int64_t)n_seg * 2 * n_bins < (1ll << 31), "f3r_depth_sparsify: %d segments x %d bins; need fewer than 2^30 bins in all", n_seg, n_bins);
  F3R_REQUIRE(out_ld >= COLS + 2 * (int64_t)n_bins, "f3r_depth_sparsify: out_ld = %lld; a result row with curves has %lld words", (long long)out_ld,
              (long long)(COLS + 2 * (int64_t)n_bins));
  Params P;
  F3R_REQUIRE(fill_params(&P, n_seg, use_thr, clip, clip_lo, clip_hi, nullptr, 0, n_bins, out_ld),
              "f3r_depth_sparsify: clip bounds (%g, %g) are not an interval", clip_lo, clip_hi);
  const DepthWs w = depth_ws(workspace, n_seg, n_tiles, total, 1, n_bins);
  F3R_REQUIRE(workspace_bytes >= w.bytes, "f3r_depth_sparsify: workspace too small (%zu bytes; need %zu)", workspace_bytes, w.bytes);
  hipStream_t s = (hipStream_t)stream;
  const DepthRow* rows = (const DepthRow*)table;
  const int64_t* ts = table + (int64_t)n_seg * ROW;
  const dim3 gt((unsigned)n_tiles), bt(64);
  hipLaunchKernelGGL(depth_count_kernel, gt, bt, 0, s, rows, ts, P, (const double*)out, w.scan, n_tiles);
  hipLaunchKernelGGL(exclusive_scan_rows_kernel<SCAN_NT>, dim3(1), dim3(SCAN_NT), 0, s, w.scan, (const int64_t*)nullptr, n_tiles + 1,
                     (uint32_t*)nullptr);
  hipLaunchKernelGGL(depth_starts_kernel, dim3(blocks_of(n_seg + 1, 256)), dim3(256), 0, s, ts, n_seg, (const uint32_t*)w.scan, starts);
  int seg_bits = 0;  // the key's bits above the 32 of the value key: the segment number
  while (seg_bits < 31 && (1ll << seg_bits) < n_seg) ++seg_bits;
  const int passes = (32 + seg_bits + 7) / 8;
  const unsigned pad_grid = (unsigned)std::min<int64_t>(blocks_of(total, 256), 1024);
  for (int by_error = 0; by_error < 2; ++by_error) {
    hipLaunchKernelGGL(depth_compact_kernel, gt, bt, 0, s, rows, ts, P, (const double*)out, (const uint32_t*)w.scan, by_error, w.err,
                       w.sort.keys_a, w.sort.idx_a);
    hipLaunchKernelGGL(depth_pad_kernel, dim3(pad_grid), dim3(256), 0, s, (const uint32_t*)w.scan, n_tiles, total, w.sort.keys_a, w.sort.idx_a);
    const uint64_t* keys;
    const uint32_t* values;
    sort_pairs_lsd(w.sort, total, passes, s, &keys, &values);
    if (hipMemcpyAsync(by_error ? order_err : order_conf, values, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToDevice, s) != hipSuccess) {
      (void)hipGetLastError();
      f3r_set_error("f3r_depth_sparsify: copying the sorted order failed");
      return F3R_ERR_LAUNCH;
    }
  }
  hipLaunchKernelGGL(depth_bin_kernel, dim3((unsigned)((int64_t)n_seg * 2 * n_bins)), dim3(ERR_NT), 0, s, rows, P, (const uint32_t*)starts,
                     (const uint32_t*)order_conf, (const uint32_t*)order_err, (const double*)w.err, w.bins);
  hipLaunchKernelGGL(depth_curve_kernel, dim3((unsigned)n_seg), dim3(64), 0, s, P, (const uint32_t*)starts, (const double*)w.bins, out);
  return f3r_check_launch("f3r_depth_sparsify");
}
