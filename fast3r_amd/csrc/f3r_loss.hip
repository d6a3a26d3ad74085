// The multi-view confidence loss of validation (include/f3r.h: f3r_mv_conf_loss): ConfLossMultiviewV2 around Regr3DMultiviewV3 / V4 with
// L21Loss (fast3r/dust3r/losses.py:404-848), forward only.  The reference concatenates all views twice, writes NaN over the invalid pixels,
// gathers `pts[valid_mask]` four times per view and runs one geotrf einsum per view and frame; here nothing is stacked, concatenated or
// compacted: two streaming passes read the per-view tensors where they lie, through device tables of pointers.
//   setup    one thread per (view, sample): general 4 x 4 inverse of the pose in fp64; one thread: the tile prefix over the segments
//   pass A   per (view, sample) and set (global / local): counts and the sums of f(|gt|), f(|pred|) over the valid pixels
//   factors  the normalisation factors of V3 / V4 from the moments, on the device
//   pass B   L = |pred / n_pred - gt / n_gt| and L conf - alpha log conf, summed per (view, sample) and set
//   finish   per-view means, the empty-view rules and the total
// A segment is one (view, sample), s = view * n_samples + sample, cut into tiles of 1024 pixels; workgroup k of nb takes the tiles
// [k T / nb, (k + 1) T / nb) of the segment-major tile order, so it meets a contiguous run of segments and writes one partial per segment it
// meets, at slot k + s (the (k, s) pairs met form a monotone staircase, so k + s is unique).  Partials are summed in slot order: no
// floating-point atomics, and the result is the same bits from run to run.  All arithmetic is fp64 on the exactly widened fp32 inputs.
// Built with -ffp-contract=off: every fp64 product rounds on its own.
#include <math.h>

#include "f3r_common.h"
#include "f3r_prims.h"

namespace {

constexpr int THREADS = 256;
constexpr int PX = 4;                 // consecutive pixels per thread: 3 x 16 B of points, 16 B of confidence, 4 B of mask
constexpr int TILE = THREADS * PX;    // pixels per tile
constexpr int MAX_BLOCKS = 2048;      // the grid is min(4 x CUs, MAX_BLOCKS); the workspace is sized for MAX_BLOCKS
constexpr int NA = 10;                // pass A moments per segment: per set { valid, non-NaN gt, sum gt, non-NaN pred, sum pred }
constexpr int NB = 4;                 // pass B sums per segment: per set { sum L, sum (L conf - alpha log conf) }
constexpr int WAVES = THREADS / 64;

struct Tables {
  const float* const* gt;
  const uint8_t* const* valid;
  const void* const* pose;
  const float* const* pred;
  const float* const* conf;
  const float* const* pred_l;  // null: no local head
  const float* const* conf_l;
  const int64_t* npix;
};

struct Work {
  double* inv;        // [nseg][12]: top three rows of inv(pose)
  long long* tile0;   // [nseg + 1]: first tile of every segment; tile0[nseg] = T
  double* mom_a;      // [nseg][NA]
  double* fac;        // [4][nseg]: pred-global, gt-global, pred-local, gt-local
  double* part_a;     // [MAX_BLOCKS + nseg][NA]
  double* part_b;     // [MAX_BLOCKS + nseg][NB]
  double* mom_b;      // [nseg][NB]
};

struct Params {
  int n_views, n_samples, nseg;
  int version, log1p_mode, gt_scale, local_scale_consistent, use_clip, pose_f64;
  double clip, alpha;
};

size_t carve(Work* w, void* base, long long nseg) {
  Carve c(base, 8);
  const size_t n = (size_t)nseg, slots = (size_t)MAX_BLOCKS + n;
  double* inv = c.take<double>(12 * n);
  long long* tile0 = c.take<long long>(n + 1);
  double* mom_a = c.take<double>(NA * n);
  double* fac = c.take<double>(4 * n);
  double* part_a = c.take<double>(NA * slots);
  double* part_b = c.take<double>(NB * slots);
  double* mom_b = c.take<double>(NB * n);
  if (w) *w = Work{inv, tile0, mom_a, fac, part_a, part_b, mom_b};
  return c.bytes();
}

// General inverse by Gauss-Jordan elimination with partial pivoting (the reference: torch.linalg.inv on the fp32 matrix).  A singular
// matrix gives inf / NaN entries (the reference raises).
__device__ void invert4(const double* m, double* top3) {
  double a[4][8];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      a[i][j] = m[i * 4 + j];
      a[i][4 + j] = i == j ? 1.0 : 0.0;
    }
  for (int c = 0; c < 4; ++c) {
    int piv = c;
    for (int r = c + 1; r < 4; ++r)
      if (fabs(a[r][c]) > fabs(a[piv][c])) piv = r;
    for (int j = 0; j < 8; ++j) {
      const double t = a[c][j];
      a[c][j] = a[piv][j];
      a[piv][j] = t;
    }
    const double d = a[c][c];
    for (int j = 0; j < 8; ++j) a[c][j] = a[c][j] / d;
    for (int r = 0; r < 4; ++r) {
      if (r == c) continue;
      const double f = a[r][c];
      for (int j = 0; j < 8; ++j) a[r][j] = a[r][j] - f * a[c][j];
    }
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) top3[i * 4 + j] = a[i][4 + j];
}

__global__ __launch_bounds__(THREADS) void loss_setup_kernel(Tables tab, Work w, Params p) {
  const long long s = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (s < p.nseg) {
    const int v = (int)(s / p.n_samples), b = (int)(s % p.n_samples);
    double m[16];
    for (int i = 0; i < 16; ++i) {
      // fp64 poses are rounded to fp32 first, as the reference's .float() does
      m[i] = p.pose_f64 ? (double)(float)((const double*)tab.pose[v])[(long long)b * 16 + i] : (double)((const float*)tab.pose[v])[(long long)b * 16 + i];
    }
    invert4(m, w.inv + s * 12);
  }
  if (s == 0) {
    long long t = 0;
    for (int q = 0; q < p.nseg; ++q) {
      w.tile0[q] = t;
      const long long n = tab.npix[q / p.n_samples];
      if (n > 0) t += (n + TILE - 1) / TILE;
    }
    w.tile0[p.nseg] = t;
  }
}

// workgroup k of nb owns the tiles [first_tile(k), first_tile(k + 1))
__device__ __forceinline__ long long first_tile(long long k, long long T, int nb) { return k * T / nb; }

__device__ inline int block_of_tile(long long t, long long T, int nb) {
  long long k = t * nb / T;
  if (k > nb - 1) k = nb - 1;
  while (k + 1 < nb && first_tile(k + 1, T, nb) <= t) ++k;
  while (k > 0 && first_tile(k, T, nb) > t) --k;
  return (int)k;
}

struct Segment {
  const float *gt, *pred, *conf, *pred_l, *conf_l;
  const uint8_t* valid;
  long long npix;
  double mg[12], ml[12];     // inv(P_anchor, b), inv(P_b, v)
  double fac[4];             // pass B
  bool vec;                  // every base pointer aligned for the 16-byte path
};

template <bool PASS_B>
__device__ inline void load_segment(Segment& g, const Tables& tab, const Work& w, const Params& p, int s) {
  const int v = s / p.n_samples, b = s % p.n_samples;
  const long long n = tab.npix[v];
  g.npix = n;
  g.gt = tab.gt[v] + (long long)b * n * 3;
  g.pred = tab.pred[v] + (long long)b * n * 3;
  g.conf = tab.conf[v] + (long long)b * n;
  g.valid = tab.valid[v] + (long long)b * n;
  g.pred_l = tab.pred_l ? tab.pred_l[v] + (long long)b * n * 3 : nullptr;
  g.conf_l = tab.pred_l ? tab.conf_l[v] + (long long)b * n : nullptr;
  uintptr_t bits = (uintptr_t)g.gt | (uintptr_t)g.pred | (uintptr_t)g.pred_l;
  if (PASS_B) bits |= (uintptr_t)g.conf | (uintptr_t)g.conf_l;
  g.vec = (bits & 15) == 0 && ((uintptr_t)g.valid & 3) == 0;
  for (int i = 0; i < 12; ++i) {
    g.mg[i] = w.inv[(long long)b * 12 + i];  // the anchor is view 0: segment b
    g.ml[i] = w.inv[(long long)s * 12 + i];
  }
  if (PASS_B)
    for (int i = 0; i < 4; ++i) g.fac[i] = w.fac[(long long)i * p.nseg + s];
}

__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

// one pixel, one set (global: m = inverse anchor pose, pr = pts3d_in_other_view; local: m = the view's own inverse pose, pr = pts3d_local)
template <bool PASS_B>
__device__ __forceinline__ void pixel_set(const double* m, const float* x, bool valid, const float* pr, float conf, const Params& p, double n_pred,
                                          double n_gt, double* acc) {
  const double x0 = x[0], x1 = x[1], x2 = x[2];
  // geotrf: the 3 x 3 product, then the translation
  const double g0 = (m[0] * x0 + m[1] * x1 + m[2] * x2) + m[3];
  const double g1 = (m[4] * x0 + m[5] * x1 + m[6] * x2) + m[7];
  const double g2 = (m[8] * x0 + m[9] * x1 + m[10] * x2) + m[11];
  double dg = 0.0;
  if (!PASS_B || p.use_clip) dg = norm3(g0, g1, g2);
  if (!valid || (p.use_clip && !(dg <= p.clip))) return;
  const double p0 = pr[0], p1 = pr[1], p2 = pr[2];
  if (!PASS_B) {
    double fg = dg, fp = norm3(p0, p1, p2);
    if (p.log1p_mode) {
      fg = log1p(fg);
      fp = log1p(fp);
    }
    acc[0] += 1.0;
    if (fg == fg) {
      acc[1] += 1.0;
      acc[2] += fg;
    }
    if (fp == fp) {
      acc[3] += 1.0;
      acc[4] += fp;
    }
  } else {
    const double L = norm3(p0 / n_pred - g0 / n_gt, p1 / n_pred - g1 / n_gt, p2 / n_pred - g2 / n_gt);
    const double c = conf;
    acc[0] += L;
    acc[1] += L * c - p.alpha * log(c);
  }
}

template <bool PASS_B>
__global__ __launch_bounds__(THREADS) void loss_pass_kernel(Tables tab, Work w, Params p) {
  constexpr int N = PASS_B ? NB : NA;
  constexpr int PER_SET = N / 2;
  const int nb = gridDim.x, k = blockIdx.x;
  const long long T = w.tile0[p.nseg];
  const long long ta = first_tile(k, T, nb), tb = first_tile(k + 1, T, nb);
  if (ta >= tb) return;
  double* part = PASS_B ? w.part_b : w.part_a;
  __shared__ double red[WAVES][N];
  double acc[N];
  for (int i = 0; i < N; ++i) acc[i] = 0.0;
  int s = last_le(w.tile0, 0, p.nseg, ta);  // tile0[s] <= ta < tile0[s + 1] (segments without pixels own no tile)
  Segment g;
  load_segment<PASS_B>(g, tab, w, p, s);
  const bool local = tab.pred_l != nullptr;
  for (long long t = ta; t < tb; ++t) {
    if (t >= w.tile0[s + 1]) {
      block_sum<N, THREADS>(acc, red, part + (long long)(k + s) * N);
      for (int i = 0; i < N; ++i) acc[i] = 0.0;
      do ++s; while (t >= w.tile0[s + 1]);
      load_segment<PASS_B>(g, tab, w, p, s);
    }
    const long long q0 = (t - w.tile0[s]) * TILE + (long long)threadIdx.x * PX;
    if (q0 >= g.npix) continue;
    float x[PX * 3], pr[PX * 3], pl[PX * 3], c[PX], cl[PX];
    uint8_t ok[PX];
    const int n = g.npix - q0 < PX ? (int)(g.npix - q0) : PX;
    if (g.vec && n == PX) {
      const float4v* gx = reinterpret_cast<const float4v*>(g.gt + q0 * 3);
      const float4v* px = reinterpret_cast<const float4v*>(g.pred + q0 * 3);
      for (int j = 0; j < 3; ++j) {
        const float4v a = gx[j], bq = px[j];
        for (int e = 0; e < 4; ++e) {
          x[j * 4 + e] = a[e];
          pr[j * 4 + e] = bq[e];
        }
      }
      const uint32_t m4 = *reinterpret_cast<const uint32_t*>(g.valid + q0);
      for (int e = 0; e < PX; ++e) ok[e] = (uint8_t)(m4 >> (8 * e));
      if (PASS_B) {
        const float4v cc = *reinterpret_cast<const float4v*>(g.conf + q0);
        for (int e = 0; e < PX; ++e) c[e] = cc[e];
      }
      if (local) {
        const float4v* lx = reinterpret_cast<const float4v*>(g.pred_l + q0 * 3);
        for (int j = 0; j < 3; ++j) {
          const float4v a = lx[j];
          for (int e = 0; e < 4; ++e) pl[j * 4 + e] = a[e];
        }
        if (PASS_B) {
          const float4v cc = *reinterpret_cast<const float4v*>(g.conf_l + q0);
          for (int e = 0; e < PX; ++e) cl[e] = cc[e];
        }
      }
    } else {
      for (int e = 0; e < PX; ++e) {
        const bool in = e < n;
        ok[e] = in ? g.valid[q0 + e] : 0;
        for (int j = 0; j < 3; ++j) {
          x[e * 3 + j] = in ? g.gt[(q0 + e) * 3 + j] : 0.f;
          pr[e * 3 + j] = in ? g.pred[(q0 + e) * 3 + j] : 0.f;
          pl[e * 3 + j] = in && local ? g.pred_l[(q0 + e) * 3 + j] : 0.f;
        }
        c[e] = in && PASS_B ? g.conf[q0 + e] : 1.f;
        cl[e] = in && PASS_B && local ? g.conf_l[q0 + e] : 1.f;
      }
    }
    for (int e = 0; e < PX; ++e) {
      pixel_set<PASS_B>(g.mg, x + e * 3, ok[e] != 0, pr + e * 3, PASS_B ? c[e] : 1.f, p, g.fac[0], g.fac[1], acc);
      if (local) pixel_set<PASS_B>(g.ml, x + e * 3, ok[e] != 0, pl + e * 3, PASS_B ? cl[e] : 1.f, p, g.fac[2], g.fac[3], acc + PER_SET);
    }
  }
  block_sum<N, THREADS>(acc, red, part + (long long)(k + s) * N);
}

// sums the partials of every segment in slot order: the workgroups from block_of_tile(first tile) to block_of_tile(last tile) that own a tile met it
template <int N>
__device__ inline void gather_partials(const Work& w, const double* part, double* mom, int nseg, int nb) {
  const long long T = w.tile0[nseg];
  for (int s = threadIdx.x; s < nseg; s += THREADS) {
    double sum[N];
    for (int i = 0; i < N; ++i) sum[i] = 0.0;
    const long long t0 = w.tile0[s], t1 = w.tile0[s + 1];
    if (t1 > t0) {
      const int kf = block_of_tile(t0, T, nb), kl = block_of_tile(t1 - 1, T, nb);
      for (int k = kf; k <= kl; ++k) {
        if (first_tile(k, T, nb) >= first_tile(k + 1, T, nb)) continue;  // a workgroup without tiles (T < nb) wrote nothing
        for (int i = 0; i < N; ++i) sum[i] += part[(long long)(k + s) * N + i];
      }
    }
    for (int i = 0; i < N; ++i) mom[(long long)s * N + i] = sum[i];
  }
  __syncthreads();
}

// One factor pair per group of segments { base + j * stride : j < n }, written to every member.  A wave owns a group; lanes stride over the
// members and a shuffle tree adds them: a fixed order.
__device__ inline void group_factors(const double* mom, int set, int n_groups, int base_mul, int stride, int n, const Params& p, double* out_pred,
                                     double* out_gt) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int grp = wave; grp < n_groups; grp += WAVES) {
    double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = lane; j < n; j += 64) {
      const long long s = (long long)grp * base_mul + (long long)j * stride;
      for (int i = 0; i < 5; ++i) m[i] += mom[s * NA + set * 5 + i];
    }
    for (int i = 0; i < 5; ++i)
      m[i] = __shfl(wave_sum(m[i]), 0);  // lane 0's sum, for every lane
    // V4: nanmean, the sum and the count of what is not NaN (0 / 0 = NaN for a sample without valid pixels); V3: mean over the valid pixels,
    // NaN as soon as one of them is NaN.  clip(min = 1e-8) leaves NaN as it is.
    double f_gt = p.version == 4 ? m[2] / m[1] : (m[1] != m[0] ? (double)NAN : m[2] / m[0]);
    double f_pr = p.version == 4 ? m[4] / m[3] : (m[3] != m[0] ? (double)NAN : m[4] / m[0]);
    if (f_gt < 1e-8) f_gt = 1e-8;
    if (f_pr < 1e-8) f_pr = 1e-8;
    if (p.gt_scale) f_gt = 1.0;
    for (int j = lane; j < n; j += 64) {
      const long long s = (long long)grp * base_mul + (long long)j * stride;
      out_pred[s] = f_pr;
      out_gt[s] = f_gt;
    }
  }
}

__global__ __launch_bounds__(THREADS) void loss_factors_kernel(Work w, Params p, int nb, int local) {
  gather_partials<NA>(w, w.part_a, w.mom_a, p.nseg, nb);
  const int V = p.n_views, B = p.n_samples, S = p.nseg;
  double* fac = w.fac;
  if (p.version == 4) {
    group_factors(w.mom_a, 0, B, 1, B, V, p, fac, fac + S);  // per sample over all views
    if (local && !p.local_scale_consistent) group_factors(w.mom_a, 1, S, 1, 1, 1, p, fac + 2 * S, fac + 3 * S);  // per (sample, view)
  } else {
    group_factors(w.mom_a, 0, 1, 0, 1, S, p, fac, fac + S);  // one over the whole batch
    if (local) group_factors(w.mom_a, 1, V, B, 1, B, p, fac + 2 * S, fac + 3 * S);  // per view over the batch
  }
  if (local && p.version == 4 && p.local_scale_consistent) {
    __syncthreads();
    for (int s = threadIdx.x; s < S; s += THREADS) {
      fac[2 * S + s] = fac[s];
      fac[3 * S + s] = fac[S + s];
    }
  }
}

// out: [0] total | pts3d_loss_global [V] | pts3d_loss_local [V] | conf_loss_global [V] | conf_loss_local [V]
__global__ __launch_bounds__(THREADS) void loss_finish_kernel(Work w, Params p, int nb, int local, double* out) {
  gather_partials<NB>(w, w.part_b, w.mom_b, p.nseg, nb);
  const int V = p.n_views, B = p.n_samples;
  for (int v = threadIdx.x; v < V; v += THREADS)
    for (int set = 0; set < 2; ++set) {
      double cnt = 0.0, sum_l = 0.0, sum_c = 0.0;
      if (set == 0 || local)
        for (int b = 0; b < B; ++b) {
          const long long s = (long long)v * B + b;
          cnt += w.mom_a[s * NA + set * 5];
          sum_l += w.mom_b[s * NB + set * 2];
          sum_c += w.mom_b[s * NB + set * 2 + 1];
        }
      // float(empty.mean()) is NaN; the confidence term of an empty view is the reference's literal 0
      out[1 + set * V + v] = sum_l / cnt;
      out[1 + (2 + set) * V + v] = cnt > 0.0 ? sum_c / cnt : 0.0;
    }
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = 0.0;
    const int terms = local ? 2 * V : V;
    for (int i = 0; i < terms; ++i) total += out[1 + 2 * V + i];
    out[0] = total / (double)terms;
  }
}

int num_blocks() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 8) {
    (void)hipGetLastError();
    cus = 256;
  }
  const int nb = cus * 4;
  return nb > MAX_BLOCKS ? MAX_BLOCKS : nb;
}

bool shape_ok(int n_views, int n_samples) { return n_views >= 1 && n_samples >= 1 && (long long)n_views * n_samples <= (1LL << 22); }

}  // namespace

extern "C" size_t f3r_mv_conf_loss_workspace_bytes(int n_views, int n_samples) {
  if (!shape_ok(n_views, n_samples)) return 0;
  return carve(nullptr, nullptr, (long long)n_views * n_samples);
}

extern "C" int f3r_mv_conf_loss(const void* const* gt_pts, const void* const* valid_mask, const void* const* camera_pose, int pose_dtype,
                                const void* const* pred_pts, const void* const* pred_conf, const void* const* pred_pts_local,
                                const void* const* pred_conf_local, const int64_t* n_pixels, int n_views, int n_samples, int version, int dis_mode,
                                int gt_scale, int local_scale_consistent, int use_dist_clip, double dist_clip, double alpha, void* workspace,
                                size_t workspace_bytes, double* out, f3r_stream_t stream) {
  const char* what = "f3r_mv_conf_loss";
  F3R_REQUIRE(n_views >= 1, "%s: n_views = %d, need at least one view", what, n_views);
  F3R_REQUIRE(n_samples >= 1, "%s: n_samples = %d, need at least one sample", what, n_samples);
  F3R_REQUIRE(shape_ok(n_views, n_samples), "%s: n_views * n_samples = %lld exceeds 2^22", what, (long long)n_views * n_samples);
  F3R_REQUIRE(gt_pts && valid_mask && camera_pose && pred_pts && pred_conf && n_pixels, "%s: null table (gt_pts / valid_mask / camera_pose / pred_pts / "
              "pred_conf / n_pixels)", what);
  F3R_REQUIRE(!(pred_conf_local && !pred_pts_local), "%s: a local confidence table without a local points table", what);
  F3R_REQUIRE(!(pred_pts_local && !pred_conf_local), "%s: a local points table without a local confidence table", what);
  F3R_REQUIRE(alpha > 0.0, "%s: alpha = %g must be positive", what, alpha);
  F3R_REQUIRE(version == 3 || version == 4, "%s: unknown mode: version = %d is neither 3 (Regr3DMultiviewV3) nor 4 (Regr3DMultiviewV4)", what, version);
  F3R_REQUIRE(dis_mode == F3R_LOSS_DIS || dis_mode == F3R_LOSS_LOG1P, "%s: unknown mode: dis_mode = %d is neither F3R_LOSS_DIS nor F3R_LOSS_LOG1P", what,
              dis_mode);
  F3R_REQUIRE(!(local_scale_consistent && version != 4), "%s: unknown mode: local_scale_consistent exists for version 4 only", what);
  F3R_REQUIRE(pose_dtype == F3R_REAL_F32 || pose_dtype == F3R_REAL_F64, "%s: pose_dtype %d is neither F3R_REAL_F32 nor F3R_REAL_F64", what, pose_dtype);
  F3R_REQUIRE(!use_dist_clip || dist_clip == dist_clip, "%s: dist_clip is NaN", what);
  F3R_REQUIRE(workspace && out, "%s: null workspace / out", what);
  const long long nseg = (long long)n_views * n_samples;
  Work w;
  const size_t need = carve(&w, workspace, nseg);
  F3R_REQUIRE(workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0, "%s: workspace of %zu bytes (8-byte aligned) needed, got %zu", what, need,
              workspace_bytes);
  Tables tab{(const float* const*)gt_pts,   (const uint8_t* const*)valid_mask,    camera_pose,
             (const float* const*)pred_pts, (const float* const*)pred_conf,       (const float* const*)pred_pts_local,
             (const float* const*)pred_conf_local, n_pixels};
  Params p;
  p.n_views = n_views;
  p.n_samples = n_samples;
  p.nseg = (int)nseg;
  p.version = version;
  p.log1p_mode = dis_mode == F3R_LOSS_LOG1P;
  p.gt_scale = gt_scale != 0;
  p.local_scale_consistent = local_scale_consistent != 0;
  p.use_clip = use_dist_clip != 0;
  p.pose_f64 = pose_dtype == F3R_REAL_F64;
  p.clip = dist_clip;
  p.alpha = alpha;
  hipStream_t s = (hipStream_t)stream;
  const int nb = num_blocks();
  const int local = pred_pts_local != nullptr;
  loss_setup_kernel<<<(unsigned)((nseg + THREADS - 1) / THREADS), THREADS, 0, s>>>(tab, w, p);
  loss_pass_kernel<false><<<nb, THREADS, 0, s>>>(tab, w, p);
  loss_factors_kernel<<<1, THREADS, 0, s>>>(w, p, nb, local);
  loss_pass_kernel<true><<<nb, THREADS, 0, s>>>(tab, w, p);
  loss_finish_kernel<<<1, THREADS, 0, s>>>(w, p, nb, local, out);
  return f3r_check_launch(what);
}
