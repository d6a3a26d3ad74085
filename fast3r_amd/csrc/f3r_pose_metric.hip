// Relative camera-pose errors over all view pairs and their counts (include/f3r.h: f3r_pose_pair_metrics, f3r_pose_error_stats).
// The reference (fast3r/eval/cam_pose_metric.py: camera_to_rel_deg, calculate_auc; fast3r/utils/so3_utils.py) gathers (pairs, 4, 4)
// tensors on the CPU; here a workgroup owns one 32 x 32 tile of the upper triangle of (i, j), stages the 2 x 32 poses of both pose sets in
// LDS once and evaluates its pairs in fp64 on the exactly widened inputs.  Counts (thresholds, torch.histc bins, two diagnostics) are
// integer sums: wave ballots and LDS integer atomics per workgroup, one 64-bit integer atomic per non-zero counter per workgroup.
// Built with -ffp-contract=off: every fp64 product rounds on its own.
#include <math.h>

#include "f3r_common.h"
#include "f3r_prims.h"

namespace {

constexpr int TILE = 32;          // pairs tile: TILE i-poses x TILE j-poses
constexpr int THREADS = 256;      // TILE * TILE / THREADS pairs per thread
constexpr int MAX_THR = 8;        // thresholds per kind
constexpr int MAX_BINS = 256;
constexpr int MAX_COUNTERS = 2 * MAX_THR + MAX_BINS + 2;

struct MetricParams {
  double r_thr[MAX_THR], t_thr[MAX_THR];
  double max_threshold;
  int n_r, n_t, n_bins;
  __host__ __device__ int stride() const { return n_r + n_t + n_bins + 2; }
};

// acos linearly extrapolated outside (-(1 - 1e-4), 1 - 1e-4): so3_utils.py acos_linear_extrapolation / _acos_linear_approximation
__device__ inline double acos_extrapolated(double x) {
  const double bound = 1.0 - 1e-4;
  if (x >= bound) return (x - bound) * (-1.0 / sqrt(1.0 - bound * bound)) + acos(bound);
  if (x <= -bound) return (x - (-bound)) * (-1.0 / sqrt(1.0 - bound * bound)) + acos(-bound);
  return acos(x);  // NaN stays NaN (neither comparison holds), as in the reference
}

// One pair's contribution to its workgroup's counters.  Every thread of the workgroup calls this the same number of times (`live`
// false for the padding of a tile), because the threshold counts are wave ballots.  cnt: LDS, p.stride() entries.
__device__ inline void accumulate(const MetricParams& p, bool live, double r, double t, bool bad_trace, bool defaulted, int* cnt) {
  for (int k = 0; k < p.n_r; ++k) wave_count_add(live && r < p.r_thr[k], &cnt[k]);
  for (int k = 0; k < p.n_t; ++k) wave_count_add(live && t < p.t_thr[k], &cnt[p.n_r + k]);
  wave_count_add(live && bad_trace, &cnt[p.n_r + p.n_t + p.n_bins]);
  wave_count_add(live && defaulted, &cnt[p.n_r + p.n_t + p.n_bins + 1]);
  if (!live) return;
  // torch.max propagates NaN; torch.histc(bins, 0, max) drops NaN and what lies outside [0, max], and puts max itself into the last bin
  const double m = (r != r || t != t) ? NAN : (r > t ? r : t);
  if (m >= 0.0 && m <= p.max_threshold) {
    long long bin = (long long)(m / p.max_threshold * (double)p.n_bins);
    if (bin >= p.n_bins) bin = p.n_bins - 1;
    if (bin >= 0) atomicAdd(&cnt[p.n_r + p.n_t + (int)bin], 1);
  }
}

__device__ inline void clear_counters(int* cnt, int n) {
  for (int k = threadIdx.x; k < n; k += blockDim.x) cnt[k] = 0;
  __syncthreads();
}

__device__ inline void flush_counters(const int* cnt, int n, long long* out) {
  __syncthreads();
  for (int k = threadIdx.x; k < n; k += blockDim.x)
    if (cnt[k]) atomicAdd(reinterpret_cast<unsigned long long*>(out + k), (unsigned long long)cnt[k]);
}

// tile t of the upper triangle (bi <= bj) of an nb x nb grid, row-major: row bi starts at bi * nb - bi (bi - 1) / 2
__device__ inline void decode_tile(long long t, int nb, int* bi_out, int* bj_out) {
  const double b = 2.0 * nb + 1.0;
  long long bi = (long long)((b - sqrt(b * b - 8.0 * (double)t)) * 0.5);
  if (bi < 0) bi = 0;
  if (bi > nb - 1) bi = nb - 1;
  while (bi > 0 && bi * nb - bi * (bi - 1) / 2 > t) --bi;
  while (bi + 1 < nb && (bi + 1) * nb - (bi + 1) * bi / 2 <= t) ++bi;
  *bi_out = (int)bi;
  *bj_out = (int)(bi + (t - (bi * nb - bi * (bi - 1) / 2)));
}

template <typename T>
__global__ __launch_bounds__(THREADS) void pose_pair_kernel(const T* __restrict__ pred, const T* __restrict__ gt, int n_views, int nb,
                                                            MetricParams p, T* __restrict__ rel_r, T* __restrict__ rel_t,
                                                            long long* __restrict__ counts) {
  // [set: pred, gt][side: i, j][pose of the tile][4 x 4 row-major]
  __shared__ double pose[2][2][TILE][16];
  __shared__ int cnt[MAX_COUNTERS];
  const int sample = blockIdx.y;
  int bi, bj;
  decode_tile(blockIdx.x, nb, &bi, &bj);
  const int stride = p.stride();
  clear_counters(cnt, stride);
  for (int e = threadIdx.x; e < 2 * 2 * TILE * 16; e += THREADS) {
    const int c = e % 16, v = (e / 16) % TILE, side = (e / (16 * TILE)) & 1, set = e / (32 * TILE);
    const int view = (side ? bj : bi) * TILE + v;
    double x = 0.0;
    if (view < n_views) x = (double)((set ? gt : pred)[((long long)sample * n_views + view) * 16 + c]);
    pose[set][side][v][c] = x;
  }
  __syncthreads();
  const long long n = n_views, n_pairs = n * (n - 1) / 2;
  for (int e = threadIdx.x; e < TILE * TILE; e += THREADS) {
    const int ti = e / TILE, tj = e % TILE;
    const long long i = (long long)bi * TILE + ti, j = (long long)bj * TILE + tj;
    const bool live = i < j && j < n;
    double r_deg = 0.0, t_deg = 0.0;
    bool bad_trace = false, defaulted = false;
    if (live) {
      // inv(P_i) P_j of both sets as the 4 x 4 product it is in the reference, inv(P_i) = [R_i^T | -(R_i^T t_i); 0 0 0 1] (closed_form_inverse):
      // the bottom row of P_j (0 0 0 1 in a valid pose) takes part, so a non-finite t_i reaches the rotation as it does there
      double rel[2][12];  // R 3 x 3 row-major | t
      for (int s = 0; s < 2; ++s) {
        const double* A = pose[s][0][ti];
        const double* B = pose[s][1][tj];
        for (int a = 0; a < 3; ++a) {
          const double tinv = -(A[0 * 4 + a] * A[3] + A[1 * 4 + a] * A[7] + A[2 * 4 + a] * A[11]);
          for (int b = 0; b < 3; ++b)
            rel[s][a * 3 + b] = A[0 * 4 + a] * B[0 * 4 + b] + A[1 * 4 + a] * B[1 * 4 + b] + A[2 * 4 + a] * B[2 * 4 + b] + tinv * B[3 * 4 + b];
          rel[s][9 + a] = A[0 * 4 + a] * B[3] + A[1 * 4 + a] * B[7] + A[2 * 4 + a] * B[11] + tinv * B[15];
        }
      }
      // rotation: trace(R_gt_rel R_pred_rel^T) = sum of the elementwise products (so3_relative_angle / so3_rotation_angle, eps = 1e-4)
      double tr = 0.0;
      for (int a = 0; a < 3; ++a) tr += rel[1][a * 3 + 0] * rel[0][a * 3 + 0] + rel[1][a * 3 + 1] * rel[0][a * 3 + 1] + rel[1][a * 3 + 2] * rel[0][a * 3 + 2];
      bad_trace = tr < -1.0 - 1e-4 || tr > 3.0 + 1e-4;
      r_deg = acos_extrapolated((tr - 1.0) * 0.5) * 180.0 / M_PI;
      // translation: compare_translation_by_angle (eps = 1e-15, default_err = 1e6)
      const double eps = 1e-15;
      const double* tp = &rel[0][9];
      const double* tg = &rel[1][9];
      const double np_ = sqrt(tp[0] * tp[0] + tp[1] * tp[1] + tp[2] * tp[2]) + eps;
      const double ng_ = sqrt(tg[0] * tg[0] + tg[1] * tg[1] + tg[2] * tg[2]) + eps;
      const double dot = (tp[0] / np_) * (tg[0] / ng_) + (tp[1] / np_) * (tg[1] / ng_) + (tp[2] / np_) * (tg[2] / ng_);
      double loss = 1.0 - dot * dot;
      if (loss < eps) loss = eps;  // clamp_min: NaN stays NaN
      double err = acos(sqrt(1.0 - loss));
      if (err != err || isinf(err)) {
        err = 1e6;
        defaulted = true;
      }
      t_deg = err * 180.0 / M_PI;
      if (rel_r) {
        const long long pidx = (long long)sample * n_pairs + i * (2 * n - i - 1) / 2 + (j - i - 1);
        rel_r[pidx] = (T)r_deg;
        rel_t[pidx] = (T)t_deg;
      }
    }
    accumulate(p, live, r_deg, t_deg, bad_trace, defaulted, cnt);
  }
  flush_counters(cnt, stride, counts + (long long)sample * stride);
}

template <typename T>
__global__ __launch_bounds__(THREADS) void pose_stats_kernel(const T* __restrict__ r, const T* __restrict__ t, long long n, MetricParams p,
                                                             long long* __restrict__ counts) {
  __shared__ int cnt[MAX_COUNTERS];
  const int stride = p.stride();
  clear_counters(cnt, stride);
  const long long step = (long long)gridDim.x * THREADS;
  // whole-workgroup rounds: every thread calls accumulate() the same number of times
  for (long long base = (long long)blockIdx.x * THREADS; base < n; base += step) {
    const long long e = base + threadIdx.x;
    const bool live = e < n;
    accumulate(p, live, live ? (double)r[e] : 0.0, live ? (double)t[e] : 0.0, false, false, cnt);
  }
  flush_counters(cnt, stride, counts);
}

int fill_params(MetricParams& p, const double* r_thr, int n_r, const double* t_thr, int n_t, int n_bins, double max_threshold, const char* what) {
  F3R_REQUIRE(n_r >= 0 && n_r <= MAX_THR && n_t >= 0 && n_t <= MAX_THR, "%s: at most %d thresholds per kind (got %d rotation, %d translation)", what,
              MAX_THR, n_r, n_t);
  F3R_REQUIRE((n_r == 0 || r_thr) && (n_t == 0 || t_thr), "%s: null threshold array", what);
  F3R_REQUIRE(n_bins >= 1 && n_bins <= MAX_BINS, "%s: n_bins = %d outside 1..%d", what, n_bins, MAX_BINS);
  F3R_REQUIRE(max_threshold > 0.0, "%s: max_threshold must be positive", what);
  for (int k = 0; k < MAX_THR; ++k) {
    p.r_thr[k] = k < n_r ? r_thr[k] : 0.0;
    p.t_thr[k] = k < n_t ? t_thr[k] : 0.0;
  }
  p.max_threshold = max_threshold;
  p.n_r = n_r;
  p.n_t = n_t;
  p.n_bins = n_bins;
  return F3R_OK;
}

}  // namespace

extern "C" int f3r_pose_pair_metrics(const void* pred, const void* gt, int dtype, int n_samples, int n_views, const double* r_thresholds, int n_r,
                                     const double* t_thresholds, int n_t, int n_bins, double max_threshold, void* rel_r, void* rel_t,
                                     int64_t* counts, f3r_stream_t stream) {
  const char* what = "f3r_pose_pair_metrics";
  F3R_REQUIRE(pred && gt && counts, "%s: null pred / gt / counts", what);
  F3R_REQUIRE(dtype == F3R_REAL_F32 || dtype == F3R_REAL_F64, "%s: dtype %d is neither F3R_REAL_F32 nor F3R_REAL_F64", what, dtype);
  F3R_REQUIRE(n_samples >= 1 && n_samples <= 65535, "%s: n_samples = %d outside 1..65535", what, n_samples);
  F3R_REQUIRE(n_views >= 2 && n_views <= (1 << 20), "%s: n_views = %d outside 2..2^20 (a pair needs two views)", what, n_views);
  F3R_REQUIRE((rel_r == nullptr) == (rel_t == nullptr), "%s: rel_r and rel_t are given together or not at all", what);
  MetricParams p;
  if (int e = fill_params(p, r_thresholds, n_r, t_thresholds, n_t, n_bins, max_threshold, what)) return e;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, sizeof(int64_t) * (size_t)n_samples * p.stride(), s) != hipSuccess) return f3r_check_launch(what);
  const int nb = (n_views + TILE - 1) / TILE;
  const long long tiles = (long long)nb * (nb + 1) / 2;
  dim3 grid((unsigned)tiles, (unsigned)n_samples);
  if (dtype == F3R_REAL_F32)
    pose_pair_kernel<float><<<grid, THREADS, 0, s>>>((const float*)pred, (const float*)gt, n_views, nb, p, (float*)rel_r, (float*)rel_t, (long long*)counts);
  else
    pose_pair_kernel<double><<<grid, THREADS, 0, s>>>((const double*)pred, (const double*)gt, n_views, nb, p, (double*)rel_r, (double*)rel_t,
                                                      (long long*)counts);
  return f3r_check_launch(what);
}

extern "C" int f3r_pose_error_stats(const void* r, const void* t, int64_t n, int dtype, const double* r_thresholds, int n_r,
                                    const double* t_thresholds, int n_t, int n_bins, double max_threshold, int64_t* counts, f3r_stream_t stream) {
  const char* what = "f3r_pose_error_stats";
  F3R_REQUIRE(counts, "%s: null counts", what);
  F3R_REQUIRE(n >= 0 && n < (1LL << 40), "%s: n = %lld outside 0..2^40", what, (long long)n);
  F3R_REQUIRE(n == 0 || (r && t), "%s: null r / t", what);
  F3R_REQUIRE(dtype == F3R_REAL_F32 || dtype == F3R_REAL_F64, "%s: dtype %d is neither F3R_REAL_F32 nor F3R_REAL_F64", what, dtype);
  MetricParams p;
  if (int e = fill_params(p, r_thresholds, n_r, t_thresholds, n_t, n_bins, max_threshold, what)) return e;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, sizeof(int64_t) * (size_t)p.stride(), s) != hipSuccess) return f3r_check_launch(what);
  if (n == 0) return F3R_OK;
  long long blocks = (n + THREADS - 1) / THREADS;
  if (blocks > 1024) blocks = 1024;
  if (dtype == F3R_REAL_F32)
    pose_stats_kernel<float><<<(unsigned)blocks, THREADS, 0, s>>>((const float*)r, (const float*)t, n, p, (long long*)counts);
  else
    pose_stats_kernel<double><<<(unsigned)blocks, THREADS, 0, s>>>((const double*)r, (const double*)t, n, p, (long long*)counts);
  return f3r_check_launch(what);
}
