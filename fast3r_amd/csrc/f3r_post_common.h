// The two solvers shared by the post-processing kernels (f3r_post.hip: align / focal; f3r_recon.hip: evaluate_reconstruction):
// the exact torch.quantile of a block's values by radix select over the order-preserving 32-bit keys of f3r_prims.h, and the
// Umeyama similarity solve from fp64 raw moments.  The wave and block primitives (keys, ballots, sums, the scan kernel) live in
// f3r_prims.h, which this header brings along.  Header-only (inline device functions and templates).
#pragma once

#include "f3r_linalg.h"
#include "f3r_prims.h"

// k-th smallest key (0-based) of conf[0..n) by radix select over 11 + 11 + 10 bits; all NT threads return the same value.
template <int NT>
__device__ uint32_t select_kth(const float* __restrict__ conf, int64_t n, int64_t k, uint32_t* hist /*2048*/, int64_t* sh_i64 /*2*/) {
  uint32_t prefix = 0, prefix_mask = 0;
  const int shifts[3] = {21, 10, 0};
  const int bits[3] = {11, 11, 10};
  for (int pass = 0; pass < 3; ++pass) {
    const int nb = 1 << bits[pass];
    for (int i = threadIdx.x; i < nb; i += NT) hist[i] = 0;
    __syncthreads();
    for (int64_t i = threadIdx.x; i < n; i += NT) {
      const uint32_t key = fkey(conf[i]);
      if ((key & prefix_mask) == prefix) atomicAdd(&hist[(key >> shifts[pass]) & (nb - 1)], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int64_t acc = 0;
      int b = 0;
      for (; b < nb; ++b) {
        if (acc + hist[b] > k) break;
        acc += hist[b];
      }
      sh_i64[0] = b;
      sh_i64[1] = k - acc;
    }
    __syncthreads();
    const uint32_t b = (uint32_t)sh_i64[0];
    k = sh_i64[1];
    prefix |= b << shifts[pass];
    prefix_mask |= (uint32_t)(nb - 1) << shifts[pass];
    __syncthreads();
  }
  return prefix;
}

// torch.quantile(conf[0..n), q) (linear): rank = q*(n-1) in fp32, at::lerp between the two order statistics.  Every thread
// returns the value (through *sh_thr).
template <int NT>
__device__ float block_quantile(const float* __restrict__ cf, int64_t n, float q, uint32_t* hist, int64_t* sh_i64, float* sh_thr) {
  const float rank = q * (float)(n - 1);
  const float rlo = floorf(rank);
  const int64_t klo = (int64_t)rlo;
  const int64_t khi = (int64_t)ceilf(rank);
  const float vlo = fkey_inv(select_kth<NT>(cf, n, klo, hist, sh_i64));
  float vhi = vlo;
  if (khi != klo) vhi = fkey_inv(select_kth<NT>(cf, n, khi, hist, sh_i64));
  if (threadIdx.x == 0) {
    const float w = rank - rlo;
    const float d = vhi - vlo;
    *sh_thr = (w < 0.5f) ? vlo + w * d : vhi - d * (1.0f - w);  // at::lerp
  }
  __syncthreads();
  return *sh_thr;
}

// Umeyama from raw moments m[17] = {n, sum x (3), sum y (3), sum y_i x_j (9), sum |x|^2} -> (R, t, s) as 13 floats
// [R row-major (9) | t (3) | s]; the caller has handled n < 3.
__device__ inline void similarity_from_moments(const double* m, float* o) {
  const double n = m[0];
  const double xm[3] = {m[1] / n, m[2] / n, m[3] / n}, ym[3] = {m[4] / n, m[5] / n, m[6] / n};
  double M[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) M[i][j] = m[7 + i * 3 + j] - n * ym[i] * xm[j];
  const double sx2 = m[16] - n * (xm[0] * xm[0] + xm[1] * xm[1] + xm[2] * xm[2]);
  double U[3][3], S[3], V[3][3];
  f3r_la::svd3(M, U, S, V);
  const double d = (f3r_la::det3(U) * f3r_la::det3(V) < 0) ? -1.0 : 1.0;
  double R[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[i][j] = U[i][0] * V[j][0] + U[i][1] * V[j][1] + d * U[i][2] * V[j][2];
  const double scale = (S[0] + S[1] + d * S[2]) / sx2;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) o[i * 3 + j] = (float)R[i][j];
    o[9 + i] = (float)(ym[i] - scale * (R[i][0] * xm[0] + R[i][1] * xm[1] + R[i][2] * xm[2]));
  }
  o[12] = (float)scale;
}

__device__ inline void identity_rts(float* o) {
  for (int i = 0; i < 9; ++i) o[i] = (i % 4 == 0) ? 1.f : 0.f;
  o[9] = o[10] = o[11] = 0.f;
  o[12] = 1.f;
}
