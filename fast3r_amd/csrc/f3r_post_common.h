// The quantile solver shared by the post-processing kernels (f3r_post.hip: align / focal; f3r_recon.hip: evaluate_reconstruction;
// f3r_depth.hip: the confidence threshold and the masked medians of the depth metrics): the
// exact torch.quantile of a block's values by radix select over the order-preserving 32-bit keys of f3r_prims.h.  The other solver they
// share, the Umeyama similarity solve from fp64 raw moments (similarity_from_moments), is in f3r_linalg.h, which also builds for the host.
// The wave and block primitives (keys, ballots, sums, the scan kernel) live in f3r_prims.h, which this header brings along.  Header-only
// (inline device functions and templates).
#pragma once

#include "f3r_linalg.h"
#include "f3r_prims.h"

// k-th smallest (0-based) of the keys key_of(0), .., key_of(n - 1) by radix select over 11 + 11 + 10 bits; all NT threads return the same
// value.  A masked select gives the entries it leaves out the largest key and takes its ranks from the count of the others.
template <int NT, class KeyOf>
__device__ uint32_t select_kth_key(KeyOf key_of, int64_t n, int64_t k, uint32_t* hist /*2048*/, int64_t* sh_i64 /*2*/) {
  uint32_t prefix = 0, prefix_mask = 0;
  const int shifts[3] = {21, 10, 0};
  const int bits[3] = {11, 11, 10};
  for (int pass = 0; pass < 3; ++pass) {
    const int nb = 1 << bits[pass];
    for (int i = threadIdx.x; i < nb; i += NT) hist[i] = 0;
    __syncthreads();
    for (int64_t i = threadIdx.x; i < n; i += NT) {
      const uint32_t key = key_of(i);
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

// the same over the keys of conf[0..n)
template <int NT>
__device__ uint32_t select_kth(const float* __restrict__ conf, int64_t n, int64_t k, uint32_t* hist /*2048*/, int64_t* sh_i64 /*2*/) {
  return select_kth_key<NT>([conf](int64_t i) { return fkey(conf[i]); }, n, k, hist, sh_i64);
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
