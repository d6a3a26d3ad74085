// TEST INFRASTRUCTURE: the product's similarity solve (fast3r_amd/csrc/f3r_linalg.h: svd3, similarity_from_moments) compiled for the host, so
// that tests/test_post_cases.py can run its arithmetic on degenerate clouds without a GPU.  The moments are accumulated as align_stats_kernel
// accumulates them: fp64 sums of products of the fp32 inputs.  Nothing in the product links this file.
#define F3R_HOST_BUILD 1
#include "../../fast3r_amd/csrc/f3r_linalg.h"

extern "C" void linalg_host_similarity(const float* x, const float* y, int n, float* rts13) {
  double m[17];
  for (int k = 0; k < 17; ++k) m[k] = 0.0;
  for (int i = 0; i < n; ++i) {
    const double x0 = x[3 * i], x1 = x[3 * i + 1], x2 = x[3 * i + 2];
    const double y0 = y[3 * i], y1 = y[3 * i + 1], y2 = y[3 * i + 2];
    const double t[17] = {1.0, x0, x1, x2, y0, y1, y2, y0 * x0, y0 * x1, y0 * x2, y1 * x0, y1 * x1, y1 * x2, y2 * x0, y2 * x1, y2 * x2,
                          x0 * x0 + x1 * x1 + x2 * x2};
    for (int k = 0; k < 17; ++k) m[k] += t[k];
  }
  if (m[0] < 3.0) identity_rts(rts13);
  else similarity_from_moments(m, rts13);
}

extern "C" void linalg_host_svd3(const double* M9, double* U9, double* S3, double* V9) {
  double M[3][3], U[3][3], V[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) M[i][j] = M9[3 * i + j];
  f3r_la::svd3(M, U, S3, V);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) { U9[3 * i + j] = U[i][j]; V9[3 * i + j] = V[i][j]; }
}
