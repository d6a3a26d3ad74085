// Small dense linear algebra in fp64 for the post-processing kernels (one thread per problem): 3x3 SVD, symmetric Jacobi eigen-solver,
// Cholesky solve, and the Umeyama similarity solve from raw moments that align and evaluate_reconstruction share.  Header-only; device
// functions in the library -- with F3R_HOST_BUILD defined the same source compiles as plain C++ (tests build this header and f3r_sqpnp.h
// that way to check the arithmetic on the CPU; the product never does).
#pragma once
#ifdef F3R_HOST_BUILD
#include <cmath>
#define F3R_LA_FN inline
#define F3R_LA_FORCE inline
#else
#include <hip/hip_runtime.h>
#define F3R_LA_FN __device__ inline
#define F3R_LA_FORCE __device__ __forceinline__
#endif

namespace f3r_la {

// 3x3 SVD of M:  M = U diag(s) V^T with V from the Jacobi eigen-decomposition of M^T M (columns sorted by eigenvalue, descending) and U, s
// from M V; U and V are orthonormal whatever the conditioning of M.
F3R_LA_FN void svd3(const double M[3][3], double U[3][3], double S[3], double V[3][3]) {
  double A[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double a = 0;
      for (int k = 0; k < 3; ++k) a += M[k][i] * M[k][j];
      A[i][j] = a;
      V[i][j] = (i == j) ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 30; ++sweep) {
    const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
    if (off < 1e-300) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        if (fabs(A[p][q]) < 1e-300) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; ++k) {  // A <- A J
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 3; ++k) {  // A <- J^T A
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 3; ++k) {  // V <- V J
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  double ev[3] = {A[0][0], A[1][1], A[2][2]};
  int idx[3] = {0, 1, 2};
  for (int i = 0; i < 2; ++i)
    for (int j = i + 1; j < 3; ++j)
      if (ev[idx[j]] > ev[idx[i]]) { const int tmp = idx[i]; idx[i] = idx[j]; idx[j] = tmp; }
  double Vs[3][3];
  for (int c = 0; c < 3; ++c) {
    S[c] = sqrt(fmax(ev[idx[c]], 0.0));
    for (int r = 0; r < 3; ++r) Vs[r][c] = V[r][idx[c]];
  }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) V[r][c] = Vs[r][c];
  // U columns: M v_c, made orthogonal to the columns before it (Gram-Schmidt, two passes) and normalised.  The eigenvalues of M^T M
  // carry the square of M's condition number, so sqrt(ev) of a singular value below ~1e-8 S0 is rounding noise, and M v_c / S_c would be
  // noise over noise: neither unit length nor orthogonal.  M v_c itself is good to eps * S0.  A column whose remainder is below
  // RANK_TOL * S0 has no direction of its own: the basis is completed instead (any unit vector orthogonal to u0; u0 x u1), and its singular
  // value is that remainder.  A small but real third singular value keeps its column, hence its sign for the caller's determinant
  // correction; a completed third column gives det U = +1, and the sign then multiplies a singular value that is zero to RANK_TOL.
  constexpr double RANK_TOL = 1e-7;
  double Un[3][3];  // Un[c] = column c of U
  double s0 = 0.0;
  for (int c = 0; c < 3; ++c) {
    double u[3];
    for (int r = 0; r < 3; ++r) u[r] = M[r][0] * V[0][c] + M[r][1] * V[1][c] + M[r][2] * V[2][c];
    const double full = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    for (int pass = 0; pass < 2; ++pass)
      for (int p = 0; p < c; ++p) {
        const double d = u[0] * Un[p][0] + u[1] * Un[p][1] + u[2] * Un[p][2];
        for (int r = 0; r < 3; ++r) u[r] -= d * Un[p][r];
      }
    const double rem = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    if (c == 0) s0 = full;
    if (rem > RANK_TOL * s0 && rem > 1e-300) {
      S[c] = full;
      for (int r = 0; r < 3; ++r) Un[c][r] = u[r] / rem;
      continue;
    }
    S[c] = rem;
    if (c == 0) {
      Un[0][0] = 1; Un[0][1] = 0; Un[0][2] = 0;
    } else if (c == 1) {  // any unit vector orthogonal to u0
      const double a0 = fabs(Un[0][0]), a1 = fabs(Un[0][1]), a2 = fabs(Un[0][2]);
      double e[3] = {0, 0, 0};
      e[(a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2)] = 1.0;
      const double d = e[0] * Un[0][0] + e[1] * Un[0][1] + e[2] * Un[0][2];
      for (int r = 0; r < 3; ++r) u[r] = e[r] - d * Un[0][r];
      const double n = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
      for (int r = 0; r < 3; ++r) Un[1][r] = u[r] / n;
    } else {  // u2 = u0 x u1
      Un[2][0] = Un[0][1] * Un[1][2] - Un[0][2] * Un[1][1];
      Un[2][1] = Un[0][2] * Un[1][0] - Un[0][0] * Un[1][2];
      Un[2][2] = Un[0][0] * Un[1][1] - Un[0][1] * Un[1][0];
    }
  }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) U[r][c] = Un[c][r];
}

F3R_LA_FORCE double det3(const double A[3][3]) {
  return A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
         A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
}


// Eigen-decomposition of a symmetric N x N matrix by cyclic Jacobi rotations: A <- diag(eigenvalues), V columns = eigenvectors.
template <int N>
F3R_LA_FN void jacobi_sym(double A[N][N], double V[N][N]) {
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 40; ++sweep) {
    double off = 0.0, dia = 0.0;
    for (int i = 0; i < N; ++i) {
      dia += fabs(A[i][i]);
      for (int j = i + 1; j < N; ++j) off += fabs(A[i][j]);
    }
    if (off <= 1e-18 * dia || off < 1e-300) break;
    for (int p = 0; p < N - 1; ++p)
      for (int q = p + 1; q < N; ++q) {
        if (fabs(A[p][q]) < 1e-300) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < N; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < N; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < N; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
}

// Solve A x = b for a symmetric positive definite N x N matrix (Cholesky); returns false when A is not numerically SPD.
template <int N>
F3R_LA_FN bool chol_solve(const double A[N][N], const double* b, double* x) {
  double L[N][N];
  for (int i = 0; i < N; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = A[i][j];
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      if (i == j) {
        if (!(s > 0.0)) return false;
        L[i][i] = sqrt(s);
      } else {
        L[i][j] = s / L[j][j];
      }
    }
  double y[N];
  for (int i = 0; i < N; ++i) {
    double s = b[i];
    for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
    y[i] = s / L[i][i];
  }
  for (int i = N - 1; i >= 0; --i) {
    double s = y[i];
    for (int k = i + 1; k < N; ++k) s -= L[k][i] * x[k];
    x[i] = s / L[i][i];
  }
  return true;
}

}  // namespace f3r_la

// Umeyama from raw moments m[17] = {n, sum x (3), sum y (3), sum y_i x_j (9), sum |x|^2} -> (R, t, s) as 13 floats
// [R row-major (9) | t (3) | s]; the caller has handled n < 3.
F3R_LA_FN void similarity_from_moments(const double* m, float* o) {
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

F3R_LA_FN void identity_rts(float* o) {
  for (int i = 0; i < 9; ++i) o[i] = (i % 4 == 0) ? 1.f : 0.f;
  o[9] = o[10] = o[11] = 0.f;
  o[12] = 1.f;
}
