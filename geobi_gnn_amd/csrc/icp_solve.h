// The per-part solve of rigid ICP (icp.hip): sixteen pivoted fp64 moments -> (R, T, s) by Umeyama's closed form, with a
// 3x3 SVD by one-sided (Hestenes) Jacobi.  Plain fp64 C++ that compiles for the host as well as the device: the same text
// runs in icp_solve_kernel and in a stand-alone host program.
#pragma once
#include <math.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace geobi {

constexpr int kIcpState = 24;      // = GEOBI_ICP_STATE
constexpr int kIcpMoments = 16;    // sum dx (3), sum dy (3), sum dx (x) dy (9), sum |dx|^2 (1)
constexpr int kIcpSweeps = 30;     // bound of the Jacobi sweeps (a 3x3 settles in 4 - 6)

// C [3][3] row-major = U diag(S) V^T, S descending, U and V orthonormal also where C has no full rank.
// One-sided Jacobi rotates the COLUMNS of A = C until they are orthogonal: A = C V, |A_j| = S_j, U_j = A_j / S_j.  The
// rotations never form C^T C, so the small singular values keep their relative accuracy.
__host__ __device__ inline void icp_svd3(const double* C, double* U, double* S, double* V) {
  double A[9];
  for (int i = 0; i < 9; ++i) { A[i] = C[i]; V[i] = (i % 4 == 0) ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < kIcpSweeps; ++sweep) {
    bool rotated = false;
    for (int pair = 0; pair < 3; ++pair) {
      const int p = pair == 2 ? 1 : 0, q = pair == 0 ? 1 : 2;
      double alpha = 0.0, beta = 0.0, gamma = 0.0;
      for (int i = 0; i < 3; ++i) {
        alpha += A[3 * i + p] * A[3 * i + p];
        beta += A[3 * i + q] * A[3 * i + q];
        gamma += A[3 * i + p] * A[3 * i + q];
      }
      if (gamma == 0.0 || fabs(gamma) <= 1e-16 * sqrt(alpha * beta)) continue;
      rotated = true;
      const double zeta = (beta - alpha) / (2.0 * gamma);
      const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
      const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
      for (int i = 0; i < 3; ++i) {
        const double ap = A[3 * i + p], aq = A[3 * i + q];
        A[3 * i + p] = c * ap - s * aq;
        A[3 * i + q] = s * ap + c * aq;
        const double vp = V[3 * i + p], vq = V[3 * i + q];
        V[3 * i + p] = c * vp - s * vq;
        V[3 * i + q] = s * vp + c * vq;
      }
    }
    if (!rotated) break;
  }
  double n[3];
  for (int j = 0; j < 3; ++j) n[j] = sqrt(A[j] * A[j] + A[3 + j] * A[3 + j] + A[6 + j] * A[6 + j]);
  int o[3] = {0, 1, 2};                                   // descending, the lower column first among equals
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2 - a; ++b)
      if (n[o[b + 1]] > n[o[b]]) { const int t = o[b]; o[b] = o[b + 1]; o[b + 1] = t; }
  double Vs[9], As[9];
  for (int j = 0; j < 3; ++j) {
    S[j] = n[o[j]];
    for (int i = 0; i < 3; ++i) { Vs[3 * i + j] = V[3 * i + o[j]]; As[3 * i + j] = A[3 * i + o[j]]; }
  }
  for (int i = 0; i < 9; ++i) V[i] = Vs[i];               // a product of rotations and a permutation: orthonormal
  // U: a column whose singular value is noise against the largest carries no direction; complete the basis instead
  if (!(S[0] > 0.0)) {                                    // C = 0 (one point, coincident points): no rotation at all, U = V = I
    for (int i = 0; i < 9; ++i) U[i] = (i % 4 == 0) ? 1.0 : 0.0;
    return;
  }
  const double tiny = 1e-12 * S[0];
  double u0[3] = {1.0, 0.0, 0.0}, u1[3], u2[3];
  if (S[0] > 0.0) for (int i = 0; i < 3; ++i) u0[i] = As[3 * i] / S[0];
  bool have1 = S[0] > 0.0 && S[1] > tiny;
  if (have1) {                                            // Gram-Schmidt against u0, then normalise
    double d = 0.0, len = 0.0;
    for (int i = 0; i < 3; ++i) d += u0[i] * As[3 * i + 1];
    for (int i = 0; i < 3; ++i) { u1[i] = As[3 * i + 1] - d * u0[i]; len += u1[i] * u1[i]; }
    len = sqrt(len);
    have1 = len > 0.5 * S[1];
    if (have1) for (int i = 0; i < 3; ++i) u1[i] /= len;
  }
  if (!have1) {                                           // any unit vector orthogonal to u0: cross with the axis u0 leans on least
    int k = 0;
    if (fabs(u0[1]) < fabs(u0[k])) k = 1;
    if (fabs(u0[2]) < fabs(u0[k])) k = 2;
    double e[3] = {0.0, 0.0, 0.0};
    e[k] = 1.0;
    u1[0] = u0[1] * e[2] - u0[2] * e[1]; u1[1] = u0[2] * e[0] - u0[0] * e[2]; u1[2] = u0[0] * e[1] - u0[1] * e[0];
    const double len = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
    for (int i = 0; i < 3; ++i) u1[i] /= len;
  }
  u2[0] = u0[1] * u1[2] - u0[2] * u1[1]; u2[1] = u0[2] * u1[0] - u0[0] * u1[2]; u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
  if (S[0] > 0.0 && S[2] > tiny && u2[0] * As[2] + u2[1] * As[5] + u2[2] * As[8] < 0.0)
    for (int i = 0; i < 3; ++i) u2[i] = -u2[i];           // the side the third column of A is on
  for (int i = 0; i < 3; ++i) { U[3 * i] = u0[i]; U[3 * i + 1] = u1[i]; U[3 * i + 2] = u2[i]; }
}

__host__ __device__ inline double icp_det3(const double* M) {
  return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// m: the moments of dx = x - px, dy = y[idx] - py over the Q rows of a part (px, py: the pivots).  Writes slots 0-12
// (R row-major, T, s) and 17 (the smallest singular value of C over the largest; 0 for C = 0) of st.
__host__ __device__ inline void icp_solve_part(const double* m, const double* px, const double* py, double Q, int flags,
                                               double* st) {
  double mx[3], my[3], C[9];
  for (int a = 0; a < 3; ++a) { mx[a] = m[a] / Q; my[a] = m[3 + a] / Q; }
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) C[3 * a + b] = (m[6 + 3 * a + b] - m[a] * my[b]) / Q;
  double var = (m[15] - (m[0] * mx[0] + m[1] * mx[1] + m[2] * mx[2])) / Q;
  if (!(var > 0.0)) var = 0.0;
  double U[9], S[3], V[9];
  icp_svd3(C, U, S, V);
  double UVt[9];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) UVt[3 * a + b] = U[3 * a] * V[3 * b] + U[3 * a + 1] * V[3 * b + 1] + U[3 * a + 2] * V[3 * b + 2];
  const double e2 = (!(flags & 2) && icp_det3(UVt) < 0.0) ? -1.0 : 1.0;
  double* R = st;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) R[3 * a + b] = U[3 * a] * V[3 * b] + U[3 * a + 1] * V[3 * b + 1] + e2 * U[3 * a + 2] * V[3 * b + 2];
  const double s = ((flags & 1) && var > 0.0) ? (S[0] + S[1] + e2 * S[2]) / var : 1.0;
  for (int b = 0; b < 3; ++b) {                           // T = mu_y - s mu_x R, mu = pivot + mean of the differences
    double r = 0.0;
    for (int a = 0; a < 3; ++a) r += (px[a] + mx[a]) * R[3 * a + b];
    st[9 + b] = (py[b] + my[b]) - s * r;
  }
  st[12] = s;
  st[17] = S[0] > 0.0 ? S[2] / S[0] : 0.0;
}

}  // namespace geobi
