// diffspectra_amd - the 3x3 fp64 singular value decomposition behind both Kabsch fits of the library: the noise-alignment rotation of the
// training loss (k_kabsch, ds_train.hip) and the rotation of the Hungarian-matched RMSD (k_match_records, ds_match.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// 3x3 SVD by one-sided Jacobi on columns (fp64): A V = U S.
__device__ inline void svd3(const double A[3][3], double U[3][3], double S[3], double V[3][3]) {
  double W[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) { W[i][j] = A[i][j]; V[i][j] = (i == j) ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        double al = 0, be = 0, ga = 0;
        for (int i = 0; i < 3; ++i) { al += W[i][p] * W[i][p]; be += W[i][q] * W[i][q]; ga += W[i][p] * W[i][q]; }
        off = fmax(off, fabs(ga) / (sqrt(al * be) + 1e-300));
        if (fabs(ga) < 1e-300) continue;
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int i = 0; i < 3; ++i) {
          const double wp = W[i][p], wq = W[i][q];
          W[i][p] = c * wp - s * wq; W[i][q] = s * wp + c * wq;
          const double vp = V[i][p], vq = V[i][q];
          V[i][p] = c * vp - s * vq; V[i][q] = s * vp + c * vq;
        }
      }
    if (off < 1e-15) break;
  }
  for (int j = 0; j < 3; ++j) {
    S[j] = sqrt(W[0][j] * W[0][j] + W[1][j] * W[1][j] + W[2][j] * W[2][j]);
    for (int i = 0; i < 3; ++i) U[i][j] = S[j] > 1e-300 ? W[i][j] / S[j] : 0.0;
  }
  // sort singular values descending (the sign correction of Kabsch acts on the smallest one)
  for (int a = 0; a < 2; ++a)
    for (int b = a + 1; b < 3; ++b)
      if (S[b] > S[a]) {
        const double ts = S[a]; S[a] = S[b]; S[b] = ts;
        for (int i = 0; i < 3; ++i) {
          const double tu = U[i][a]; U[i][a] = U[i][b]; U[i][b] = tu;
          const double tv = V[i][a]; V[i][a] = V[i][b]; V[i][b] = tv;
        }
      }
  // complete a rank-deficient U to an orthonormal basis (columns with zero singular value)
  if (S[2] <= 1e-300 * 0 + 1e-14 * (S[0] + 1e-300)) {
    if (S[1] > 1e-14 * (S[0] + 1e-300)) {
      U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
      U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
      U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
    }
  }
}
