// proposal_factor.h -- the re-tuning of a correlated proposal (include/sxmc_hip.h, sxmc_proposal_factor): pure host
// code, no device, no library state; the one implementation behind the C entry point, which both walkers call.  The
// law is written out in the header and replayed by tests/step_reference_cov.py, which this file is held to bit for
// bit: every operation below is a separate double operation (build with -ffp-contract=off), every sum sequential.
#pragma once

#include <cmath>
#include <cstddef>
#include <vector>

namespace sxproposal {

// T (row-major, P x P, zero above the diagonal) = the Cholesky factor of A (row-major, unit diagonal), row by row.
// False at the first pivot that is not positive.
inline bool cholesky_rows(const std::vector<double>& A, size_t P, std::vector<double>& T) {
  T.assign(P * P, 0.0);
  for (size_t i = 0; i < P; i++) {
    for (size_t j = 0; j <= i; j++) {
      double s = A[i * P + j];
      for (size_t k = 0; k < j; k++) {
        const double prod = T[i * P + k] * T[j * P + k];
        s = s - prod;
      }
      if (j == i) {
        if (!(s > 0.0)) return false;
        T[i * P + i] = std::sqrt(s);
      } else {
        s = s / T[j * P + j];
        T[i * P + j] = s;
      }
    }
  }
  return true;
}

// factor[j * P + i] = L_ij.  Arguments checked by the caller.  Returns the shrinkage that succeeded.
inline double proposal_factor(const float* rows, size_t nrows, size_t P, const float* new_widths, double shrinkage,
                              double* factor) {
  const size_t pitch = P + 1;
  std::vector<double> mean(P, 0.0), S(P * P, 0.0), dx(P);
  if (nrows > 0) {
    for (size_t r = 0; r < nrows; r++) {
      for (size_t j = 0; j < P; j++) mean[j] = mean[j] + (double)rows[r * pitch + j];
    }
    for (size_t j = 0; j < P; j++) mean[j] = mean[j] / (double)nrows;
    for (size_t r = 0; r < nrows; r++) {
      for (size_t j = 0; j < P; j++) dx[j] = (double)rows[r * pitch + j] - mean[j];
      for (size_t j = 0; j < P; j++) {
        if (!(new_widths[j] > 0)) continue;
        for (size_t k = 0; k <= j; k++) {
          const double prod = dx[j] * dx[k];
          S[j * P + k] = S[j * P + k] + prod;
        }
      }
    }
  }
  // the correlation matrix of the free columns; a fixed column, or one without spread, keeps the identity's row and column
  std::vector<char> coupled(P);
  std::vector<double> root(P, 0.0), R(P * P, 0.0);
  for (size_t j = 0; j < P; j++) {
    coupled[j] = new_widths[j] > 0 && S[j * P + j] > 0.0;
    if (coupled[j]) root[j] = std::sqrt(S[j * P + j]);
  }
  for (size_t j = 0; j < P; j++) {
    for (size_t k = 0; k < j; k++) {
      if (!coupled[j] || !coupled[k]) continue;
      const double den = root[j] * root[k];
      R[j * P + k] = S[j * P + k] / den;
    }
  }
  std::vector<double> A(P * P), T;
  double b = shrinkage;
  for (;;) {
    bool ok = false;
    if (b < 1.0) {
      const double keep = 1.0 - b;
      for (size_t j = 0; j < P; j++) {
        for (size_t k = 0; k < j; k++) A[j * P + k] = A[k * P + j] = keep * R[j * P + k];
        A[j * P + j] = 1.0;
      }
      ok = cholesky_rows(A, P, T);
    } else {
      b = 1.0;
      T.assign(P * P, 0.0);
      for (size_t j = 0; j < P; j++) T[j * P + j] = 1.0;
      ok = true;
    }
    if (ok) break;
    b = b + b;
  }
  for (size_t i = 0; i < P; i++) {
    for (size_t j = 0; j < P; j++) {
      const bool live = j <= i && new_widths[i] > 0 && new_widths[j] > 0;
      factor[j * P + i] = live ? (double)new_widths[i] * T[i * P + j] : 0.0;
    }
  }
  return b;
}

}  // namespace sxproposal
