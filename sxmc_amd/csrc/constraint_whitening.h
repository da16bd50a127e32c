// constraint_whitening.h -- correlated Gaussian constraints (include/sxmc_hip.h, sxmc_constraint_whitening): the
// validation of a correlation matrix and its whitening matrix W = T^-1, T the Cholesky factor.  Pure host code, no
// device, no library state: the one implementation behind the C entry point, which both walkers and both loaders call.
// The law is replayed by tests/step_reference_constraints.py, which this file is held to bit for bit: every operation
// below is a separate double operation (build with -ffp-contract=off), every sum sequential.
//
// THE ORDER OF OPERATIONS (rho row-major, P x P; every assignment one rounding):
//   T, row by row (Cholesky-Banachiewicz): for i = 0 .. P-1, for j = 0 .. i:
//       s = rho[i][j];  for k = 0 .. j-1 ascending:  prod = T[i][k] * T[j][k];  s = s - prod;
//       j == i:  the pivot s must be > 0 ("not positive definite at parameter i");  T[i][i] = sqrt(s)
//       j <  i:  T[i][j] = s / T[j][j]
//   W = T^-1, row by row (forward substitution): for i = 0 .. P-1:
//       W[i][i] = 1 / T[i][i]
//       for j = 0 .. i-1:  s = 0;  for k = j .. i-1 ascending:  prod = T[i][k] * W[k][j];  s = s + prod;
//                          q = s * W[i][i];  W[i][j] = -q      (the reciprocal formed once per row, not a division per
//                          entry: rho = [[1, -0.6], [-0.6, 1]] gives exactly W = [[1, 0], [0.75, 1.25]])
//   A product whose T factor is exactly zero is skipped in both loops (adding or subtracting an exact +-0 changes no
//   sum that is not itself zero, and the skipped sums start at +0): rows of the identity cost nothing, and a parameter
//   outside every correlated group has W[i][i] = 1 and zeros beside it, with no -0.0 among them.
//   Output: W[i][j] at W[j * P + i] (column-major, as the proposal factor), zeros above the diagonal.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <string>
#include <vector>

namespace sxconstraint {

// Why the matrix is refused, naming the entry; empty: accepted.  sigmas: the constraints' widths (<= 0: no constraint).
inline std::string check_correlation(const double* rho, const double* sigmas, size_t P) {
  char buf[200];
  for (size_t i = 0; i < P; i++) {
    for (size_t j = 0; j < P; j++) {
      const double v = rho[i * P + j];
      if (!std::isfinite(v) || v < -1.0 || v > 1.0) {
        std::snprintf(buf, sizeof buf, "constraint correlation: entry (%zu, %zu) is not a finite number in [-1, 1]", i, j);
        return buf;
      }
    }
  }
  for (size_t i = 0; i < P; i++) {
    if (rho[i * P + i] != 1.0) {
      std::snprintf(buf, sizeof buf, "constraint correlation: diagonal entry (%zu, %zu) is not 1", i, i);
      return buf;
    }
  }
  for (size_t i = 0; i < P; i++) {
    for (size_t j = 0; j < i; j++) {
      if (rho[i * P + j] != rho[j * P + i]) {
        std::snprintf(buf, sizeof buf, "constraint correlation: not symmetric at (%zu, %zu)", i, j);
        return buf;
      }
    }
  }
  for (size_t i = 0; i < P; i++) {
    if (sigmas[i] > 0) continue;
    for (size_t j = 0; j < P; j++) {
      if (j != i && rho[i * P + j] != 0.0) {
        std::snprintf(buf, sizeof buf,
                      "constraint correlation: parameter %zu has no constraint (sigma <= 0) but entry (%zu, %zu) is not 0",
                      i, i, j);
        return buf;
      }
    }
  }
  return std::string();
}

// W (column-major, all P * P written) from an accepted rho.  Returns -1, or the parameter whose pivot is not positive.
inline long whitening(const double* rho, size_t P, double* W) {
  std::vector<double> T(P * P, 0.0), V(P * P, 0.0);   // row-major both
  for (size_t i = 0; i < P; i++) {
    for (size_t j = 0; j <= i; j++) {
      double s = rho[i * P + j];
      for (size_t k = 0; k < j; k++) {
        if (T[i * P + k] == 0.0) continue;
        const double prod = T[i * P + k] * T[j * P + k];
        s = s - prod;
      }
      if (j == i) {
        if (!(s > 0.0)) return (long)i;
        T[i * P + i] = std::sqrt(s);
      } else {
        T[i * P + j] = s / T[j * P + j];
      }
    }
  }
  for (size_t i = 0; i < P; i++) {
    const double inverse = 1.0 / T[i * P + i];
    V[i * P + i] = inverse;
    for (size_t j = 0; j < i; j++) {
      double s = 0.0;
      bool any = false;
      for (size_t k = j; k < i; k++) {
        if (T[i * P + k] == 0.0) continue;
        const double prod = T[i * P + k] * V[k * P + j];
        s = s + prod;
        any = true;
      }
      if (!any) continue;   // (stays +0)
      const double q = s * inverse;
      V[i * P + j] = -q;
    }
  }
  for (size_t i = 0; i < P; i++)
    for (size_t j = 0; j < P; j++) W[j * P + i] = V[i * P + j];
  return -1;
}

}  // namespace sxconstraint
