// intervals.h -- what the reference takes from a sampled likelihood space, without ROOT: intervals by contour or by
// projection, the correlation matrix, and the text of the best-fit report.
//
//   LikelihoodSpace::get_contour src/likelihood.cpp:90-102
//   Contour::get_interval        src/error_estimators/contour.cpp:18-69
//   Projection::get_interval     src/error_estimators/projection.cpp:14-77
//   Interval                     src/interval.h:11-29
//   median                       src/utils.h:76-90
//
// chain.h and the standard library only: no device, no library call, so that tests/cpp/intervals_dump builds (and runs
// under the sanitizers) without libsxmc_hip.so.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iomanip>
#include <limits>
#include <map>
#include <ostream>
#include <sstream>
#include <string>
#include <vector>

#include "chain.h"

namespace sxmc {

/** interval.h:11-29 */
struct Interval {
  bool one_sided = false;
  float point_estimate = -1;
  float lower = -1;
  float upper = -1;
  float cl = -1;
  float coverage = -1;
};

/** utils.h:76-90 */
template <typename T>
T median(std::vector<T> v) {
  std::sort(v.begin(), v.end());
  const size_t half = v.size() / 2;
  return v.size() % 2 == 0 ? (T)(1.0 * (v[half - 1] + v[half]) / 2) : v[half];
}

/** TMath::ChisquareQuantile(cl, 1) = (Phi^-1((1 + cl) / 2))^2, by bisection on erf. */
inline double chisquare_quantile_1dof(double cl) {
  double lo = 0.0, hi = 40.0;
  for (int i = 0; i < 200; i++) {
    const double mid = 0.5 * (lo + hi);
    (std::erf(std::sqrt(mid / 2.0)) < cl ? lo : hi) = mid;
  }
  return 0.5 * (lo + hi);
}

/** What `ostream << float` writes (6 significant digits, %g) read back: the reference builds its selections as
 *  TEXT -- "likelihood+" << -lmin << "<" << delta (likelihood.cpp:93-94, contour.cpp:45-46) -- so the offset and
 *  the threshold it actually applies are the printed, rounded ones.  With |lmin| of a few 1e5 (BASELINE config 3)
 *  the offset is off by up to 0.5, which moves the contour; reproduced here because the intervals are results. */
inline double as_printed(float v) {
  char buf[64];
  std::snprintf(buf, sizeof buf, "%g", (double)v);
  return std::strtod(buf, nullptr);
}

/** Contour::get_interval for every parameter of a chain (contour.cpp:17-69, likelihood.cpp:90-102). */
inline std::vector<Interval> contour_intervals(const Chain& chain, float cl = 0.9f) {
  const size_t ncol = chain.names.size(), P = ncol - 1, n = chain.nrows();
  float lmin = chain.at(0, P);
  for (size_t r = 1; r < n; r++) lmin = std::min(lmin, chain.at(r, P));
  const float delta = 0.5 * chisquare_quantile_1dof(cl);   // contour.cpp:19 (a float there too)
  // likelihood.cpp:90-102: rows with likelihood + (-lmin as printed) < (delta as printed)
  std::vector<size_t> contour;
  const double off = as_printed(-lmin), dprinted = as_printed(delta);
  for (size_t r = 0; r < n; r++)
    if ((double)chain.at(r, P) + off < dprinted) contour.push_back(r);
  if (contour.empty()) {   // (the reference asserts here: the printed offset lost the minimum; use the exact one)
    for (size_t r = 0; r < n; r++)
      if (chain.at(r, P) - lmin < delta) contour.push_back(r);
  }
  // contour.cpp:39-53: points near the maximum-likelihood point, widened 0.13, 0.65, 3.25, ... until one is found;
  // the offset is the minimum over the contour points, printed the same way
  float cmin = chain.at(contour[0], P);
  for (size_t r : contour) cmin = std::min(cmin, chain.at(r, P));
  const double coff = as_printed(-cmin);
  std::vector<size_t> near;
  float dnll = 0.13f;
  do {
    near.clear();
    const double dn = as_printed(dnll);
    for (size_t r : contour)
      if ((double)chain.at(r, P) + coff < dn) near.push_back(r);
    dnll *= 5;
  } while (near.empty());
  std::vector<Interval> out(P);
  for (size_t p = 0; p < P; p++) {
    Interval iv;
    iv.cl = cl;
    iv.one_sided = false;
    iv.coverage = -999;
    float nlo = chain.at(near[0], p), nhi = nlo, clo = chain.at(contour[0], p), chi = clo;
    for (size_t r : near) {
      nlo = std::min(nlo, chain.at(r, p));
      nhi = std::max(nhi, chain.at(r, p));
    }
    for (size_t r : contour) {
      clo = std::min(clo, chain.at(r, p));
      chi = std::max(chi, chain.at(r, p));
    }
    iv.point_estimate = (nlo + nhi) / 2;
    iv.lower = clo;
    iv.upper = chi;
    out[p] = iv;
  }
  return out;
}

/** What `TH1::Fit("gaus")` minimises (projection.cpp:22-23): chi2 over the non-empty bins of
 *  ((n_i - A exp(-(x_i - mu)^2 / (2 sigma^2))) / sqrt(n_i))^2, the function taken at the bin centre, started from
 *  the histogram's maximum, mean and RMS (TH1's InitGaus).  Levenberg-Marquardt here, Minuit MIGRAD in ROOT: the
 *  same minimum.  false when it does not converge to a positive width. */
inline bool gaus_fit(const std::vector<double>& centers, const std::vector<double>& counts, double& A, double& mu,
                     double& sigma) {
  std::vector<double> x, y;
  for (size_t i = 0; i < centers.size(); i++)
    if (counts[i] > 0) {
      x.push_back(centers[i]);
      y.push_back(counts[i]);
    }
  const size_t n = x.size();
  if (n < 3) return false;
  double sy = 0, sxy = 0, ymax = 0;
  for (size_t i = 0; i < n; i++) {
    sy += y[i];
    sxy += x[i] * y[i];
    ymax = std::max(ymax, y[i]);
  }
  const double mean = sxy / sy;
  double var = 0;
  for (size_t i = 0; i < n; i++) var += y[i] * (x[i] - mean) * (x[i] - mean);
  const double rms = std::sqrt(std::max(var / sy, 0.0));
  if (!(rms > 0)) return false;
  double p[3] = {ymax, mean, rms};
  auto chi2_of = [&](const double* q) {
    if (!(q[2] > 0)) return std::numeric_limits<double>::infinity();
    double c = 0;
    for (size_t i = 0; i < n; i++) {
      const double z = (x[i] - q[1]) / q[2], r = (y[i] - q[0] * std::exp(-0.5 * z * z)) / std::sqrt(y[i]);
      c += r * r;
    }
    return c;
  };
  double lam = 1e-3, chi2 = chi2_of(p);
  for (int it = 0; it < 200; it++) {
    double a[3][3] = {{0}}, b[3] = {0};
    for (size_t i = 0; i < n; i++) {
      const double e = std::sqrt(y[i]), d = x[i] - p[1], g = std::exp(-0.5 * d * d / (p[2] * p[2]));
      const double j[3] = {g / e, p[0] * g * d / (p[2] * p[2]) / e, p[0] * g * d * d / (p[2] * p[2] * p[2]) / e};
      const double r = (y[i] - p[0] * g) / e;
      for (int u = 0; u < 3; u++) {
        b[u] += j[u] * r;
        for (int v = 0; v < 3; v++) a[u][v] += j[u] * j[v];
      }
    }
    double m[3][4];
    for (int u = 0; u < 3; u++) {
      for (int v = 0; v < 3; v++) m[u][v] = a[u][v] + (u == v ? lam * (a[u][u] + 1e-300) : 0.0);
      m[u][3] = b[u];
    }
    bool singular = false;
    for (int c = 0; c < 3 && !singular; c++) {   // Gauss-Jordan with partial pivoting
      int piv = c;
      for (int r = c + 1; r < 3; r++)
        if (std::fabs(m[r][c]) > std::fabs(m[piv][c])) piv = r;
      if (m[piv][c] == 0.0) singular = true;
      for (int k = 0; k < 4 && !singular; k++) std::swap(m[c][k], m[piv][k]);
      for (int r = 0; r < 3 && !singular; r++) {
        if (r == c) continue;
        const double f = m[r][c] / m[c][c];
        for (int k = c; k < 4; k++) m[r][k] -= f * m[c][k];
      }
    }
    if (singular) return false;
    const double step[3] = {m[0][3] / m[0][0], m[1][3] / m[1][1], m[2][3] / m[2][2]};
    const double trial[3] = {p[0] + step[0], p[1] + step[1], p[2] + step[2]};
    const double c2 = chi2_of(trial);
    if (c2 <= chi2) {
      bool small = chi2 - c2 <= 1e-12 * std::max(chi2, 1e-300);
      for (int u = 0; u < 3; u++) small = small && std::fabs(step[u]) <= 1e-10 * (std::fabs(p[u]) + 1e-300);
      for (int u = 0; u < 3; u++) p[u] = trial[u];
      chi2 = c2;
      lam = std::max(lam * 0.3, 1e-12);
      if (small) break;
    } else {
      lam *= 10.0;
      if (lam > 1e12) break;
    }
  }
  if (!(p[2] > 0) || !std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) return false;
  A = p[0];
  mu = p[1];
  sigma = p[2];
  return true;
}

/** Projection::get_interval on one parameter's samples (projection.cpp:14-77): histogram (ROOT's TTree::Draw
 *  picks range and binning by its own "nice limits" rule, not reproduced: `nbins` bins over [min, max] here),
 *  Gaussian fit for the point estimate, limits walked outwards from the mean's bin until cl / 2 of the samples
 *  lie on either side (one-sided from the low edge when less than cl / 2 lies below the mean). */
inline Interval projection_interval(const std::vector<float>& values, float cl = 0.9f, int nbins = 100) {
  Interval iv;
  iv.cl = cl;
  double lo = values.at(0), hi = lo;
  for (float v : values) {
    lo = std::min<double>(lo, v);
    hi = std::max<double>(hi, v);
  }
  if (!(hi > lo)) {
    iv.point_estimate = iv.lower = (float)lo;
    iv.upper = (float)hi;
    iv.coverage = 1;
    return iv;
  }
  const double width = (hi - lo) / nbins;
  std::vector<double> counts((size_t)nbins, 0.0), centers((size_t)nbins), csum((size_t)nbins + 1, 0.0);
  // TH1 conventions (TAxis::FindBin): bin = 1 + int(nbins (x - xmin) / (xmax - xmin)); the maximum counts in the last bin
  for (float v : values) counts[(size_t)std::min<long>(nbins - 1, (long)(nbins * ((double)v - lo) / (hi - lo)))] += 1;
  for (int i = 0; i < nbins; i++) centers[(size_t)i] = lo + (i + 0.5) * width;
  double total = 0;
  for (int i = 0; i < nbins; i++) csum[(size_t)i + 1] = (total += counts[(size_t)i]);   // csum[i] = bins 1..i
  double a = 0, mu = 0, sigma = 0;
  if (!gaus_fit(centers, counts, a, mu, sigma)) {
    mu = centers[(size_t)(std::max_element(counts.begin(), counts.end()) - counts.begin())];
  }
  // 1-based bin of the mean (TH1::FindBin): 0 below the range, nbins + 1 at or beyond its end
  long imax = mu < lo ? 0 : mu >= hi ? nbins + 1 : 1 + (long)(nbins * (mu - lo) / (hi - lo));
  if (imax < 1) {                                         // projection.cpp:28-31
    imax = 1;
    mu = lo;
  }
  imax = std::min<long>(imax, nbins);
  long ilo = 1, ihi = 0;
  if (csum[(size_t)imax] / total < cl / 2) {              // projection.cpp:36-45
    iv.one_sided = true;
    for (long i = 0; i <= nbins; i++)
      if (csum[(size_t)i] / total >= cl) {
        ihi = i;
        break;
      }
  } else {
    iv.one_sided = false;
    for (long i = imax; i > 0; i--)
      if ((csum[(size_t)imax] - csum[(size_t)i - 1]) / total >= cl / 2) {
        ilo = i;
        break;
      }
    for (long i = imax + 1; i <= nbins; i++)
      if ((csum[(size_t)i] - csum[(size_t)imax]) / total >= cl / 2) {
        ihi = i;
        break;
      }
  }
  ihi = ihi ? std::max(ihi, ilo) : nbins;
  iv.point_estimate = (float)mu;
  iv.coverage = (float)((csum[(size_t)ihi] - csum[(size_t)ilo - 1]) / total);
  iv.lower = (float)(lo + (ilo - 1) * width);
  iv.upper = (float)(lo + (ihi - 1) * width + width);   // projection.cpp:73: GetBinLowEdge(ihi) + GetBinWidth(ihi)
  return iv;
}

/** Projection::get_interval for every parameter of a chain. */
inline std::vector<Interval> projection_intervals(const Chain& chain, float cl = 0.9f) {
  const size_t P = chain.names.size() - 1;
  std::vector<Interval> out;
  for (size_t p = 0; p < P; p++) {
    std::vector<float> col;
    for (size_t r = 0; r < chain.nrows(); r++) col.push_back(chain.at(r, p));
    out.push_back(projection_interval(col, cl));
  }
  return out;
}

/** error_estimator.h: how the intervals are taken from the sampled likelihood space (fit.error_type). */
enum ErrorType { ERROR_CONTOUR, ERROR_PROJECTION };

/** LikelihoodSpace::extract_best_fit (likelihood.cpp:104-137): every parameter's interval by the chosen estimator. */
inline std::vector<Interval> extract_intervals(const Chain& chain, float cl, ErrorType error_type) {
  return error_type == ERROR_PROJECTION ? projection_intervals(chain, cl) : contour_intervals(chain, cl);
}

/** Interval::str (interval.cpp:6-20): "point -lower_error +upper_error", or "point <upper (cl% CL)". */
inline std::string interval_str(const Interval& iv) {
  const float lower_error = iv.point_estimate - iv.lower, upper_error = iv.upper - iv.point_estimate;
  std::ostringstream ss;
  ss << iv.point_estimate;
  if (iv.one_sided) ss << " <" << iv.upper << " (" << 100 * iv.cl << "% CL)";
  else ss << " -" << lower_error << " +" << upper_error;
  return ss.str();
}

/** get_correlation_matrix (utils.cpp:29-77) of a chain's parameter columns (every column but `likelihood`), row-major
 *  [P][P].  As there: sums, means and products accumulate in float in row order, the square root is taken in double,
 *  and only the diagonal and what is to the right of it is computed -- the entries below stay 0. */
inline std::vector<float> correlation_matrix(const Chain& chain) {
  const size_t P = chain.names.size() - 1, n = chain.nrows();
  std::vector<float> matrix(P * P, 0.0f), means(P, 0.0f);
  for (size_t k = 0; k < n; k++)
    for (size_t j = 0; j < P; j++) means[j] += chain.at(k, j);
  for (size_t j = 0; j < P; j++) means[j] /= (int)n;
  for (size_t i = 0; i < P; i++) {
    for (size_t j = i; j < P; j++) {
      float t = 0, dx2 = 0, dy2 = 0;
      for (size_t k = 0; k < n; k++) {
        const float x1 = chain.at(k, i) - means[i], x2 = chain.at(k, j) - means[j];
        t += x1 * x2;
        dx2 += x1 * x1;
        dy2 += x2 * x2;
      }
      matrix[i * P + j] = (float)(t / std::sqrt((double)(dx2 * dy2)));
    }
  }
  return matrix;
}

/** LikelihoodSpace::print_best_fit (likelihood.cpp:34-45): the parameters in NAME order (a std::map there), then
 *  the minimum of the likelihood column (likelihood.cpp:134). */
inline void print_best_fit(std::ostream& os, const Chain& chain, const std::vector<Interval>& intervals) {
  const size_t P = chain.names.size() - 1;
  std::map<std::string, Interval> by_name;
  for (size_t p = 0; p < P && p < intervals.size(); p++) by_name[chain.names[p]] = intervals[p];
  os << "-- Best fit --" << std::endl;
  for (const auto& kv : by_name) {
    if (kv.first == "likelihood") continue;
    os << " " << kv.first << ": " << interval_str(kv.second) << std::endl;
  }
  float lmin = chain.nrows() ? chain.at(0, P) : 0.0f;
  for (size_t r = 1; r < chain.nrows(); r++) lmin = std::min(lmin, chain.at(r, P));
  os << " NLL: " << lmin << std::endl;
}

/** LikelihoodSpace::print_correlations (likelihood.cpp:48-72): names in column order, right-aligned to the longest,
 *  entries fixed with three decimals in eight columns. */
inline void print_correlations(std::ostream& os, const Chain& chain) {
  const size_t P = chain.names.size() - 1;
  const std::vector<float> c = correlation_matrix(chain);
  os << "-- Correlation matrix --" << std::endl;
  int maxlen = 0;
  for (size_t i = 0; i < P; i++) maxlen = std::max(maxlen, (int)chain.names[i].length());
  for (size_t i = 0; i < P; i++) {
    os << std::setw(maxlen) << chain.names[i] << " ";
    for (size_t j = 0; j < P; j++) {
      os << std::setiosflags(std::ios::fixed) << std::setprecision(3) << std::setw(8) << c[j + i * P];
    }
    os << std::resetiosflags(std::ios::fixed) << std::endl;
  }
}

}  // namespace sxmc
