// fit_spectra.h -- what plot_fit draws (src/plots.cpp:150-302), without the drawing: per data set and observable the
// fitted signals' spectra, their sum and the histogrammed data, and their JSON files.
#pragma once

#include <cerrno>
#include <cstdio>
#include <fstream>
#include <set>
#include <string>
#include <vector>

#include <sys/stat.h>

#include "fit_types.h"

namespace sxmc {

/** One signal's PDF at the shown parameters, scaled to its fitted number of events and projected onto one observable. */
struct SignalSpectrum {
  std::string name;
  double nexp = 0;
  std::vector<double> spectrum;
};

/** What plot_fit draws for one data set and observable (plots.cpp:255-300). */
struct FitSpectrum {
  std::string observable;   //!< its name
  unsigned dataset = 0;
  double lower = 0, upper = 0;
  size_t bins = 0;
  std::vector<SignalSpectrum> signals;     //!< the data set's signals, in signal order
  std::vector<double> fit;                 //!< their sum, added in that order
  std::vector<unsigned long long> data;    //!< the data set's events, histogrammed
};
typedef std::vector<FitSpectrum> FitSpectra;   //!< data sets ascending, per data set the observables in their order

namespace detail {

/** Every signal's PDF at `params` (their count checked by the caller), evaluated and projected onto every observable on
 *  the device: [signal][observable][bin], scaled to the signal's fitted number of events, which goes to nexps[signal].
 *  The evaluators' buffers are un-bound on every way out. */
inline std::vector<std::vector<std::vector<double>>> signal_spectra(const std::vector<double>& params, size_t nsources,
                                                                    std::vector<Signal>& signals,
                                                                    const std::vector<Observable>& observables,
                                                                    std::vector<double>& nexps) {
  const size_t npars = params.size();
  pdfz::Array<double> param_buffer(npars, true);
  std::vector<float> shown(npars);
  for (size_t p = 0; p < npars; p++) {
    shown[p] = (float)params[p];
    param_buffer.writeOnlyHostPtr()[p] = (double)shown[p];
  }
  pdfz::Array<unsigned> norms_buffer(signals.size(), true);
  norms_buffer.writeOnlyHostPtr();

  std::vector<std::vector<std::vector<double>>> spectra(signals.size());
  nexps.assign(signals.size(), 0.0);
  for (size_t i = 0; i < signals.size(); i++) {
    Signal& sig = signals[i];
    pdfz::Eval* ev = sig.histogram;
    ev->SetParameterBuffer(&param_buffer, (int)nsources);
    ev->SetNormalizationBuffer(&norms_buffer, (int)i);
    try {
      ev->EvalAsync(false);
      ev->EvalFinished();
      const double eff = 1.0 * norms_buffer.readOnlyHostPtr()[i] / (double)sig.n_mc;
      const double nexp = sig.nexpected * eff * shown[sig.source.index];
      nexps[i] = nexp;
      pdfz::EvalHist* hist = dynamic_cast<pdfz::EvalHist*>(ev);
      for (const Observable& o : observables) {
        std::vector<double> sp(o.bins, 0.0);
        if (hist) {
          const std::vector<unsigned long long> counts = hist->ProjectCounts((int)o.field_index);
          unsigned long long total = 0;
          for (unsigned long long c : counts) total += c;
          if (total > 0) {
            const double scale = nexp / (double)total;
            for (size_t j = 0; j < sp.size(); j++) sp[j] = (double)counts[j] * scale;
          }
        } else {
          const std::vector<double> m = ev->Project((int)o.field_index, (int)o.bins);
          for (size_t j = 0; j < sp.size(); j++) sp[j] = m[j] * nexp;
        }
        spectra[i].push_back(sp);
      }
    } catch (...) {
      ev->ForgetBuffers();
      throw;
    }
    ev->ForgetBuffers();   // the two arrays above die with this call
  }
  return spectra;
}

}  // namespace detail

/** plot_fit without ROOT (plots.cpp:150-302).  params: the P parameter values to show (the intervals' point estimates),
 *  held as floats as there.  Per signal (:205-227): parameters (double)(float)params[p] bound at offset nsources,
 *  EvalAsync(false), eff = norm / n_mc, nexp = nexpected * eff * params[source.index], then per observable
 *  spectrum = Project(...) * nexp -- for a histogram signal counts * (nexp / sum of counts), TH1::Scale's arithmetic
 *  on the integers; all zeros when the PDF is empty.  The projections are made on the device (EvalHist::ProjectCounts,
 *  EvalKernel::Project): no histogram is copied to the host.  data: rows of nobservables + 1 floats; an event with
 *  lower <= x < upper is counted in bin (int)(bins * ((double)x - lower) / (upper - lower)) (TAxis::FindBin), under-
 *  and overflow are not (nor a value whose quotient rounds up to `bins`: ROOT's overflow bin).  The evaluators'
 *  buffers are un-bound on return. */
inline FitSpectra fit_spectra(const std::vector<double>& params, std::vector<Source>& sources,
                              std::vector<Signal>& signals, std::vector<Systematic>& systematics,
                              std::vector<Observable>& observables, const std::set<unsigned>& datasets,
                              const std::vector<float>& data) {
  size_t npars = sources.size();
  for (const Systematic& s : systematics) npars += s.npars;
  if (params.size() != npars) {
    throw pdfz::Error("fit_spectra: " + std::to_string(params.size()) + " parameter values for " +
                      std::to_string(npars) + " parameters");
  }
  std::vector<double> nexps;
  const std::vector<std::vector<std::vector<double>>> spectra =
      detail::signal_spectra(params, sources.size(), signals, observables, nexps);
  const size_t nobs = observables.size(), row = nobs + 1;
  FitSpectra out;
  for (unsigned ds : datasets) {
    for (size_t k = 0; k < nobs; k++) {
      const Observable& o = observables[k];
      FitSpectrum f;
      f.observable = o.name;
      f.dataset = ds;
      f.lower = (double)o.lower;
      f.upper = (double)o.upper;
      f.bins = o.bins;
      f.fit.assign(o.bins, 0.0);
      f.data.assign(o.bins, 0ull);
      for (size_t i = 0; i < signals.size(); i++) {
        if (signals[i].dataset != ds) continue;
        f.signals.push_back(SignalSpectrum{signals[i].name, nexps[i], spectra[i][k]});
        for (size_t j = 0; j < o.bins; j++) f.fit[j] = f.fit[j] + spectra[i][k][j];
      }
      for (size_t e = 0; e + row <= data.size(); e += row) {
        if ((unsigned)data[e + nobs] != ds) continue;
        const double x = (double)data[e + o.field_index];
        if (!(x >= f.lower && x < f.upper)) continue;
        const long long bin = (long long)((double)o.bins * (x - f.lower) / (f.upper - f.lower));
        if (bin >= 0 && bin < (long long)o.bins) f.data[(size_t)bin]++;
      }
      out.push_back(f);
    }
  }
  return out;
}

/** The spectra as one <observable name>_<dataset>.json per observable and data set in `dir` (created if missing): the
 *  file names of plot_fit (plots.cpp:297-299).  One object per file: observable, dataset, lower, upper, bins,
 *  signals [{name, nexp, spectrum}], fit, data; numbers with 17 significant digits (a double survives the round
 *  trip).  Nothing calls this by default.  Returns the paths. */
inline std::vector<std::string> write_fit_spectra(const std::string& dir, const FitSpectra& spectra) {
  auto quoted = [](const std::string& s) {
    std::string q = "\"";
    for (char c : s) {
      if (c == '"' || c == '\\') q += '\\';
      q += c;
    }
    return q + "\"";
  };
  auto number = [](double v) {
    char buf[64];
    std::snprintf(buf, sizeof buf, "%.17g", v);
    return std::string(buf);
  };
  auto array = [&](const std::vector<double>& v) {
    std::string a = "[";
    for (size_t j = 0; j < v.size(); j++) a += (j ? ", " : "") + number(v[j]);
    return a + "]";
  };
  if (::mkdir(dir.c_str(), 0777) != 0 && errno != EEXIST) throw pdfz::Error("cannot create directory " + dir);
  std::vector<std::string> paths;
  for (const FitSpectrum& f : spectra) {
    const std::string path = dir + "/" + f.observable + "_" + std::to_string(f.dataset) + ".json";
    std::ofstream os(path);
    os << "{\n  \"observable\": " << quoted(f.observable) << ",\n  \"dataset\": " << f.dataset
       << ",\n  \"lower\": " << number(f.lower) << ",\n  \"upper\": " << number(f.upper)
       << ",\n  \"bins\": " << f.bins << ",\n  \"signals\": [\n";
    for (size_t i = 0; i < f.signals.size(); i++) {
      os << "    {\"name\": " << quoted(f.signals[i].name) << ", \"nexp\": " << number(f.signals[i].nexp)
         << ", \"spectrum\": " << array(f.signals[i].spectrum) << "}" << (i + 1 < f.signals.size() ? ",\n" : "\n");
    }
    os << "  ],\n  \"fit\": " << array(f.fit) << ",\n  \"data\": [";
    for (size_t j = 0; j < f.data.size(); j++) os << (j ? ", " : "") << f.data[j];
    os << "]\n}\n";
    os.close();
    if (!os) throw pdfz::Error("cannot write " + path);
    paths.push_back(path);
  }
  return paths;
}

}  // namespace sxmc
