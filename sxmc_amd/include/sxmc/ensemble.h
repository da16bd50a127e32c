// ensemble.h -- ROOT-free forms of the code around the MCMC driver in the reference's experiment loop
// (src/sxmc.cpp:44-145): fake data sets, interval extraction, the loop itself.
//
//   make_fake_dataset            src/generator.cpp:10-48
//   EvalHist::RandomSample       src/pdfz.cpp:817-922 (TH1::GetRandom / GetRandom2 / GetRandom3: pick a bin
//                                with probability proportional to its content, then uniform inside the bin)
//   LikelihoodSpace::get_contour src/likelihood.cpp:90-102
//   Contour::get_interval        src/error_estimators/contour.cpp:18-69
//   Interval                     src/interval.h:11-29
//   median                       src/utils.h:76-90
//   plot_fit                     src/plots.cpp:150-302 (fit_spectra: the spectra without the drawing)
//
// Parity with the reference is statistical only: these draw on ROOT's generators and TMath, and the
// reference holds no test for them.  Deviates come from std::mt19937_64 here.  Experiments are
// independent, so a multi-GPU run gives experiment k to rank k mod G (sxmc_amd/dist.py) and gathers
// the intervals once at the end.
//
// By concern:
//   chain.h          the sampled likelihood space (also what mcmc.h returns)
//   intervals.h      intervals, correlations, the best-fit report -- chain.h and the standard library only
//   fake_data.h      the host samplers and make_fake_dataset
//   lane_sync.h      LaneBarrier, Rendezvous -- the standard library only
//   experiment.h     the hooks, one experiment, ensemble / ensemble_concurrent / ensemble_lockstep and their options
//   ensemble_plan.h  how experiments and their intervals are shared among ranks -- the standard library only
//   multi_gpu.h      ensemble_multi_gpu
//   fit_spectra.h    fit_spectra, write_fit_spectra
#pragma once

#include "chain.h"
#include "ensemble_plan.h"
#include "experiment.h"
#include "fake_data.h"
#include "fit_spectra.h"
#include "intervals.h"
#include "lane_sync.h"
#include "multi_gpu.h"
