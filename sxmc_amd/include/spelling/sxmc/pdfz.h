// <sxmc/pdfz.h> as the reference's sources include it (mcmc.h:20): pdfz::Eval, pdfz::EvalHist and pdfz::EvalKernel
// (the kernel-density PDF, pdfz.h:578-625) exactly as sxmc_amd/include/sxmc/pdfz.h defines them.
#pragma once
#include "../hemi/array.h"
#include "../../sxmc/pdfz.h"
