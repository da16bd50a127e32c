/*
 * sxmc_hip.h -- C ABI of libsxmc_hip.so: the MI355X (gfx950) implementation of sxmc's per-step
 * NLL evaluation (pdfz::EvalHist histogram fill with per-sample systematics + the nll_kernels
 * event log-sum, reduction and fused MCMC step).
 *
 * This is the drop-in boundary: plain pointers and sizes, `int` status returns, no exceptions,
 * no torch or C++ types.  Each entry point names the reference interface it replaces
 * (file:line relative to /root/reference).  The C++ mirror of the reference's own classes
 * (pdfz::Eval, pdfz::EvalHist, the device-mirror array and the kernel launch points mcmc.cpp
 * uses) lives in sxmc_amd/include/sxmc/ and is a header-only layer over this ABI.
 *
 * Unless stated otherwise pointers named `d_*` or documented "device" are HIP device pointers
 * (hipMalloc'd, or any pointer valid on the current device such as a torch tensor's data_ptr),
 * and everything else is host memory.  All functions return SXMC_OK (0) or an error code;
 * sxmc_last_error() returns the message of the last failure on the calling thread.
 */
#ifndef SXMC_HIP_H
#define SXMC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SXMC_OK 0
#define SXMC_ERR_INVALID 1 /* argument validation failed: where the reference throws pdfz::Error */
#define SXMC_ERR_HIP 2     /* a HIP runtime call failed (reference: checkCuda) */
#define SXMC_ERR_STATE 3   /* call sequence error, e.g. eval before the buffers are bound */
#define SXMC_ERR_SHAPE 4   /* a shape the requested form has no kernel for (a proposal factor or whitening matrix beyond 256 parameters) */

#define SXMC_MAX_NFIELDS 10   /* pdfz.cpp:17 MAX_NFIELDS */
#define SXMC_MAX_SYST 16      /* systematics per evaluator (reference: unbounded array, pdfz.cpp:126-132) */
#define SXMC_MAX_SYST_PARS 8  /* polynomial coefficients per systematic */

/* pdfz.h:111-116 Systematic::Type */
#define SXMC_SYST_SHIFT 0
#define SXMC_SYST_SCALE 1
#define SXMC_SYST_RESOLUTION_SCALE 2
#define SXMC_SYST_CTSCALE 3

typedef struct sxmc_hist* sxmc_hist_t;   /* one pdfz::EvalHist (pdfz.h:402-574) */
typedef struct sxmc_group* sxmc_group_t; /* the set of evaluators MCMC steps together (mcmc.cpp:264-271) */
typedef void* sxmc_stream_t;             /* hipStream_t; NULL = the legacy default stream */
typedef void* sxmc_event_t;              /* hipEvent_t */

/* Counter-based generator state, one per parameter.  Replaces curandStateXORWOW
 * (nll_kernels.h:25-29 RNGState).  Philox4x32-10 keyed by `seed`, stream `subsequence`. */
typedef struct {
  uint64_t seed;
  uint64_t subsequence;
  uint64_t offset; /* draws consumed so far */
  uint64_t reserved;
} sxmc_rng_state;

/* ---------------------------------------------------------------- runtime / memory ---------- */
/* Replaces hemi's checkCuda error reporting. */
const char* sxmc_last_error(void);
const char* sxmc_version(void);

int sxmc_device_count(int* count);
int sxmc_set_device(int device);
int sxmc_get_device(int* device); /* the calling thread's current device */
/* name: at least 256 bytes. */
int sxmc_device_info(int device, char* name, int* compute_units, size_t* hbm_bytes,
                     int* lds_bytes_per_cu, int* clock_khz);
/* Host-side roctx ranges around the phases of a step (launch plan, fill, step end, SetEvalPoints, graph replay), for
 * rocprofv3 --marker-trace beside --kernel-trace.  Off by default; SXMC_ROCTX=1 in the environment turns them on too. */
int sxmc_set_tracing(int enable);
int sxmc_device_synchronize(void);
/* PCI bus id of a device ("0000:05:00.0"): tells two ranks on ONE card from two ranks on two cards of the same name. */
int sxmc_device_pci_bus_id(int device, char* out, size_t out_bytes);
/* Free and total device memory in bytes (hipMemGetInfo). */
int sxmc_mem_info(size_t* free_bytes, size_t* total_bytes);

/* Device side of hemi::Array<T>: allocation and the two copy directions
 * its accessors perform implicitly. */
int sxmc_malloc(void** d_ptr, size_t bytes);
int sxmc_free(void* d_ptr);
int sxmc_host_alloc(void** h_ptr, size_t bytes); /* pinned; hemi::Array(n, pinned=true) */
int sxmc_host_free(void* h_ptr);
int sxmc_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes);
int sxmc_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes);
int sxmc_memcpy_d2d(void* d_dst, const void* d_src, size_t bytes);
int sxmc_memcpy_h2d_async(void* d_dst, const void* h_src, size_t bytes, sxmc_stream_t s);
int sxmc_memcpy_d2h_async(void* h_dst, const void* d_src, size_t bytes, sxmc_stream_t s);
int sxmc_memset(void* d_dst, int value, size_t bytes);

/* cudaStreamCreate / cudaStreamSynchronize (pdfz.cpp:91, 493) */
int sxmc_stream_create(sxmc_stream_t* s);
/* A stream that does not synchronise with the legacy default stream: one per concurrent chain. */
int sxmc_stream_create_nonblocking(sxmc_stream_t* s);
int sxmc_stream_destroy(sxmc_stream_t s);
int sxmc_stream_synchronize(sxmc_stream_t s);
/* *done = 1 when everything queued on `s` has finished, 0 while work is pending (hipStreamQuery): lets a host thread
 * wait for a collective WITHOUT blocking inside the runtime, so that it can give up when a peer has failed. */
int sxmc_stream_query(sxmc_stream_t s, int* done);

/* HIP-graph capture of a launch sequence (the per-step sequence of mcmc.cpp:264-348 is the
 * same launches with the same arguments every step, so it can be recorded once and replayed).
 * Between begin and end, every sxmc_group_* evaluation and sxmc_launch_* call given `s` is recorded
 * instead of executed; `s` must be a created stream (the legacy default stream cannot be captured).
 * The group must already have evaluated once with its current configuration (descriptor uploads cannot
 * be recorded: SXMC_ERR_STATE otherwise), and a recorded graph is only valid until an evaluator of the
 * group changes (systematics, evaluation points, bindings, launch configuration).  Kernel arguments are
 * frozen at capture: device buffers are re-read at replay, scalar arguments are not.
 * Host threads: while one thread records, no other thread may allocate, free, copy through the legacy
 * default stream or synchronise the device (the ROCm runtime refuses those calls and fails the
 * recording); launching, and waiting on or copying through its own non-blocking stream, is fine.  A
 * program with one chain per host thread serialises set-up, recording and tear-down with a mutex
 * (sxmc::MCMC::exclusive, sxmc::ensemble_concurrent). */
typedef void* sxmc_graph_t;              /* hipGraphExec_t */
int sxmc_graph_begin_capture(sxmc_stream_t s);
int sxmc_graph_end_capture(sxmc_stream_t s, sxmc_graph_t* out);
/* Replays the recorded sequence `times` times on `s` (asynchronous). */
int sxmc_graph_launch(sxmc_graph_t graph, sxmc_stream_t s, int times);
int sxmc_graph_destroy(sxmc_graph_t graph);

int sxmc_event_create(sxmc_event_t* e);
int sxmc_event_destroy(sxmc_event_t e);
int sxmc_event_record(sxmc_event_t e, sxmc_stream_t s);
int sxmc_event_synchronize(sxmc_event_t e);
int sxmc_event_elapsed_ms(sxmc_event_t start, sxmc_event_t stop, float* ms);

/* ---------------------------------------------------------------- pdfz::EvalHist ------------ */
/* EvalHist::EvalHist + Eval::Eval (pdfz.cpp:57-97, 179-236).
 * samples: row-major [nsamples_floats / nfields][nfields] float32; host memory, or device
 * memory when samples_on_device != 0.  The evaluator keeps its own column-major copy
 * (the reference also copies, pdfz.cpp:197).  n_lower/n_upper/n_nbins are the lengths of the
 * three arrays so that the reference's size validation can be reproduced:
 * SXMC_ERR_INVALID for every condition under which the reference throws pdfz::Error
 * (pdfz.cpp:64-82, 189-195, 217-219) and additionally for upper[i] <= lower[i], nbins[i] < 0. */
int sxmc_hist_create(const float* samples, size_t nsamples_floats, int samples_on_device,
                     int nfields, int nobservables,
                     const double* lower, size_t n_lower,
                     const double* upper, size_t n_upper,
                     const int* nbins, size_t n_nbins,
                     unsigned dataset, sxmc_hist_t* out);
/* A second evaluator over the SAME sample table as `base` (shared, reference counted; nothing is
 * copied): own histogram, evaluation points, bindings and stream, systematics copied from `base`.
 * For several chains / fake experiments running concurrently on one GPU (BASELINE config 4: one
 * experiment per stream) without holding the MC tables more than once. */
int sxmc_hist_create_shared(sxmc_hist_t base, sxmc_hist_t* out);
/* EvalHist::~EvalHist (pdfz.cpp:239-242); also destroys the evaluator's stream, which the
 * reference leaks (pdfz.cpp:100-103). */
int sxmc_hist_destroy(sxmc_hist_t h);

/* Eval::AddSystematic (pdfz.cpp:126-174).  `pars` are indices into the parameter buffer
 * (npars of them, host memory, copied).  extra_field is used by RESOLUTION_SCALE only. */
int sxmc_hist_add_systematic(sxmc_hist_t h, int type, int obs, int extra_field,
                             int npars, const short* pars);

/* EvalHist::SetEvalPoints (pdfz.cpp:245-302).  points: host, rows of nobservables+1 floats
 * (last = dataset id).  SXMC_ERR_INVALID if npoints_floats % (nobservables+1) != 0.
 * The evaluator's previous evaluations must have finished (as for the reference: it replaces the arrays they
 * read).  A new data set that fits the buffers of the previous one -- every fake experiment after the first --
 * costs one host-to-device copy: no device-wide synchronisation and no allocation, so other chains running on
 * the same GPU are not stalled, and the groups the evaluator belongs to patch their descriptors instead of
 * re-planning their launches. */
int sxmc_hist_set_eval_points(sxmc_hist_t h, const float* points, size_t npoints_floats);

/* Eval::SetPDFValueBuffer / SetNormalizationBuffer / SetParameterBuffer (pdfz.cpp:106-124).
 * Device pointers, borrowed: they must outlive every evaluation that uses them. */
int sxmc_hist_set_pdf_value_buffer(sxmc_hist_t h, float* d_output, int offset, int stride);
int sxmc_hist_set_normalization_buffer(sxmc_hist_t h, unsigned* d_norm, int offset);
int sxmc_hist_set_parameter_buffer(sxmc_hist_t h, const double* d_params, int offset, int stride);

/* EvalHist::EvalAsync / EvalFinished (pdfz.cpp:441-495): zero, fill, (evaluate); eval_async returns before
 * completion, eval_finished when the evaluator's results are in its bound buffers.
 * TRANSPARENT BATCHING.  The reference's callers evaluate their S signals as "EvalAsync on all, then EvalFinished on
 * all" (mcmc.cpp:264-271, bench_sxmc.cpp:193-200).  Launched one by one that is S full-grid fills with S fixed
 * costs; so sxmc_hist_eval_async DEFERS: the evaluator joins the calling host thread's batch, and the batch is
 * launched as ONE group evaluation (what sxmc_group_eval_async does: one zero, ONE fill over all members' samples, one
 * lookup) -- at once when the last evaluator of a batch seen before has arrived (so the device works while the caller
 * goes on, as with the reference), otherwise at the first call that could tell the difference: sxmc_hist_eval_finished
 * of a member, any copy, launch, synchronisation or stream query through this ABI, a change of a member's bindings,
 * systematics or points, its destruction.  Results are identical (integer counters; the lookup is per evaluator).  An
 * unchanged mcmc.cpp gets the batched fill this way; the explicit group API below remains for callers that want
 * more (fused lookup + event sum, fused step end, HIP-graph replay).  A batch is per host thread: EvalFinished must
 * come from the thread that called EvalAsync (SXMC_ERR_STATE otherwise).  While a HIP graph is being recorded on the
 * calling thread, and after sxmc_set_deferred_eval(0) (or SXMC_DEFER_EVAL=0 in the environment), evaluations are
 * launched as asked: each at once, on its evaluator's own stream. */
int sxmc_hist_eval_async(sxmc_hist_t h, int do_eval_pdf);
int sxmc_hist_eval_finished(sxmc_hist_t h);
/* 0: sxmc_hist_eval_async launches at once on the evaluator's own stream (S separate launch sequences for S
 * evaluators: the reference's literal behaviour; measurement / tests).  Default 1.  Process-wide. */
int sxmc_set_deferred_eval(int enable);
/* LAZY EvalFinished (default 1; SXMC_LAZY_FINISH=0 in the environment changes the default).  A batch of two or more
 * deferred evaluations is launched on the legacy default stream -- where the reference's caller launches its NLL
 * kernels (mcmc.cpp:314-348) and with which every blocking stream orders.  What the caller does next through this ABI
 * on that stream or on a blocking stream (its kernels, blocking copies to the host, the next evaluation) is therefore
 * ordered after the batch ON THE DEVICE, and sxmc_hist_eval_finished of such a batch does not stop the host: the wait
 * is carried out by the first call that could tell the difference -- one that names a stream created non-blocking,
 * or that synchronises or queries a stream or the device.  The host then runs ahead of the device as a caller of the
 * group API does, instead of idling the device once per MCMC step.  NOT covered: device work the caller issues
 * outside this ABI, on a non-blocking stream of its own, straight after EvalFinished -- such a caller sets 0, and
 * EvalFinished blocks until the evaluation has finished, as in the reference. */
int sxmc_set_lazy_finish(int enable);
/* Process-wide counters of the batching above: group launches made for deferred evaluations, and the evaluations
 * (evaluator x EvalAsync) they carried -- 1 and S per MCMC step of an unchanged mcmc.cpp.  For tests and logs. */
int sxmc_deferred_eval_stats(unsigned long long* launches, unsigned long long* evaluations);

/* Introspection used by CreateHistogram / GetSamples / tests (pdfz.cpp:498-594, pdfz.h:542-556). */
int sxmc_hist_total_nbins(sxmc_hist_t h, int* total_nbins);
int sxmc_hist_bin_volume(sxmc_hist_t h, double* bin_volume);
int sxmc_hist_nsamples(sxmc_hist_t h, size_t* nsamples);
int sxmc_hist_npoints(sxmc_hist_t h, size_t* npoints);
int sxmc_hist_get_bins(sxmc_hist_t h, unsigned* h_bins, size_t n);       /* after eval_finished */
int sxmc_hist_get_read_bins(sxmc_hist_t h, int* h_read_bins, size_t n);
/* The histogram of the evaluator's LAST evaluation projected onto observable `obs` (TH2D::ProjectionX and its kin, as
 * plot_fit uses them, plots.cpp:226-241; CreateHistogramProjection, pdfz.h:505-518): h_counts[j] = the sum of the bins
 * whose index along `obs` is j, exact integers in 64 bits; n must be that observable's bin count.  The bins are summed
 * where they are -- one pass over the histogram with integer atomics, partial marginals in LDS up to 2048 bins of the
 * asked observable, one HBM atomic per non-empty bin beyond -- and only the n totals come back (sxmc_hist_get_bins
 * copies the whole histogram: 512 MB at BASELINE config 5).  The histogram is left untouched.  Runs on the evaluator's
 * stream after whatever is queued there; returns when h_counts is filled.  SXMC_ERR_INVALID (before the device is
 * touched): a null argument, obs outside [0, nobservables), a wrong n.  SXMC_ERR_STATE, with sxmc_hist_get_bins'
 * message: the histogram is not filled (a sparse look-up, a consuming step). */
int sxmc_hist_project(sxmc_hist_t h, int obs, unsigned long long* h_counts, size_t n);
/* GetSamples: rows of nobservables+1 floats (observables, dataset id); n = nsamples*(nobs+1). */
int sxmc_hist_get_samples(sxmc_hist_t h, float* h_out, size_t n);
/* EvalHist::RandomSample's sampling step (pdfz.cpp:817-922; 1-3 observables, as there) on the device: nobserved
 * events drawn from the histogram of the evaluator's LAST evaluation (evaluate with do_eval_pdf = 0 first, what
 * CreateHistogram does) -- a bin with probability proportional to its content, a point uniform inside it (TH1::
 * GetRandom's rule) -- redrawn while outside [lowers, uppers] when those are given (pdfz.cpp:853-857).  The
 * histogram stays in HBM (the reference, and round 1 of this library, copied every signal's histogram to the
 * host per fake experiment); only the events come back: h_events receives nobserved rows of nobservables + 1
 * floats (last = the evaluator's dataset id), the layout sxmc_hist_set_eval_points takes.  The Poisson fluctuation
 * of the event count (pdfz.cpp:836-841) is the caller's, on the host: it decides array sizes.  The contract, which
 * tests/hist_sample_reference.py restates and the device output equals bit for bit:
 *   words    event e, attempt t (from 0): Philox4x32-10 with counter words (e low, e high, t, 0) and key
 *            (seed low, seed high) gives x, y, z, w -- the same seed and histogram give the same bits, on a shared
 *            evaluator too
 *   bin      cdf = the inclusive uint32 prefix sum of the flat row-major histogram, total = its last entry (0:
 *            SXMC_ERR_INVALID); target = (x * total) >> 32; the bin is the first with cdf > target, so an empty bin
 *            is never drawn; it is unravelled with the last observable fastest
 *   point    observable k of index idx takes the next word of y, z, w:
 *            xd = lower + (idx + (word + 0.5) * 2^-32) * ((upper - lower) / nbins), every operation rounded in f64
 *   float    xf = (float)xd.  Rounding can carry xf out of the bin or of the domain, so xf is then moved one float at
 *            a time, at most 4, towards the bin until the evaluator's own look-up of it -- lower <= xf < upper and
 *            (int)((xf - lower) * (nbins / (upper - lower))), in f64 on the float, with the evaluator's lower, upper
 *            and quotient -- gives idx.  Every event therefore looks up into the bin it was drawn from.  Only a bin that
 *            holds no float at all (it is narrower than the float spacing at its position) cannot be met: the event is
 *            then the in-domain float nearest to xd
 *   cuts     lowers / uppers (host float arrays, both or neither), inclusive, tested on xf: while xf > upper cut or
 *            xf < lower cut in any observable the event is redrawn with the next attempt, bin and point; after 1024
 *            attempts SXMC_ERR_STATE with the count of such events -- none is handed out
 * nobserved == 0 does nothing; more than 3 observables: SXMC_ERR_INVALID with the reference's message; after an
 * evaluation that left the histogram unfilled (sparse look-up, a consuming step): SXMC_ERR_STATE. */
int sxmc_hist_random_sample(sxmc_hist_t h, size_t nobserved, unsigned long long seed, const float* lowers,
                            const float* uppers, float* h_events);
int sxmc_hist_get_stream(sxmc_hist_t h, sxmc_stream_t* s);

/* EvalHist's `optimize` constructor argument (pdfz.cpp:188; default 1).  The reference's evaluator runs its launch-shape
 * trials (Optimize, pdfz.cpp:622-814) inside its first EvalAsync once it has evaluation points (:441-448), never while
 * CreateHistogram evaluates (:503-504).  Here the trials are those of the BATCH the library forms behind the
 * per-evaluator calls (sxmc_group_optimize: a few timed fills pick lanes per CU, teams and codes on the box it runs on),
 * at the batch's first lookup evaluation, when EVERY member has optimize on; 0 pins the analytic launch shape. */
int sxmc_hist_set_optimize(sxmc_hist_t h, int enable);
/* EvalHist::Optimize (pdfz.cpp:622-628) called by hand: the trials run (again) at the next lookup evaluation of every
 * batch `h` is part of.  Nothing without evaluation points, as in the reference. */
int sxmc_hist_optimize(sxmc_hist_t h);
/* The launch plan of the batch the evaluator's evaluations go into (one line per fill launch, as
 * sxmc_group_launch_info) and a last line "tuned=<0|1> trial_launches=<n>".  Empty before the first evaluation. */
int sxmc_hist_launch_info(sxmc_hist_t h, char* out, size_t n);
/* Replaces EvalHist::Optimize/OptimizeBin/OptimizeEval (pdfz.cpp:622-814): the launch shape
 * is sized analytically from the device; 0 keeps the default.  threads: a multiple of 64 up to 1024. */
int sxmc_hist_set_launch_config(sxmc_hist_t h, int bin_threads, int bin_blocks_per_cu);

/* ---------------------------------------------------------------- pdfz::EvalKernel ---------- */
/* The kernel-density PDF (pdfz.h:578-625; the reference declares it and leaves it unimplemented): a Gaussian kernel
 * on every Monte Carlo sample, after the systematics have moved it, truncated to the domain and renormalised there.
 * Contract (sxmc_amd/include/sxmc/pdfz.h, class EvalKernel, says it in full):
 *   h_d = bandwidth_scale_d * sigma_d * n^(-1/(D+4)) (Scott's rule), fixed at creation, sigma_d the sample standard
 *   deviation (n - 1) of observable d over the n untransformed samples inside the domain;
 *   norm = the in-domain count after the systematics (equal to EvalHist's on the same inputs);
 *   pdf(x) = 1/norm sum_i w_i prod_d phi((x_d - s_id)/h_d)/h_d, w_i = 1 / prod_d [Phi((upper_d - s_id)/h_d) -
 *   Phi((lower_d - s_id)/h_d)] for in-domain samples, 0 otherwise; points outside the domain NaN, points of another
 *   data set 0, norm 0 NaN.  At most 4 observables.  Cost: O(points x samples) per evaluation.
 * Validation as sxmc_hist_create (pdfz.cpp:64-82, MAX_NFIELDS), then the bandwidth scales (count, positive and
 * finite), at most 4 observables, upper > lower, at least 2 in-domain samples and no zero spread. */
typedef struct sxmc_kde* sxmc_kde_t;     /* one pdfz::EvalKernel */
int sxmc_kde_create(const float* samples, size_t nsamples_floats, int samples_on_device,
                    int nfields, int nobservables,
                    const double* lower, size_t n_lower,
                    const double* upper, size_t n_upper,
                    const double* bandwidth_scale, size_t n_bandwidth_scale,
                    unsigned dataset, sxmc_kde_t* out);
/* Adaptive (sample-point) bandwidths, Abramson's estimator (Silverman 5.3): sxmc_kde_create with one more number, the
 * bandwidth sensitivity alpha in [0, 1] (SXMC_ERR_INVALID otherwise, or when not finite).  alpha == 0 IS
 * sxmc_kde_create: the same kernels, the same row layout, the same bits.  For alpha > 0 every table row i gets a
 * factor lambda_i on all its bandwidths, fixed at creation on the UNTRANSFORMED table, after the Scott bandwidths h_d:
 *   pilot   S0 = the n untransformed samples inside the domain.  For every table row i (inside the domain or not), in
 *           f64 on the device:  f_i = (1/n) sum_{j in S0} w_j prod_d phi((x_id - x_jd)/h_d)/h_d,
 *           w_j = 1 / prod_d [Phi((upper_d - x_jd)/h_d) - Phi((lower_d - x_jd)/h_d)] -- the evaluator's own
 *           fixed-bandwidth PDF at zero systematics, continued by the same formula outside the domain.  The difference
 *           x_id - x_jd is taken first, on the f64 values of the floats, then divided by h_d; Phi through erfc.
 *   scale   g = exp((1/n) sum_{i in S0} ln f_i), on the host in f64, in table order (f_i > 0 on S0: a row's own term).
 *   factors lambda_i = min(10, max(0.1, (f_i / g)^(-alpha))); a row whose f_i is not finite and positive takes 10.  The
 *           clips bound how far the f32 coordinates of the pair sum are stretched.
 * The factors belong to table rows: a sample keeps its lambda_i wherever the systematics move it, rows that start
 * outside the domain and move in included.  Per evaluation, with s_i the moved samples and norm the in-domain count
 * (unchanged: EvalHist's, bit for bit):
 *   pdf(x) = (1/norm) sum_{i in domain} w_i prod_d phi((x_d - s_id)/(h_d lambda_i))/(h_d lambda_i),
 *   w_i the truncation weight at bandwidth h_d lambda_i, so the integral over the domain is still exactly 1; point
 *   codes, the NaN / 0 rules and norm == 0 as for sxmc_kde_create.
 * sxmc_kde_random_sample draws coordinate d of an event that picked row i from N(s_id, (h_d lambda_i)^2) truncated to
 * the domain (the same Philox words, counters, rounding and clamps); sxmc_kde_project uses, per sample and bin,
 *   [Phi((t_j+1 - u_i)/lambda_i) - Phi((t_j - u_i)/lambda_i)] / [Phi((T - u_i)/lambda_i) - Phi(-u_i/lambda_i)].
 * Deterministic: no floating-point atomics; the pilot's split over workgroups depends on n alone and the splits are
 * added in order, so two creations, on any device, give the same lambda bits.
 * Accuracy of a value: the bound of tests/kde_adaptive_reference.py; relative to the fixed-bandwidth bound the
 * coordinate term grows by at most the largest 1/lambda_i^2 in reach of the point (<= 100 by the clips).
 * Cost: one more multiply per pair than the fixed-bandwidth sum, rows of nobservables + 2 floats; the pilot is
 * O(samples^2) in f64, once per creation. */
int sxmc_kde_create_adaptive(const float* samples, size_t nsamples_floats, int samples_on_device,
                             int nfields, int nobservables,
                             const double* lower, size_t n_lower,
                             const double* upper, size_t n_upper,
                             const double* bandwidth_scale, size_t n_bandwidth_scale,
                             unsigned dataset, double sensitivity, sxmc_kde_t* out);
/* The sensitivity the evaluator was created with (0 for sxmc_kde_create). */
int sxmc_kde_sensitivity(sxmc_kde_t k, double* sensitivity);
/* lambda[0 .. nsamples): the factors fixed at creation, in table order; all 1.0 for a fixed-bandwidth evaluator.
 * n must be nsamples. */
int sxmc_kde_local_factors(sxmc_kde_t k, double* lambda, size_t n);
/* WEIGHTED MONTE CARLO SAMPLES in the kernel-density evaluator: sxmc_kde_create_adaptive with one integer MULTIPLICITY
 * m_i per table row (host memory), the fixed-point weights sxmc_sample_multiplicities makes -- as for
 * sxmc_hist_set_sample_multiplicities, the norm stays an `unsigned` (equal to a weighted histogram evaluator's, bit for
 * bit) and the scale 2^k cancels wherever norm and n_mc meet.  multiplicities == NULL IS sxmc_kde_create_adaptive.  An
 * evaluator without multiplicities launches the kernels it launched before they existed; with them only the prepass, the
 * sampler's pick, the projection's preparation and the pilot's combine are siblings of their own, and the pair sum, the
 * cutoff's gather and culled pair sum and the combine are the same code, because the multiplicity is folded into the
 * row's weight.  THE LAWS (restated in numpy by tests/kde_weighted_reference.py):
 *   construction  multiplicities are given here and cannot be set afterwards (bandwidths, pilot and padding are fixed
 *                 here).  nmultiplicities must be the table's row count (SXMC_ERR_INVALID, by name); their total over
 *                 all rows must be <= 2^32 - 1 (SXMC_ERR_INVALID).  The library keeps its own device copy, padded with 0
 *                 to the padded row count; evaluators made by sxmc_kde_create_shared share it.
 *   bandwidths    on the host in f64 before anything is allocated on the device (sxmc_amd/csrc/kde_weights.h; also
 *                 sxmc_kde_weighted_bandwidths below), over the untransformed in-domain rows in table order, one
 *                 rounding per operation, sums sequential:
 *                   S1 = sum m_i, S2 = sum m_i^2 as exact integers (S2 in 128 bits), each converted to double once;
 *                   n_eff = S1 * (S1 / S2)  (Kish);  mu_d = (sum (double)m_i * x_id) / S1;
 *                   V_d = sum (double)m_i * (dx * dx), dx = x_id - mu_d;  sigma_d = sqrt(V_d / (S1 - S2 / S1));
 *                   h_d = scale_d * sigma_d * pow(n_eff, -1/(D+4)).
 *                 Refused by name (SXMC_ERR_INVALID): fewer than 2 in-domain rows with m > 0, S1 - S2 / S1 not positive,
 *                 sigma_d == 0.  A power-of-two rescaling of every m gives the same bytes (all m == 8: the unweighted
 *                 evaluator's); a bandwidth does not depend on the quantiser's k.
 *   evaluation    norm = sum of m_i over the rows that pass the domain test after the systematics (integer atomics).
 *                 The prepass stores the row's weight as (float)((double)m_i / mass_i), adaptive evaluators
 *                 (float)((double)m_i / (mass_i * lambda_i^D)); 0 outside the domain or when m_i == 0 -- such a row then
 *                 drops out of the cutoff's tile boxes and of the sampler's pool by the tests those make on the weight.
 *                 pdf(x) = prefactor / norm * sum_i m_i w_i prod_d phi(...).  Point codes, NaN rules, do_eval_pdf = 0
 *                 unchanged.  The four multiplicities of a lane's rows are one 16-byte load.
 *   sampling      T = norm.  C_j: the inclusive prefix sums of the multiplicities of the in-domain rows with m > 0, in
 *                 table order.  An attempt's first Philox word picks target = (word * T) >> 32 in 64 bits and the row
 *                 picked is the first whose C_j exceeds target; everything after the pick is sxmc_kde_random_sample's.
 *                 sxmc_kde_sample_pool answers the number of in-domain rows with m > 0.
 *   projection    a row's reciprocal mass is multiplied by (double)m_i and m_i is counted:
 *                 h_prob[j] = (1/norm) sum_i m_i [...]; the lane-per-bin kernel and the combine are unchanged.
 *   pilot         f_i = prefactor / S1 * sum_j m_j w_j prod phi(...) over the in-domain rows in table order (the host
 *                 hands m_j / mass_j as the row's weight and S1 in place of n); g = exp((sum (double)m_i * ln f_i) / S1)
 *                 over the in-domain rows (a row with m_i == 0 adds nothing and its f_i is not read); lambda_i as for
 *                 sxmc_kde_create_adaptive, for every row.
 * Not built, refused by name: cross-validation of such an evaluator (sxmc_kde_cv_scores, sxmc_kde_cv_select:
 * SXMC_ERR_STATE). */
int sxmc_kde_create_weighted(const float* samples, size_t nsamples_floats, int samples_on_device,
                             int nfields, int nobservables,
                             const double* lower, size_t n_lower,
                             const double* upper, size_t n_upper,
                             const double* bandwidth_scale, size_t n_bandwidth_scale,
                             unsigned dataset, double sensitivity,
                             const unsigned* multiplicities, size_t nmultiplicities, sxmc_kde_t* out);
/* sum m_i over all rows, or the row count when no multiplicities are set: what n_mc is for either kind. */
int sxmc_kde_sample_total(sxmc_kde_t k, unsigned long long* total);
/* The multiplicities back on the host, n = the row count; all 1 when none are set (*is_set, optional, says which;
 * h_m NULL with n 0 asks that question alone). */
int sxmc_kde_get_sample_multiplicities(sxmc_kde_t k, unsigned* h_m, size_t n, int* is_set);
/* n_eff of the bandwidths, or the in-domain row count n when no multiplicities are set. */
int sxmc_kde_effective_samples(sxmc_kde_t k, double* n_eff);
/* The bandwidth law above on the host alone: no device call, usable without a GPU.  samples: the row-major table on the
 * host; multiplicities NULL: every row counts once (the unweighted rule's bytes).  Outputs, each optional: h, sigma, mean
 * [nobservables]; n_eff, s1, s2 (the two sums as doubles; written even when the table is then refused).  Validation and
 * refusals as at creation. */
int sxmc_kde_weighted_bandwidths(const float* samples, size_t nsamples_floats, int nfields, int nobservables,
                                 const double* lower, size_t n_lower, const double* upper, size_t n_upper,
                                 const double* bandwidth_scale, size_t n_bandwidth_scale,
                                 const unsigned* multiplicities, size_t nmultiplicities,
                                 double* h, double* sigma, double* mean, double* n_eff, double* s1, double* s2);
/* A second evaluator over the SAME sample table as `base` (as sxmc_hist_create_shared: the table is shared and reference
 * counted, nothing is copied): systematics, bandwidths, prefactor and (adaptive) the sensitivity and the factors copied
 * from `base`, never recomputed; own rows, evaluation points, bindings, partial sums and stream.  For concurrent
 * experiments on one GPU.  May outlive `base`. */
int sxmc_kde_create_shared(sxmc_kde_t base, sxmc_kde_t* out);
int sxmc_kde_destroy(sxmc_kde_t k);
/* As sxmc_hist_add_systematic.  SXMC_ERR_INVALID beyond 7 columns (observables + fields systematics read) or 64
 * polynomial coefficients in all. */
int sxmc_kde_add_systematic(sxmc_kde_t k, int type, int obs, int extra_field, int npars, const short* pars);
/* As sxmc_hist_set_eval_points: rows of nobservables + 1 floats (last = dataset id), host memory. */
int sxmc_kde_set_eval_points(sxmc_kde_t k, const float* points, size_t npoints_floats);
int sxmc_kde_set_pdf_value_buffer(sxmc_kde_t k, float* d_output, int offset, int stride);
int sxmc_kde_set_normalization_buffer(sxmc_kde_t k, unsigned* d_norm, int offset);
int sxmc_kde_set_parameter_buffer(sxmc_kde_t k, const double* d_params, int offset, int stride);
/* Launches on the evaluator's own stream and returns before completion; do_eval_pdf = 0 computes the norm only.
 * eval_finished waits for the evaluator's stream. */
int sxmc_kde_eval_async(sxmc_kde_t k, int do_eval_pdf);
int sxmc_kde_eval_finished(sxmc_kde_t k);
int sxmc_kde_get_stream(sxmc_kde_t k, sxmc_stream_t* s);
/* What sxmc_kde_eval_async launches -- norm clear, prepass, pair sum, combine: the same kernels, the same split over
 * workgroups, the same bits -- on the CALLER's stream `s`, for a walk that keeps its whole step on one stream (a mixed
 * fit: sxmc_group_eval_columns_nll_async).  Capture-safe: no allocation, no blocking copy, no wait, so it may be recorded
 * into a graph (sxmc_graph_begin_capture on `s`).  The evaluator remembers `s`: set_eval_points, random_sample,
 * sample_pool, project, eval_async, eval_finished and destroy wait for the last work given to it before they touch the
 * evaluator's own stream (a host wait, once; SXMC_ERR_STATE while a graph is being recorded), and this entry waits for
 * work on the evaluator's own stream that no eval_finished has waited for (outside a recording; inside one that is
 * SXMC_ERR_STATE: call eval_finished first). */
int sxmc_kde_eval_on_stream_async(sxmc_kde_t k, int do_eval_pdf, sxmc_stream_t s);
/* The parameter indices the attached systematics read, in the order attached: the `pars` of add_systematic, before the
 * parameter buffer's offset and stride.  *n: how many there are; pars[0 .. min(cap, *n)) is written.  A walk re-evaluates
 * a kernel-density signal only when one of them floats. */
int sxmc_kde_parameters_read(sxmc_kde_t k, short* pars, size_t cap, size_t* n);
/* Evaluations launched so far, by eval_async or eval_on_stream_async (launches recorded into a graph count when they are
 * recorded, not when the graph is replayed).  For tests and reports, like sxmc_deferred_eval_stats. */
int sxmc_kde_evaluation_count(sxmc_kde_t k, unsigned long long* n);
/* h[0 .. nobservables): the bandwidths fixed at creation. */
int sxmc_kde_bandwidths(sxmc_kde_t k, double* h, size_t n);
int sxmc_kde_nsamples(sxmc_kde_t k, size_t* nsamples);
int sxmc_kde_npoints(sxmc_kde_t k, size_t* npoints);
/* The counterpart of sxmc_hist_random_sample: nobserved events drawn from the PDF of the evaluator's LAST evaluation
 * (eval_async with do_eval_pdf 0 or 1; before any: SXMC_ERR_STATE).  Let S be that evaluation's in-domain moved samples
 * (n = |S| = its norm; n == 0: SXMC_ERR_STATE).  An event picks s_i from S uniformly (the mixture weight 1/n; w_i only
 * renormalises the truncated kernel), then each x_d from N(s_id, h_d^2) truncated to [lower_d, upper_d), by the inverse
 * CDF in f64; a value that rounds to upper_d as a float becomes the float below it, so every event passes the
 * evaluator's domain test lower <= x < upper.  Outside [lowers, uppers] (inclusive, host float arrays, both or
 * neither) the event is redrawn, a new sample and new coordinates, up to 1024 attempts; then SXMC_ERR_STATE with the
 * count.  h_events: nobserved rows of nobservables + 1 floats (last = dataset id).  Counter-based: Philox4x32-10 keyed
 * by `seed`, counters (event, 2 attempt) and (event, 2 attempt + 1) -- the same seed and parameters give the same
 * bits, on a shared evaluator too.  nobserved == 0 does nothing.  1 to 4 observables.  Which word does what, as
 * tests/kde_sample_reference.py restates it and the device output equals, bit for bit wherever the last bits of the
 * device's erfc and erfcinv cannot decide a rounding:
 *   words    event e, attempt t (from 0): block A = Philox4x32-10 with counter words (e low, e high, 2t, 0), block B
 *            with (e low, e high, 2t + 1, 0), both with key (seed low, seed high), each giving x, y, z, w
 *   row      the in-domain rows of the last evaluation are listed in table order (n of them); A.x picks place
 *            (A.x * n) >> 32 of that list
 *   point    observables 0..3 take the words A.y, A.z, A.w, B.x in this order.  With c the float the evaluation left
 *            for the row and observable, (float)((x - lower) * (0.84932180028801907 / h)), every operation rounded
 *            in f64: s = lower + (double)c * (h / 0.84932180028801907) and hw = h * lambda[table row] (lambda = 1 on a
 *            fixed-bandwidth evaluator: the factor belongs to the table row, not to the place in the list);
 *            pa = Phi((lower - s) / hw), qb = Phi((s - upper) / hw), Phi(z) = 0.5 * erfc(-z * 0.70710678118654752),
 *            m = (0.5 - pa) + (0.5 - qb), p = pa + (word + 0.5) * 2^-32 * m
 *   branch   p <= 0.5: z = -1.4142135623730950 * erfcinv(2 p); otherwise the complement is formed without
 *            cancellation, q = qb + ((2^32 - 1 - word) + 0.5) * 2^-32 * m, and z = +1.4142135623730950 * erfcinv(2 q);
 *            xd = s + hw * z
 *   float    xf = (float)xd; then xf = bottom, the smallest float >= lower, if not (xf >= lower), then xf = top, the
 *            largest float < upper, if not (xf < upper): both tests in f64 on the float, after the rounding
 *   cuts     on the floats: while xf > upper cut or xf < lower cut in any observable (all are drawn first) the event
 *            takes attempt t + 1, a new row and new words */
int sxmc_kde_random_sample(sxmc_kde_t k, size_t nobserved, unsigned long long seed, const float* lowers,
                           const float* uppers, float* h_events);
/* n: how many samples the last evaluation left inside the domain, counted by the sampler's own compaction (its norm;
 * for tests).  SXMC_ERR_STATE before an evaluation. */
int sxmc_kde_sample_pool(sxmc_kde_t k, size_t* n);
/* The PDF of the evaluator's LAST evaluation projected onto observable `obs`: h_prob[j] = its share in bin j of nbins
 * equal bins of [lower, upper).  The kernel of a sample is a product over the observables, the others integrate to
 * their own truncation mass and cancel, so with (c_i, w_i) the rows the evaluation left (c the sample's scaled
 * coordinate along `obs`, a float: (s - lower) sqrt(log2(e) / 2) / h), n the rows with w_i > 0 (the norm),
 * u_i = c_i / sqrt(log2(e) / 2) in f64 (so u = (s - lower) / h), T = (upper - lower) / h, edges e_j = lower + j ((upper - lower) / nbins) (e_0 = lower
 * and e_nbins = upper themselves) and t_j = (e_j - lower) / h:
 *   h_prob[j] = (1/n) sum_i [Phi(t_j+1 - u_i) - Phi(t_j - u_i)] / [Phi(T - u_i) - Phi(-u_i)]
 * over those rows; the shares sum to 1; all 0 when n = 0.  f64 throughout, Phi(z) = erfc(-z / sqrt 2) / 2; the samples
 * are split across workgroups in a way that depends on their number alone and the splits are added in order, without
 * floating-point atomics: two calls give the same bits.  Cost O(samples x nbins).  Runs on the evaluator's stream;
 * returns when h_prob is filled; the rows are left untouched.  SXMC_ERR_INVALID: a null argument, obs outside
 * [0, nobservables), nbins < 1.  SXMC_ERR_STATE before any evaluation. */
int sxmc_kde_project(sxmc_kde_t k, int obs, int nbins, double* h_prob);
/* A cutoff radius R on the pair sum, in units of each sample's own bandwidth (h_d, or h_d lambda_i when adaptive):
 * opt-in, and an approximation whose error is the bound stated here.  R = 0, the default, is everything above: the same
 * kernels, the same row layout, the same bits.  Accepted: 0, or 1 <= R <= +infinity; anything else, NaN included, is
 * SXMC_ERR_INVALID (checked first, without a device).
 *   qcut   = R^2 log2(e) / 2, as an f32 rounded up.
 *   q'     of a pair = g_i sum_d (c_pd - c_id)^2 exactly as the pair kernels compute it in f32 (the square of the first
 *            difference, a fused multiply-add per further observable, then times g_i; g_i = 1 for fixed bandwidths).
 *   A pair is dropped only if the kernel's own f32 q' for it would have been >= qcut; pairs below qcut are always
 *   summed.  A value therefore lies between the full sum and the sum over the pairs with q' < qcut (before the common
 *   rounding bound of tests/kde_cutoff_reference.py); each dropped term is at most W_i 2^-qcut.  So the PDF no longer
 *   integrates to exactly 1: it falls short by at most the dropped mass, at most 2^-qcut (2 pi)^(-D/2) / prod h times
 *   the mean weight per point.  From qcut > 149 (R >= 15) every dropped exp2 is exactly 0 in f32 and the values are
 *   those of R = +infinity bit for bit.  R = +infinity drops nothing but sums in the sorted order below.
 * Pairs are dropped a 256-sample tile at a time against a wave of 64 points at a time:
 *   order    when a cutoff is first set the host orders the table rows by their UNTRANSFORMED coordinates clamped to the
 *            domain: a plain sort for one observable, else the Morton order of a fixed grid of 2^(32 / D) cells per
 *            observable over [lower, upper); stable, ties by table index.  Built once per table and kept on the device;
 *            evaluators made by sxmc_kde_create_shared use it and copy R from their base.
 *   gather   per evaluation, after the unchanged prepass (which keeps writing its rows in table order; random_sample,
 *            sample_pool and project keep reading them and return the bytes of the same evaluator at R = 0), one more
 *            launch copies the rows into that order and writes each tile's box: min and max of c_d over its rows with
 *            weight > 0, and their smallest g when adaptive.  The boxes are of the MOVED samples of this evaluation, so
 *            the culling is exact under any systematic; the order only keeps tiles compact.  A tile without such a row
 *            has an empty box and is never visited.
 *   points   set_eval_points sorts the live points (code 0) by the same key, the others last, and keeps the
 *            permutation for the combine, which still writes pdf_out[offset + stride * i] for the caller's i; one box per
 *            wave of 64 sorted points, over live points only; a wave without live points visits nothing.
 *   visit    per wave and tile gap_d = max(0, tile_lo_d - wave_hi_d, wave_lo_d - tile_hi_d) and q_lb from the gaps by
 *            the pair's own operation sequence, times the tile's smallest g.  Rounding is monotone, so every pair of that
 *            wave and tile has q' >= q_lb: no margin.  A tile is visited iff q_lb < qcut
 *            (sxmc_amd/csrc/kde_cutoff.h, cutoff_visit: one function for the device and for a host replay).
 *   sums     f32 within a visited tile, f64 across the visited tiles in tile order, the sample split over workgroups
 *            and the combine in split order as without a cutoff; the split itself is the plain one's with the tiles of
 *            a workgroup doubled up to 16 while four workgroups remain to every resident one (kde_cutoff.h,
 *            cutoff_split), so that a wave's tile tests and its count are paid once per 16 tiles.
 * What does not change: the norm, the point codes, the NaN and 0 rules, norm == 0; bandwidths, local factors,
 * cross-validation and the pilot.  What does: a point's value depends on which other points share its wave (the decision
 * is per wave), always inside the envelope above.  Two evaluations, a shared evaluator and any device still give the
 * same bits: no floating-point atomics, and the tiles a wave visits depend on the data alone.
 * sxmc_kde_set_cutoff: the evaluator must be idle (it waits for its streams); SXMC_ERR_STATE while a graph is being
 * recorded.  Plans the points again if they are already set.  Every buffer an evaluation needs is allocated here or in
 * set_eval_points, so sxmc_kde_eval_on_stream_async stays capture-safe.
 * sxmc_kde_cutoff_stats: of the LAST evaluation, the tiles its waves visited (each wave and sample split adds its own with
 * one integer atomic, into one of 64 counters that are added on the host) and tiles_possible = live point-waves x tiles; both 0 when that evaluation had no cutoff or no
 * lookup.  Waits for the evaluator.
 * sxmc_kde_cutoff_boxes (for tests: a host replay of the visit test): the tile boxes the last evaluation wrote,
 * [tiles][9] floats lo[4], hi[4], smallest g, and the wave boxes of the point plan, [pitch / 64][8] floats lo[4], hi[4],
 * pitch the points rounded up to 256.  SXMC_ERR_STATE without a cutoff or points.
 * sxmc_kde_pair_split (for tests: which regime of the pair sum a shape reaches on this device): the split of the
 * current point plan, with or without a cutoff -- the pair sum's next launch has nsplit workgroups to every 256 points,
 * each over tiles_per_split tiles of 256 sample rows (the last split: what is left of them).  It depends on the points,
 * the table, the device's compute units and whether a cutoff is set.  Reads the plan only: no launch, no wait.
 * SXMC_ERR_STATE without points. */
int sxmc_kde_set_cutoff(sxmc_kde_t k, double R);
int sxmc_kde_cutoff(sxmc_kde_t k, double* R);
int sxmc_kde_cutoff_stats(sxmc_kde_t k, unsigned long long* tiles_visited, unsigned long long* tiles_possible);
int sxmc_kde_cutoff_boxes(sxmc_kde_t k, float* tile_boxes, size_t ntile_floats, float* wave_boxes, size_t nwave_floats);
int sxmc_kde_pair_split(sxmc_kde_t k, int* nsplit, unsigned* tiles_per_split);
/* scale[0 .. nobservables): the bandwidth scales the evaluator was created with (a shared evaluator: its base's). */
int sxmc_kde_bandwidth_scale(sxmc_kde_t k, double* scale, size_t n);
/* Bandwidths by leave-one-out likelihood cross-validation (Silverman 3.4.4): the bandwidths that maximise the
 * log-likelihood of the sample under its own estimate with each row left out of its own sum.  Contract, all in f64 on
 * the f64 values of the float table at zero systematics:
 *   rows     the n untransformed rows inside the domain, in table order; with max_rows > 0 and n > max_rows every
 *            ceil(n / max_rows)-th of them from the first (max_rows == 0: all).  m of them are scored; m < 2 is
 *            SXMC_ERR_INVALID.
 *   score    for a candidate bandwidth vector h, [L_d, U_d) the domain, Phi through erfc as the prepass and the pilot
 *            write it:
 *              M_jd(h)  = Phi((U_d - x_jd)/h_d) - Phi((L_d - x_jd)/h_d)
 *              f_-i(h)  = 1/(m-1) sum_{j != i} prod_d phi((x_id - x_jd)/h_d) / (h_d M_jd(h))
 *              score(h) = (1/m) sum_i ln f_-i(h)
 *            The pair j == i is left out of the sum, never subtracted afterwards (for an isolated row subtraction would
 *            cancel what the score is about); rows with equal coordinates are different rows.  A row with f_-i = 0
 *            (no neighbour within exp's range) contributes -inf: the candidate scores -inf and is never chosen.
 *   device   one lane per scored row, the m sample rows wave-uniform; per pair the D squared differences e_d once, per
 *            candidate q = sum_d e_d / (2 h_d^2) with the reciprocal taken once per scan, one exp and one multiply-add
 *            by the weight 1 / prod_d (h_d M_jd) into the candidate's own accumulator: K <= 32 candidates share the
 *            loads and the differences of one pass over the m^2 pairs.
 *   order    no floating-point atomics.  The sample rows are cut over workgroups by a rule that reads m and K alone
 *            (sxmc_amd/csrc/kde_cv.h, cv_split, beside the pilot's), the partial sums are added in split order, then
 *            the logarithm is taken; the m logarithms of a candidate are added on the host in table order.  Two calls
 *            give the same score bits, on any device, and so does a shared evaluator.
 *   subsets  the candidates of a search are scaled to the rows scored: h_cd = s_c sigma_d m^(-1/(D+4)), sigma_d the
 *            evaluator's own standard deviation over all n in-domain rows.  n^(-1/(D+4)) is the exponent Scott's rule
 *            and the AMISE optimum share, so a multiplier found on m rows carries over to n.
 *   grid     multipliers s_k = lo (hi/lo)^(k/(steps-1)), k = 0 .. steps - 1 (taken through log2 / exp2, so that powers of two are
 *            met exactly); 1 <= steps <= 32, 0 < lo <= hi, both finite.  The default lo = 1/8, hi = 4, steps = 21 has
 *            ratio 2^(1/4) and 1 on the grid.
 *   choice   the largest finite score; a tie goes to the multiplier with the smaller |ln s|, then to the smaller s; no
 *            finite score at all is SXMC_ERR_INVALID with a message.
 *   search   (a) one scan of a common multiplier on all observables; (b) with per_observable one round of coordinate
 *            scans in observable order over the same grid, the other observables held at the values chosen so far.
 *            The value held is on the grid, so the chosen score never decreases from one scan to the next.
 * Cross-validation chooses the GLOBAL scales, the Scott stage: an adaptive evaluator created with the chosen scales
 * runs its pilot and takes its factors lambda_i at the chosen bandwidths, as if the scales had been typed in.  The
 * evaluator these are called on keeps its own bandwidths, fixed at creation, and neither call touches its rows or
 * its last evaluation.  Accuracy of a score: the bound of tests/kde_cv_reference.py.  Cost O(m^2 K) per scan.
 *
 * sxmc_kde_cv_scores: the primitive, no search.  bandwidths[c * nobservables + d]: ncandidates (1 .. 32) absolute
 * candidate vectors, positive and finite; scores[c] their scores; *rows_used (may be null) = m.
 * sxmc_kde_cv_select: the search on the evaluator's table.  scale_out[0 .. nobservables): the chosen multipliers of
 * Scott's rule, a bandwidth_scale for sxmc_kde_create.  The report, every pointer of which may be null: *score the
 * score of the choice; *score_at_one the common scan's score at s = 1 (NaN when 1 is not on the grid);
 * at_edge[d] = 1 when the choice of observable d sits on the first or last grid value (widen the grid); *rows_used = m;
 * *nscans = 1 or 1 + nobservables; scan_grid and scan_scores [nscans][steps] every scan's multipliers and scores, the
 * common scan first; scan_chosen[nscans] the index each scan chose.
 * Argument validation (null arguments, the candidate count and values, the grid, m < 2) needs no GPU. */
int sxmc_kde_cv_scores(sxmc_kde_t k, const double* bandwidths, int ncandidates, size_t max_rows, double* scores,
                       size_t* rows_used);
int sxmc_kde_cv_select(sxmc_kde_t k, double lo, double hi, int steps, int per_observable, size_t max_rows,
                       double* scale_out, size_t n_scale, double* score, double* score_at_one, int* at_edge,
                       size_t* rows_used, int* nscans, double* scan_grid, double* scan_scores, int* scan_chosen);

/* ---------------------------------------------------------------- evaluator group ----------- */
/* The "EvalAsync on all signals, then EvalFinished on all" of mcmc.cpp:264-271 and
 * bench_sxmc.cpp:193-200 as ONE batched launch sequence (zero, fill, evaluate) over all
 * members.  Members are borrowed; their bindings are re-read whenever they change. */
int sxmc_group_create(const sxmc_hist_t* members, int nmembers, sxmc_group_t* out);
int sxmc_group_destroy(sxmc_group_t g);
int sxmc_group_set_launch_config(sxmc_group_t g, int bin_threads, int bin_blocks_per_cu);
/* EvalHist::Optimize / OptimizeBin (pdfz.cpp:622-727) for the batched launch: times the fill with a few
 * lane counts per CU on stream `s` and keeps the fastest (the analytic default is within a few per cent;
 * which count wins differs from one box to the next).  Only acts when every member is a pure stream and no
 * launch configuration was set by hand; results never depend on the shape.  The members' histograms and
 * normalisation slots hold counts of the trial runs afterwards (the next evaluation zeroes them as usual).
 * Where the plan streams codes (sxmc_group_set_codes left at its default) the candidates run to 1024 lanes and the
 * codes are then timed against the float columns at the parameters bound now: the float stream is taken if it wins
 * by 3 % (whether codes pay is otherwise estimated from the binning when the table is laid out).
 * *chosen_threads (optional): the lane count kept, 0 when nothing was tried. */
int sxmc_group_optimize(sxmc_group_t g, sxmc_stream_t s, int* chosen_threads);
/* How the fill kernel's work is cut over workgroups: 0 = automatic, 1 = sliced (each workgroup one
 * contiguous slice of the concatenated members), 2 = interleaved (each member's workgroups stride
 * through it chunk by chunk, like a grid-stride copy). */
int sxmc_group_set_partition(sxmc_group_t g, int mode);
/* Interleaved partition of a BUCKETED table (rows sorted by bin): a member's workgroups split into `teams` teams, each
 * over a contiguous part of the member (so a workgroup sees a fraction of the bins and flushes as few).  0 = default
 * (one team); sxmc_group_optimize tries three on the box it runs on.  Results never depend on it. */
int sxmc_group_set_partition_teams(sxmc_group_t g, int teams);
/* Sparse counting (default on): a histogram too large for LDS (more than 40 832 bins) costs one scattered
 * HBM atomic per sample plus zeroing the whole array, yet an evaluation for lookup (do_eval_pdf != 0, the
 * fused evaluations, the MCMC step) reads it only at the data events' bins.  Such evaluations count into one
 * counter per distinct event bin instead; lut, normalisations and NLL are identical.  The dense histogram
 * is then NOT filled: sxmc_hist_get_bins returns SXMC_ERR_STATE until an evaluation with do_eval_pdf = 0
 * (what CreateHistogram does, pdfz.cpp:503-506) has run. */
int sxmc_group_set_sparse(sxmc_group_t g, int enable);
/* Pre-binning (default on): an observable that no systematic writes has the same bin index at every
 * evaluation, so for launches that run a static program the evaluators build, once, a 1- or 2-byte column
 * with the partial flat index of those observables and the fill streams it instead of their float
 * columns.  Results are identical; sxmc_group_algorithmic_bytes counts the bytes actually needed. */
int sxmc_group_set_prebinning(sxmc_group_t g, int enable);
/* Bucketing (default on; takes precedence over pre-binning where it applies): the same fact taken further.
 * Where the fill runs a static program and at least one observable is written by a systematic and at least one
 * is not, the evaluator keeps, once, a second copy of its table with the samples GROUPED by their bin indices
 * in the untouched observables (stable radix sort), holding only the columns that change from evaluation to
 * evaluation (the written observables + the truth fields referenced); samples outside the domain in an
 * untouched observable can never be counted and are left out.  The fill then solves the lower-dimensional
 * problem of the written observables and reads one bin offset per 256-sample granule for the rest: BASELINE
 * config 3 streams 12 bytes per sample instead of 16 (13 with pre-binning), config 5 12 instead of 24 (14).
 * Counters are integers, so visiting the samples in another order changes no count: histograms, norms, lookup
 * tables and NLL are bit-identical (the parity tests compare on/off and against the CPU restatement).  GetSamples keeps the
 * caller's row order (it reads the original table).  Skipped for a table whose granule padding would outweigh
 * the saving (few samples, many buckets).  sxmc_group_algorithmic_bytes counts the bytes actually needed. */
int sxmc_group_set_bucketing(sxmc_group_t g, int enable);
/* Ordering (default on; needs bucketing and a histogram that fits LDS): bucketing taken to ONE observable that is
 * written -- but only by one-coefficient shift / scale / cos-theta-scale systematics (pdfz.cpp:316-325) and read
 * by nothing else.  For the evaluation's parameters each of those is a monotone map of the sample's value (IEEE
 * addition of / multiplication by a constant rounds monotonically), and so is the binning after it
 * (pdfz.cpp:388-398).  The bucketed copy keeps the rows of every bucket sorted by the raw value; a 256-sample
 * granule whose first and last sample land in the same bin (or both below / both above the domain) therefore has
 * ALL its samples there.  The fill works that out per evaluation from two floats per granule, with the per-sample
 * arithmetic, and does not read the observable's column at all; only the granules that straddle a bin edge (at
 * most nbins + 1 per bucket) take the per-sample path over the column, granules outside the domain are skipped.
 * Any NaN (sample value or coefficient) sends a granule down the per-sample path.  BASELINE config 3 streams
 * 8 bytes per sample instead of 12; a 1-D histogram with one shift (bench_sxmc pdfz) streams 12 bytes per 256
 * samples.  Histograms, norms and NLL stay bit-identical (parity tests: on/off, the CPU restatement, samples
 * placed within ulps of the bin edges).  Of several eligible observables the one with the fewest bins is taken.
 * enable = 1 (default): where it pays -- the table must have at least twice as many granules as can straddle an edge
 * (buckets x (nbins + 1)); BASELINE config 5 with its 200 bins of r and 61 granules per bucket does not qualify and
 * keeps the unordered bucketed table.  enable = 2: wherever it applies (tests).  Histograms beyond LDS capacity: the
 * sparse counting over runs and the dense evaluation have ordered forms too (run-time compiled). */
int sxmc_group_set_ordering(sxmc_group_t g, int enable);
/* Codes (default on; needs an ordered table with its histogram in LDS, 2 to 4 streamed fields and only one-coefficient
 * systematics on them).  shift / scale / cos-theta scale / resolution scale with one coefficient are affine maps of
 * the sample's fields (pdfz.cpp:316-330), so for the evaluation's parameters the bin coordinate of a written
 * observable is ONE affine function of the fields, which the reference evaluates in double, operation by operation,
 * to within a few units in the last place of it.  The ordered copy therefore keeps each streamed field a second time
 * as a 16-bit code inside a window (value = base + (code + 1/2) step, off by at most step / 2: checked when the
 * table is laid out), two fields to a word, and the fill streams THOSE: it composes the program into
 * single-precision coefficients over the codes per evaluation, together with an error bound that covers the half
 * step, its own single-precision arithmetic and the reference's double roundings, and bins every sample whose bin
 * coordinate lies further than that bound from the nearest bin edge straight from its codes -- that bin IS the
 * reference's.  The few samples in 10^4 that lie closer go into a queue in LDS and are binned at the end of the
 * stream from their float values with the reference's arithmetic, as are rows outside the windows and the granules
 * that straddle an edge of the ordered observable.  Parameters that are not finite, or so large that the bound
 * reaches an eighth of a bin, switch the codes off for that evaluation (the float columns are streamed).  BASELINE
 * config 3 streams 4 bytes per sample instead of 8.  Histograms, norms and NLL stay bit-identical (parity tests:
 * on / off, the CPU restatement, samples within ulps of the transformed edges, rows outside the windows, queues
 * that overflow).  enable = 0: stream the float columns; 1: use the codes where they apply; -1: the library's
 * default (on unless the environment says SXMC_CODES=0). */
int sxmc_group_set_codes(sxmc_group_t g, int enable);
/* Boxes (default: where they pay; needs codes on, the histogram in LDS, exactly two written observables).  The ordered form
 * makes an observable written by ONE-field systematics a per-granule constant.  An observable that is resolution-scaled
 * (pdfz.cpp:326-329: x += p * (x - t), t a field nothing writes) depends on two fields and has no order -- but every
 * IEEE operation of its program is monotone in each operand, so the reference's own operations applied to the CORNERS
 * of a box [xmin, xmax] x [tmin, tmax] (the corner chosen by the coefficient's sign) bound the result of every row
 * inside the box from both sides, exactly: interval arithmetic whose endpoints round the way the values between them do.
 * The boxed copy sorts the rows of a bucket by (stratum of x - t, x), keeps the box of every 256-row granule (16 bytes), and
 * the fill (fill_boxed_kernel) works out per evaluation, one lane per granule, whether both ends of the box's image land
 * in one bin: then so does every row, and the observable costs nothing per sample.  Granules whose image straddles an
 * edge (a few per cent at BASELINE config 3, more for large resolution parameters) are binned from their float columns
 * with the reference's arithmetic.  The OTHER written observable is streamed as one 16-bit code per row (the codes above,
 * one field): BASELINE config 3 streams 2 bytes per sample instead of 4.  Any value or coefficient that is not finite
 * sends its granule (or the whole evaluation) to the float columns.  Histograms, norms and NLL stay bit-identical
 * (tests/test_gpu_boxed.py: against the ordered form, the float stream and the CPU restatement).  enable = -1 (default):
 * where it pays (at least four granules per bin of the boxed observable, stratum and bucket), TOGETHER WITH the ordered plan
 * (below); 1: wherever it applies, the boxed plan alone (tests); 0: never (the ordered / bucketed forms).  Lockstep sets
 * and the look-ahead pass use the ordered form. */
int sxmc_group_set_boxes(sxmc_group_t g, int enable);
/* With enable = -1 the boxed plan comes with an ORDERED TWIN.  How many boxes straddle an edge depends on the parameters of
 * the evaluation (the image of a box is |dx'/dx| dx + |dx'/dt| dt wide: it grows with the resolution parameter): at BASELINE
 * config 3 the boxed fill takes 65-67 us at a resolution parameter of 0, 76 at 0.05, 84 at 0.07, 131 at 0.2, the ordered
 * one 82-85 whatever the parameters (one box, profiles/r05_boxed_crossover.log).  Both plans stay resident -- the boxed tables with their partition
 * and launch shape, the ordered ones with theirs -- and every fill launches ONE of them: the ordered one until told
 * otherwise, so a caller that never asks runs the ordered form.
 *   sxmc_group_adapt_fill_form: waits for the group's stream, reads the parameters the evaluators are bound to back from
 *   the device, runs the reference's operations on the corners of a box of the tables' mean extents and takes the boxed
 *   form while its image is narrower than the limit (sxmc_group_set_box_limit, bins of the boxed observable; default
 *   0.12; back to boxed below 0.8 of it), the ordered form beyond.  *form: 1 boxed, 2 ordered, 0 the plan has one form
 *   only; *changed: it differs from the form of the launches so far -- recorded graphs of the group's steps keep
 *   replaying the OLD form (both stay valid) until they are recorded again.  The walks of this repository
 *   (sxmc::MCMC, sxmc_amd/mcmc.py) ask at set-up and after every flush of their jump buffer.  Not while a graph is being
 *   recorded.  Results do not depend on the form.
 *   sxmc_group_set_fill_form: 1 or 2 by hand (tests, measurements); sxmc_group_fill_form: the current one. */
int sxmc_group_set_box_limit(sxmc_group_t g, double bins);
int sxmc_group_adapt_fill_form(sxmc_group_t g, int* form, int* changed);
int sxmc_group_set_fill_form(sxmc_group_t g, int form);
int sxmc_group_fill_form(sxmc_group_t g, int* form);
/* What the codes of the group's current plan amount to: members whose fill streams codes, rows they hold, rows marked
 * "ask the exact columns" (outside a window) and rows marked "never counted" (not finite, or granule padding). */
int sxmc_group_codes_info(sxmc_group_t g, int* members, unsigned long long* rows, unsigned long long* exact_rows,
                          unsigned long long* never_rows);
/* The windows the codes of member `member` were cut from: field m of the streamed ones has code
 * floor((x - base[m]) / step[m]); *nfields = how many (0: the member's fill does not stream codes).  base, step: room for
 * SXMC_MAX_QSLOTS (4) doubles each.  For tests that place samples relative to the code cells. */
int sxmc_group_codes_windows(sxmc_group_t g, int member, int* nfields, double* base, double* step);
/* Cap on the per-workgroup queues of ambiguous rows of a fill over codes: 2^log2_entries entries, 9 .. 11; 0 (default):
 * as many as fit beside the histogram.  Smaller queues fill up and are emptied in the middle of the stream, and whole
 * granules are handed to the float columns; the RESULTS do not depend on it (tests/test_gpu_codes.py). */
int sxmc_group_set_codes_queue_log(sxmc_group_t g, int log2_entries);
/* Run-time kernels (default on).  The fill is fastest as straight-line code with the program of systematics
 * (apply_systematic, pdfz.cpp:306-331: which systematic writes which column, in which order, with how many
 * polynomial coefficients) fixed at compile time.  The library carries such kernels for a handful of programs;
 * for any other program of at most 8 systematics and 16 coefficients in all it compiles the same kernel template
 * with hiprtc when the group's launch plan is built (about half a second per program and process, cached) and
 * launches it like a built-in one -- bucketing and sparse counting included.  Off, or when hiprtc fails, such
 * programs run the kernel that decodes the program at run time (same results; sxmc_group_launch_info says why).
 * Results are bit-identical either way (same source, same flags: -ffp-contract=off). */
int sxmc_group_set_runtime_kernels(sxmc_group_t g, int enable);
/* One text line per fill launch of the group's current plan: members, shape, where the histogram lives, how the
 * program runs (builtin / runtime / decoded / generic), how the table is streamed (rows / prebinned / bucketed),
 * launch shape.  For logs and tests. */
int sxmc_group_launch_info(sxmc_group_t g, char* out, size_t n);
/* 1 (default): sxmc_group_eval_nll_async / sxmc_group_mcmc_step_async write the lookup table
 * (lut[j * E + i], the array eval_pdf produces at pdfz.cpp:411-436) as they consume it.  0: the table is
 * an intermediate nobody reads (the MCMC loop, mcmc.cpp:264-348), so it is not written, and the event
 * sum of nll_kernels.cpp:89-116 runs over the DISTINCT tuples of event bins, each log term weighted by
 * the number of events sharing the tuple: sum_i log(s_i) = sum_k n_k log(s_k).  Same value up to
 * rounding (the terms are added in another order); the work no longer grows with the number of
 * events.  sxmc_group_eval_async always writes the table. */
int sxmc_group_set_lut_output(sxmc_group_t g, int enable);
/* CORRELATED PROPOSALS (opt-in; NULL, the default, is the reference's diagonal proposal, bit for bit).  With a factor
 * set, every step end this group launches -- sxmc_group_step_async in all its forms (one-workgroup, cooperative,
 * two-launch, fused), sxmc_group_mcmc_step_async, sxmc_group_finish_step_async, sxmc_group_finish_columns_step_async --
 * writes the next proposal as
 *     v_proposed[i] = v_current[i] + d_i,   d_i = sum_{j <= i} L_ij z_j   for a free parameter i (jump width > 0),
 *     v_proposed[i] = v_current[i]                                        for a fixed one,
 * where z is exactly the diagonal proposal's draw (same generators, order and offsets; z_j = 0 for a fixed j), d_i
 * starts at 0 and takes its terms in ascending j, each as ONE fused multiply-add in double, and the final addition is
 * rounded once.  The widths d_jump_width still say which parameters are free; their magnitudes are not read.
 * LAYOUT: d_factor holds P x P doubles (P = nparameters), COLUMN-major: L_ij at d_factor[j * P + i], so that lanes
 * i, i + 1, ... read consecutive addresses for a fixed j.  Only j <= i is read.  The pointer is BORROWED: it must stay
 * valid while steps are in flight or recorded in a graph; its CONTENTS may change between steps (a re-tuning rewrites
 * them in place, and recorded graphs stay valid).  The product is formed before the step end waits for the event sums.
 * At step time SXMC_ERR_SHAPE beyond 256 parameters or 256 signals (the step end's unstaged form has no such product).
 * The look-ahead pass and lockstep sets have no correlated form: with a factor set on a member group
 * sxmc_multigroup_step_async and sxmc_multigroup_lookahead_step_async return SXMC_ERR_STATE, and
 * sxmc_group_lookahead_supported answers 0. */
int sxmc_group_set_proposal_factor(sxmc_group_t g, const double* d_factor);
/* WEIGHTED DATA EVENTS (opt-in; without weights a group runs the kernels it ran before, bit for bit).  THE LAW
 * (restated for tests in tests/weighted_events_reference.py):
 *   - event i has a weight w_i, a finite double >= 0; the log-likelihood's event term becomes sum_i w_i log(s_i), with
 *     s_i exactly the unweighted s (same look-ups, same -1 / -2 / NaN rules, same s > 0 guard).  nll_total is untouched.
 *   - rows are CLASSES (sxmc_group_set_lut_output off): the class weight is W_k = sum of w_i over the events of class k
 *     in ASCENDING EVENT INDEX, in double, added one by one; a row's term is W_k * log(s_k), rounded once; the terms are
 *     added in the order and partition of the unweighted kernels.
 *   - rows are EVENTS (lut_output on, and sxmc_launch_nll_event_chunks_weighted): the term is w_i * log(s_i); the
 *     lookup table is written as before.
 * Two exact consequences: weights all 1.0 give every partial sum and every chain of the unweighted group as bytes; and
 * integer weights m_i >= 1 with lut_output off give, as bytes, the unweighted walk over the data set in which event i is
 * repeated m_i times.
 * h_weights is a HOST array of nevents doubles and is copied; NULL, 0 switches weights off.  SXMC_ERR_INVALID: a weight
 * that is NaN, infinite or negative (the message names the first such index).  SXMC_ERR_STATE: under a graph recording;
 * and, at the next evaluation, a count that differs from the members' evaluation points.  Setting weights invalidates
 * the event classes, as new points do.  The weights reach sxmc_group_eval_nll_async, sxmc_group_mcmc_step_async and
 * sxmc_group_step_async in all its forms (one-workgroup, cooperative, two-launch, fused); sxmc_group_finish_step_async and
 * sxmc_group_finish_columns_step_async finish whatever partial sums they are given.  There is no weighted lockstep set,
 * look-ahead pass or in-place column sum: with weights set, sxmc_multigroup_step_async,
 * sxmc_multigroup_lookahead_step_async and sxmc_group_eval_columns_nll_async return SXMC_ERR_STATE, and
 * sxmc_group_lookahead_supported answers 0. */
int sxmc_group_set_event_weights(sxmc_group_t g, const double* h_weights, size_t nevents);
/* The re-tuning of a correlated proposal, on the host (no device call; usable without a GPU).  rows: nrows kept rows
 * of the jump buffer, nparameters + 1 floats each (the last is the NLL, not read); new_widths: the widths AFTER the
 * reference's re-tuning (<= 0: a fixed parameter).  With every float widened to double and every sum taken
 * sequentially in row order:
 *   mean_j = (sum_r x_rj) / nrows;  S_jk = sum_r (x_rj - mean_j)(x_rk - mean_k);
 *   R_jk = S_jk / (sqrt(S_jj) sqrt(S_kk)), R_jj = 1; a column with S_jj == 0 (or no rows) is decoupled: its row and
 *   column of R are the identity's;  R_b = (1 - b) R + b I off the diagonal, 1 on it, b = shrinkage in (0, 1];
 *   T = the Cholesky factor of R_b row by row (Cholesky-Banachiewicz); a pivot that is not positive doubles b (capped at
 *   1, where T = I) and the factorisation starts again;  L = diag((double)new_widths) T.
 * Rows and columns of fixed parameters are zero.  factor: nparameters^2 doubles in sxmc_group_set_proposal_factor's
 * layout (all of them written); shrinkage_used (optional): the b that succeeded.  nrows == 0: L = diag(new_widths).
 * SXMC_ERR_INVALID: a null argument (rows may be null when nrows == 0), nparameters < 1, shrinkage outside (0, 1]. */
int sxmc_proposal_factor(const float* rows, size_t nrows, int nparameters, const float* new_widths, double shrinkage,
                         double* factor, double* shrinkage_used);
/* CORRELATED GAUSSIAN CONSTRAINTS (opt-in; NULL, the default, is the reference's one independent Gaussian per parameter,
 * bit for bit).  With a whitening matrix W set, every step end this group launches (the same list as for the proposal
 * factor above) replaces the constraint terms of nll_total by those of the whitened residuals.  Per evaluation:
 *     x_i   = (p_i - mean_i) / sigma_i   for sigma_i > 0 (exactly the division made without W), otherwise x_i = 0;
 *     r_i   = 0, then for j = 0 .. i ascending  r_i = fma(W_ij, x_j, r_i)   (one fused multiply-add in double per term);
 *     pen_i = 0.5 * r_i * r_i             for sigma_i > 0, otherwise -0.0 (which changes no sum);
 * pen_i takes THE SLOT constraint i has without W: nll_total adds the same number of terms in the same order, the
 * negative-rate and NaN rules (1e18) unchanged.  Mathematically sum pen_i = 0.5 x^T rho^-1 x for W = T^-1, T the
 * Cholesky factor of the correlation matrix rho (sxmc_constraint_whitening below).  Two exact consequences: with W = I,
 * r_i = fma(1, x_i, 0) = x_i and every chain is the uncorrelated chain's bytes; a block-diagonal rho gives inside each
 * block the bytes that block gives alone.  A fixed parameter may take part: its x is constant.
 * LAYOUT: d_whitening holds P x P doubles (P = nparameters), COLUMN-major: W_ij at d_whitening[j * P + i]; only j <= i is
 * read.  The pointer is BORROWED: it must stay valid while steps are in flight or recorded in a graph.  The product is
 * formed before the step end waits for the event sums.  At step time SXMC_ERR_SHAPE beyond 256 parameters or 256
 * signals.  The look-ahead pass and lockstep sets have no such form: with a matrix set on a member group
 * sxmc_multigroup_step_async and sxmc_multigroup_lookahead_step_async return SXMC_ERR_STATE, and
 * sxmc_group_lookahead_supported answers 0 without touching the group. */
int sxmc_group_set_constraint_whitening(sxmc_group_t g, const double* d_whitening);
/* The whitening matrix of a correlation matrix, on the host (no device call; usable without a GPU).  rho: P x P doubles
 * (symmetric, so either major order) over the parameter vector in the walk's order (sources, then <systematic>_<j>);
 * sigmas: the P constraint widths (<= 0: no constraint); W: P x P doubles in sxmc_group_set_constraint_whitening's layout,
 * all of them written on success (zeros above the diagonal).
 * SXMC_ERR_INVALID, the message naming row and column, when rho has an entry that is not finite or lies outside
 * [-1, 1], a diagonal entry that is not exactly 1, is not exactly symmetric, or gives a parameter with sigma_i <= 0 a
 * non-zero off-diagonal entry -- checked in that order, each over the rows ascending.
 * Every operation is one double operation rounded once:
 *   T = the Cholesky factor of rho, row by row: for i, for j = 0 .. i:  s = rho_ij;  for k = 0 .. j-1 ascending
 *       s = s - T_ik * T_jk;  j == i: a pivot s that is not > 0 is SXMC_ERR_INVALID "not positive definite at parameter
 *       i" (no shrinkage: the user's matrix is the model), T_ii = sqrt(s);  j < i: T_ij = s / T_jj.
 *   W = T^-1 by forward substitution, row by row: W_ii = 1 / T_ii;  for j = 0 .. i-1:  s = 0;  for k = j .. i-1
 *       ascending  s = s + T_ik * W_kj;  W_ij = -(s * W_ii).
 *   A product whose T_ik is exactly zero is skipped in both loops, and a W_ij all of whose products were skipped is +0:
 *   a parameter outside every correlated group has W_ii = 1 and +0 in the rest of its row. */
int sxmc_constraint_whitening(const double* rho, const double* sigmas, int P, double* W);
/* WEIGHTED MONTE CARLO SAMPLES (opt-in; an evaluator without multiplicities runs the kernels it ran before).  Histograms
 * and normalisations are `unsigned` counts and every consumer is linear in them, so a row's weight enters as an integer
 * MULTIPLICITY m_i, a fixed-point weight on a power-of-two scale 2^k; only the fill changes (it adds m_i where it added 1)
 * and the scale cancels exactly wherever bins, norm and n_mc meet, since all three carry it.
 * THE LAW of the quantiser, on the host (no device call; usable without a GPU; restated in
 * tests/sample_weights_reference.py):
 *   - a weight is a finite double >= 0 (-0.0 is 0); one that is negative or not finite is SXMC_ERR_INVALID and the
 *     message names the first such row;
 *   - max_total = 0 means 2^32 - 1; a larger value is SXMC_ERR_INVALID;
 *   - for a candidate k, m_i = (unsigned) nearbyint(ldexp(w_i, k)), rounding half to even;
 *   - k is the LARGEST integer in [-32, 24] for which every m_i <= 2^32 - 1 and sum m_i <= max_total;
 *   - no such k, or sum m_i == 0 at the chosen one (no rows, every weight 0): SXMC_ERR_INVALID;
 *   - *total = sum m_i, summed in 64 bits; *log2_scale = k (both optional).
 * Consequences: non-negative integer weights that fit come back as m_i = w_i * 2^k exactly; all-ones weights come back all
 * equal to 2^k.  m: n words, written (partly, on failure). */
int sxmc_sample_multiplicities(const double* w, size_t n, unsigned long long max_total, unsigned* m, int* log2_scale,
                               unsigned long long* total);
/* The multiplicities of an evaluator's table rows, one word per row (nsamples must be sxmc_hist_nsamples'), from host or
 * device memory; the library keeps its own device copy, padded with 0 to the columns' pitch (the float columns' row
 * padding stays NaN).  THE DEVICE LAW: bins[b] = sum of m_i over the rows the reference's arithmetic puts into bin b;
 * norm = sum of m_i over the rows that pass the domain test, the in-domain row whose index comes out one past the end
 * included; nothing else about an evaluation changes.  All m_i == c give the unweighted evaluator's pdf values as bytes;
 * m in {0, 1, 2, ...} gives the counts of the table with row i repeated m_i times.
 * Allowed before the evaluator's first evaluation and before it joins a group: SXMC_ERR_STATE afterwards.  A total beyond
 * 2^32 - 1: SXMC_ERR_INVALID.  Evaluators made from this one by sxmc_hist_create_shared share the column.
 * A weighted member's fill (fill_body with PREW = kPreWeighted, sxmc_amd/csrc/fill_kernels.inc.h) streams the table as
 * it is (no pre-binned column, no bucketed, ordered or boxed copy, no codes,
 * no run-time specialisation: sxmc_group_launch_info says "weighted"), 20 bytes per row and float column where the rows
 * form streams 16; the unweighted members of the same group keep the forms they plan alone.  A group with a weighted member
 * evaluates in the dense flavour (no sparse event-bin counters).  With a weighted member sxmc_multigroup_step_async and
 * sxmc_multigroup_lookahead_step_async return SXMC_ERR_STATE and sxmc_group_lookahead_supported answers 0 without touching
 * the group; sxmc_group_set_fill_form on a group whose members are all weighted returns SXMC_ERR_STATE. */
int sxmc_hist_set_sample_multiplicities(sxmc_hist_t h, const unsigned* m, size_t nsamples, int on_device);
/* sum m_i, or the row count when no multiplicities are set: what n_mc is for either kind (sxmc_hist_nsamples stays the
 * row count). */
int sxmc_hist_sample_total(sxmc_hist_t h, unsigned long long* total);
/* The multiplicities back on the host, n = the row count; all 1 when none are set (*is_set, optional, says which;
 * h_m NULL with n 0 asks that question alone). */
int sxmc_hist_get_sample_multiplicities(sxmc_hist_t h, unsigned* h_m, size_t n, int* is_set);
int sxmc_group_eval_async(sxmc_group_t g, int do_eval_pdf, sxmc_stream_t s);
/* As sxmc_group_eval_async(g, 1, s) followed by nll_event_chunks (nll_kernels.cpp:89-116) over
 * the members' lookup table, with the table lookup and the event sum fused in one kernel: the
 * lut is still written (it is the API contract, mcmc.cpp:232-236; unless sxmc_group_set_lut_output
 * switched that off) but not re-read.  Requires
 * all members to share the same number of evaluation points.  Writes one partial sum per
 * block: d_sums[0 .. *npartial_out).  d_sums must hold at least 1024 doubles. */
int sxmc_group_eval_nll_async(sxmc_group_t g, sxmc_stream_t s,
                              const double* d_pars, const double* d_nexpected,
                              const unsigned* d_n_mc, const short* d_source_id,
                              const unsigned* d_norms, double* d_sums, int* npartial_out);
/* EXPERIMENTAL (measured ~3% slower per step than sxmc_group_eval_nll_async + finish_nll_jump_pick_combo at
 * E = 1e5: every workgroup pays an agent-scope release and a ticket on one counter).
 * One whole MCMC step (mcmc.cpp:264-271 + 314-348) as three launches: zero, fill of all members, and
 * one kernel doing lookup + nll_event_chunks + finish_nll_jump_pick_combo (the workgroup that finishes
 * its event partial sum last also runs the step end).  The NLL is evaluated at d_v_proposed, which is
 * also the members' parameter buffer in an MCMC walk (mcmc.cpp:241).  Arguments as
 * finish_nll_jump_pick_combo (nll_kernels.h:190-207) without the partial-sum buffer. */
int sxmc_group_mcmc_step_async(sxmc_group_t g, sxmc_stream_t s, const double* d_means, const double* d_sigmas,
                               sxmc_rng_state* d_rng, double* d_nll_current, double* d_nll_proposed,
                               double* d_v_current, double* d_v_proposed, int* d_accepted, int* d_counter,
                               float* d_jump_buffer, int nparameters, size_t nsources,
                               const float* d_jump_width, const double* d_nexpected, const unsigned* d_n_mc,
                               const short* d_source_id, const unsigned* d_norms, int debug_mode);
/* finish_nll_jump_pick_combo (nll_kernels.cpp:230-271; arguments as sxmc_launch_finish_nll_jump_pick_combo,
 * one workgroup of 128) launched TOGETHER with the zeroing the group's next evaluation would start with:
 * that evaluation then skips its zero launch (3 launches per MCMC step instead of 4).  For a walk that does
 * not look at them between steps: the group's histograms and the members' normalisation slots are CLEARED
 * when this returns (sxmc_hist_get_bins gives SXMC_ERR_STATE until an evaluation with do_eval_pdf = 0).
 * Must follow an evaluation of the group on the same stream; d_norms is the array the members'
 * normalisations are bound into. */
int sxmc_group_finish_step_async(sxmc_group_t g, sxmc_stream_t s, size_t npartial_sums, const double* d_sums,
                                 const double* d_means, const double* d_sigmas, sxmc_rng_state* d_rng,
                                 double* d_nll_current, double* d_nll_proposed, double* d_v_current,
                                 double* d_v_proposed, int* d_accepted, int* d_counter, float* d_jump_buffer,
                                 int nparameters, size_t nsources, const float* d_jump_width,
                                 const double* d_nexpected, const unsigned* d_n_mc, const short* d_source_id,
                                 const unsigned* d_norms, int debug_mode);
/* MIXED FITS: a walk whose lookup table has columns the group does not write -- kernel-density signals
 * (sxmc_kde_eval_on_stream_async) beside the histogram members.  sxmc_group_set_columns describes the walk's `nsignals`
 * columns in signal order, a host array: member_of_signal[j] >= 0 is that member of `g`, looked up from its histogram;
 * -1 is a dense column somebody else writes.  Every member must appear exactly once; anything else (a null argument,
 * nsignals < 1, an index below -1 or beyond the members, a member twice or not at all) is SXMC_ERR_INVALID.  The table
 * is uploaded here, once (waits for the group's last stream; not while a graph is recorded): the two step entries below
 * neither copy nor allocate. */
int sxmc_group_set_columns(sxmc_group_t g, int nsignals, const int* member_of_signal);
/* The group's zero and fill exactly as sxmc_group_eval_async(g, 1, s) does them (boxed, ordered, codes, the event-bin
 * counters of histograms beyond LDS, the zero launch skipped after a clearing step end), then nll_event_chunks
 * (nll_kernels.cpp:89-116) over the mixed table with the histogram columns looked up IN PLACE (columns_kernels.hip):
 * d_sums[0 .. grid * block) receives, bit for bit, what sxmc_launch_nll_event_chunks(grid, block, ...) gives over the
 * fully materialised table -- lane t sums events t, t + grid * block, ... in index order, the terms of an event in
 * signal order, a histogram column's value being eval_pdf's (pdfz.cpp:423-434) from the descriptors
 * sxmc_group_eval_async's lookup would be given, so sparse plans look up what they count.  Dense column j is
 * d_lut[j * nevents + i], valid on `s` when the kernel runs; the histogram members' columns of d_lut are NOT written
 * (d_lut may be null when there is no dense column).  d_norms: the walk's normalisation array in signal order (a
 * member's own slot is read for its bin norm).  Requires sxmc_group_set_columns, members that share one set of points
 * of `nevents` rows, 1 <= block <= 256, at most 1024 columns.  Capture-safe once the group has evaluated.
 * MEASURED SLOWER than materialising (sxmc_group_eval_async(g, 1, s) + sxmc_launch_nll_event_chunks) where the event
 * sum is large: the look-ups, a double division each, sit on the event sum's `grid` workgroups -- 64 in a walk --
 * instead of the whole device.  tests/cpp/mixed_walk --bench, 20 000 steps, twice, on two cards: 8 histogram signals of
 * 4e6 samples + 2 kernel-density signals, 4.75e4 events, graph replays of 100 steps: 6 240 / 6 237 steps/s in place
 * against 6 312 / 6 259 materialised (-0.8 %), and 6 387 / 6 390 against 6 477 / 6 482 (-1.4 %, the repeats agreeing
 * to 0.1 %); 1 histogram + 2 kernel-density signals, 874 events (one event to a lane, one launch less): 25 580 / 25 720
 * against 24 620 / 24 620, and 25 210 / 25 060 against 24 190 / 24 150 (+4 %).  So sxmc::MCMC materialises by default
 * and takes this entry on request (MCMC::columns_in_place). */
int sxmc_group_eval_columns_nll_async(sxmc_group_t g, sxmc_stream_t s, const float* d_lut, size_t nevents,
                                      const double* d_pars, const double* d_nexpected, const unsigned* d_n_mc,
                                      const short* d_source_id, const unsigned* d_norms, double* d_sums, int grid,
                                      int block);
/* sxmc_group_finish_step_async for a mixed fit (same arguments): the step end -- finish_nll_jump_pick_combo, nll_total
 * over all signals -- runs over the `nsignals` columns of sxmc_group_set_columns, not over the members; the clearing
 * covers the group's histograms and its MEMBERS' normalisation slots only: the slots of dense columns are left as they
 * are (a kernel-density signal no floating parameter touches keeps the norm of its last evaluation).  Follows
 * sxmc_group_eval_columns_nll_async, or sxmc_group_eval_async + sxmc_launch_nll_event_chunks, on the same stream. */
int sxmc_group_finish_columns_step_async(sxmc_group_t g, sxmc_stream_t s, size_t npartial_sums, const double* d_sums,
                                         const double* d_means, const double* d_sigmas, sxmc_rng_state* d_rng,
                                         double* d_nll_current, double* d_nll_proposed, double* d_v_current,
                                         double* d_v_proposed, int* d_accepted, int* d_counter, float* d_jump_buffer,
                                         int nparameters, size_t nsources, const float* d_jump_width,
                                         const double* d_nexpected, const unsigned* d_n_mc, const short* d_source_id,
                                         const unsigned* d_norms, int debug_mode);
/* One whole MCMC step (mcmc.cpp:264-271 + 314-348) for a walk that reads neither histograms, normalisations nor
 * the lookup table between steps: the fill of all members, then lookup + nll_event_chunks (nll_kernels.cpp:89-116)
 * + nll_event_reduce + nll_total + finish_nll_jump_pick_combo (:230-271) + the clearing the next evaluation
 * would start with (so that one skips its zero launch).  The step end runs as ONE workgroup in ONE launch
 * (2 launches per step) where it is small -- at most 256 row x member look-ups and 65 536 counters: BASELINE
 * config 1 -- and as two launches otherwise (lookup + event sum over many workgroups,
 * then step end beside the clearing: what sxmc_group_eval_nll_async + sxmc_group_finish_step_async do).  A row
 * costs one double division per member and a log, so beyond a few hundred of them one CU is slower than the
 * extra launch (measured: config 3, ~8000 x 12, 59 us against 15.6 us; bench_pdfz, 1000 x 1, 8 against 7;
 * config 1, 10 x 2, 7.0 against 7.6).
 * The NLL is evaluated at d_v_proposed, which is also the members' parameter buffer in a walk (mcmc.cpp:241).
 * Histograms and normalisations are CLEARED when this returns, as after sxmc_group_finish_step_async; the
 * lookup table is written only when sxmc_group_set_lut_output is on.  The one-workgroup form adds the log terms
 * in the many-workgroup form's order -- its waves' sums block of 128 rows by block -- so the NLL, and with it the chain,
 * is the same bit for bit whichever form ends the step (tests/test_gpu_step_end_forms.py). */
int sxmc_group_step_async(sxmc_group_t g, sxmc_stream_t s, const double* d_means, const double* d_sigmas,
                          sxmc_rng_state* d_rng, double* d_nll_current, double* d_nll_proposed,
                          double* d_v_current, double* d_v_proposed, int* d_accepted, int* d_counter,
                          float* d_jump_buffer, int nparameters, size_t nsources,
                          const float* d_jump_width, const double* d_nexpected, const unsigned* d_n_mc,
                          const short* d_source_id, const unsigned* d_norms, int debug_mode);
/* LOCKSTEP CHAINS.  Several chains over the SAME sample tables -- the fake experiments in flight on one GPU,
 * BASELINE config 4's per-GPU shape: evaluators made with sxmc_hist_create_shared, same systematics, each chain
 * with its own group, parameters, data and state -- evaluate different parameter vectors on identical samples.
 * Stepped one by one each evaluation streams the tables again while the vector units idle under the stream
 * (config 3: 175 us of stream against 122 us of arithmetic).  A multigroup steps 2-4 such chains TOGETHER: one
 * fill pass streams the tables once and bins every sample under each chain's parameters into that chain's LDS
 * histogram (bytes per evaluation divided by the number of chains; per chain exactly the operations of its own
 * fill, so its counts are bit-identical), then every chain's own step end runs as in sxmc_group_step_async.
 * Chains advanced this way walk exactly the chains they walk alone (tests).  The kernel is compiled through
 * hiprtc for the chains' program.  SXMC_ERR_STATE (with the reason) when the chains cannot share a pass --
 * different tables, systematics or launch configuration, histograms beyond LDS or not fitting LDS together, a
 * run-time decoded program: step them separately then.  args: one sxmc_step_args per chain, in group order. */
typedef struct {
  const double* d_means;
  const double* d_sigmas;
  sxmc_rng_state* d_rng;
  double* d_nll_current;
  double* d_nll_proposed;
  double* d_v_current;
  double* d_v_proposed;
  int* d_accepted;
  int* d_counter;
  float* d_jump_buffer;
  int nparameters;
  size_t nsources;
  const float* d_jump_width;
  const double* d_nexpected;
  const unsigned* d_n_mc;
  const short* d_source_id;
  const unsigned* d_norms;
  int debug_mode;
} sxmc_step_args; /* the arguments of finish_nll_jump_pick_combo (nll_kernels.h:190-207) */
typedef struct sxmc_multigroup* sxmc_multigroup_t;
/* groups: borrowed; they must outlive the multigroup (destroy it first). */
int sxmc_multigroup_create(const sxmc_group_t* groups, int ngroups, sxmc_multigroup_t* out);
int sxmc_multigroup_destroy(sxmc_multigroup_t mg);
int sxmc_multigroup_step_async(sxmc_multigroup_t mg, sxmc_stream_t s, const sxmc_step_args* args);
/* The chains' step ends (lookup + event sum; finish_nll_jump_pick_combo + clearing) share two launches for the whole
 * set -- chain = blockIdx.y, every workgroup doing what it does for a chain stepped alone, so the chains are the
 * same bit for bit -- instead of two launches per chain.  Default 1; 0: chain by chain (measurement / tests; in the
 * measurement build SXMC_JOINT_STEP_END=0 in the environment makes that the default of multigroups created afterwards,
 * for A/B runs of whole programs: profiles/r03_lockstep_step_ends.log). */
int sxmc_multigroup_set_joint_step_end(sxmc_multigroup_t mg, int enable);
/* LOOK-AHEAD WALK: one chain, two likelihood evaluations per pass over the tables.  A Metropolis step that rejects
 * (jump_decider, nll_kernels.cpp:56-86) leaves the chain where it was, and the next proposal -- current vector +
 * jump width x the next deviates (pick_new_vector, :30-53) -- is then known BEFORE the step is decided.  A
 * multigroup of exactly two groups over the same tables -- groups[0]'s evaluators bound to the chain's proposal
 * (args->d_v_proposed, args->d_norms), groups[1]'s to the look-ahead vector (d_v_lookahead, d_norms_lookahead) --
 * evaluates both in ONE fill pass (the lockstep kernel); the step end decides the step from the first and, if it
 * rejected, the FOLLOWING step from the second at once, then writes the next proposal and the next look-ahead
 * vector.  A pass advances the chain by 1 + P(reject) steps on average for about 1.2 x the time of a
 * single evaluation.  The chain is the sequential one bit for bit: every row of the jump buffer, the counters, the
 * generator states (pre-fetching: Brockwell, J. Comput. Graph. Stat. 15 (2006)).  d_cap (device, optional): the
 * value of *args->d_counter at which the walk stops -- a pass takes its second step only below it and does
 * nothing at or beyond it, so a caller that needs exactly n steps launches passes until the counter says n.
 * Needs the lookup table off (sxmc_group_set_lut_output(g, 0)), histograms in LDS and at most 256 parameters.
 * sxmc_lookahead_begin: the first look-ahead vector of a walk, from the state sxmc_launch_pick_new_vector left. */
int sxmc_multigroup_lookahead_step_async(sxmc_multigroup_t mg, sxmc_stream_t s, const sxmc_step_args* args,
                                         double* d_v_lookahead, const unsigned* d_norms_lookahead, const int* d_cap);
/* *ok = 1 when a walk over this group (evaluation points set, buffers bound) can be taken by the look-ahead pass and
 * stay the sequential chain bit for bit.  0: histograms beyond LDS, a materialised lookup table, members with
 * different points -- or a problem so small (at most 256 look-ups per step) that the sequential step ends in the
 * one-workgroup form, which the pass has no counterpart of: walk sequentially then. */
int sxmc_group_lookahead_supported(sxmc_group_t g, int* ok);
int sxmc_lookahead_begin(sxmc_stream_t s, int nparameters, const sxmc_rng_state* d_rng, const float* d_jump_width,
                         const double* d_v_current, double* d_v_lookahead);
/* Kernels launched by the last sxmc_group_step_async (2 or 3, see there; +1 when the histograms had to be
 * zeroed first). */
int sxmc_group_last_step_launches(sxmc_group_t g, int* launches);
/* 0: sxmc_group_step_async always takes its three-launch route (measurement / tests).  Default 1. */
int sxmc_group_set_tail_kernel(sxmc_group_t g, int enable);
/* The step end of sxmc_group_step_async as ONE cooperative launch (default 1; SXMC_COOP_STEP_END=0 in the environment
 * changes the default): where the event sum is at most 128 workgroups of 128 rows (up to 16 384 rows: BASELINE
 * configs 2 and 3 with event classes), the look-ups + event sum (nll_event_chunks, nll_kernels.cpp:89-116), the step
 * end (finish_nll_jump_pick_combo, :230-271) and the clearing for the next evaluation run in one kernel: every
 * workgroup of the event sum hands its partial sum to a finisher workgroup through a slot of its own (one device-scope
 * store; no fences, no counters); the finisher -- which has meanwhile done everything of the step end that does not
 * need the sums -- polls the slots, finishes the step and empties them, which tells the other workgroups that every
 * look-up is done and the histograms may be cleared.  Same partial sums, same order: the chain is the one the
 * separate launches walk, bit for bit.  2 launches per step instead of 3: 14.2 us against 9.5 + 6.8 at BASELINE
 * config 3, 9.3 against 6.1 + 5.3 at config 2 (+10 % evaluations per second).  Every wait inside the kernel is bounded
 * (~0.3 s): a lane that gives up counts a timeout, which sxmc_group_step_end_timeouts reports (0 in any healthy run;
 * the results of a step that timed out are not valid). */
int sxmc_group_set_cooperative_step_end(sxmc_group_t g, int enable);
/* THE WHOLE STEP IN ONE LAUNCH (default 0: built, bit-identical and MEASURED SLOWER than the fill followed by the
 * cooperative step end -- 6 640-6 970 against 6 870-7 260 evaluations/s at BASELINE config 3, DESIGN.md section 4;
 * SXMC_FUSED_STEP=1 in the environment changes the default).  Where the step
 * end is cooperative (above), the plan is a single fill launch with a built-in kernel that has the form (the ordered
 * programs -- BASELINE config 3 --, the empty program over a pre-binned column -- config 2) and at most 256
 * parameters and signals, sxmc_group_step_async launches the fill's workgroups AND the step end's finisher and workers
 * as one grid: the roles start on CUs the fill's first workgroups have left, wait for the fill's workgroups to count
 * themselves done (each after its flush has landed), acquire, and go on as the cooperative step end.  Waits go from
 * later blocks to earlier ones (which the dispatcher has started before them) except the finisher's for its workers;
 * all are bounded and counted like the step end's.  Same arithmetic, same partial sums: the chain is the same bit for
 * bit.  1 launch per step.  A step whose fill is being timed (sxmc_group_profile) is launched unfused, so that the
 * fill's own duration stays measurable. */
int sxmc_group_set_fused_step(sxmc_group_t g, int enable);
/* s: the stream the count is read through (the chain's own; NULL = a blocking copy through the legacy stream, which
 * must not happen while another host thread records a graph). */
int sxmc_group_step_end_timeouts(sxmc_group_t g, sxmc_stream_t s, unsigned* timeouts);
/* Compiles (does not load or run) the fill kernel the library would specialise at run time for a program of
 * systematics -- see sxmc_group_set_runtime_kernels.  Needs no GPU: a build check, and the test hook of the
 * run-time compilation.  ops[i] = type | obs_slot << 4 | extra_slot << 8 | npars << 12 (npars 0 = one coefficient);
 * pre_width: the table's form -- 0 rows, 1 / 2 a pre-binned column of that many bytes per sample, 3 bucketed, 5 bucketed
 * with an ordered observable, 6 with a boxed one; sparse_runs != 0: the kernel for histograms beyond LDS over a bucketed
 * table walked in runs.  *code_bytes (optional): size of the gfx950 code object. */
int sxmc_rtc_compile_check(int nobs, int nslot, int lds_hist, int pre_width, int sparse_runs, const unsigned* ops,
                           int nops, size_t* code_bytes);
/* The same for the lockstep-chains kernel (sxmc_multigroup_step_async), which exists only as a run-time kernel. */
int sxmc_rtc_compile_check_lockstep(int nobs, int nslot, int pre_width, int nchains, const unsigned* ops, int nops,
                                    size_t* code_bytes);
int sxmc_group_synchronize(sxmc_group_t g);
/* Live timing of the dominant kernel (the histogram fill) with HIP events on the stream it is
 * launched on.  enable!=0 starts recording (at most `capacity` launches are kept). */
int sxmc_group_profile(sxmc_group_t g, int enable, int capacity);
int sxmc_group_profile_read(sxmc_group_t g, double* fill_ms_total, int* nlaunches);
/* Algorithmic bytes of one group evaluation, SURVEY 8(d):
 * sum_j 4*N_j*U_j  (fill_read) ; sum_j 4*B_j*w (hist) ; 16*E*S (event) */
int sxmc_group_algorithmic_bytes(sxmc_group_t g, double* fill_read, double* hist, double* event);

/* ---------------------------------------------------------------- NLL / MCMC step kernels --- */
/* Launch points with the argument lists of nll_kernels.h:60-207, preceded by the
 * (grid, block, stream) triple the caller passes to HEMI_KERNEL_LAUNCH (mcmc.cpp:252, 314,
 * 326, 396, 404, 409).  All array arguments are device pointers. */

/* init_device_rngs (nll_kernels.cpp:18-27): state[i] = (seed, subsequence i, offset 0) */
int sxmc_launch_init_device_rngs(int grid, int block, sxmc_stream_t s, int nthreads,
                                 unsigned long long seed, sxmc_rng_state* d_state);
/* pick_new_vector (nll_kernels.cpp:191-197) */
int sxmc_launch_pick_new_vector(int grid, int block, sxmc_stream_t s, int nthreads,
                                sxmc_rng_state* d_rng, const float* d_jump_width,
                                const double* d_current_vector, double* d_proposed_vector);
/* jump_decider (nll_kernels.cpp:200-206) */
int sxmc_launch_jump_decider(int grid, int block, sxmc_stream_t s, sxmc_rng_state* d_rng,
                             double* d_nll_current, const double* d_nll_proposed,
                             double* d_v_current, const double* d_v_proposed,
                             unsigned nparameters, int* d_accepted, int* d_counter,
                             float* d_jump_buffer);
/* nll_event_chunks (nll_kernels.cpp:89-116): thread t of grid*block writes d_sums[t] */
int sxmc_launch_nll_event_chunks(int grid, int block, sxmc_stream_t s, const float* d_lut,
                                 const double* d_pars, size_t ne, size_t ns,
                                 const double* d_nexpected, const unsigned* d_n_mc,
                                 const short* d_source_id, const unsigned* d_norms,
                                 double* d_sums);
/* The same with one weight per event (the law: sxmc_group_set_event_weights): thread t adds d_weights[i] * log(s_i),
 * rounded once, over its events i = t, t + grid*block, ... in index order.  d_weights: ne doubles in DEVICE memory. */
int sxmc_launch_nll_event_chunks_weighted(int grid, int block, sxmc_stream_t s, const float* d_lut,
                                          const double* d_pars, size_t ne, size_t ns,
                                          const double* d_nexpected, const unsigned* d_n_mc,
                                          const short* d_source_id, const unsigned* d_norms,
                                          double* d_sums, const double* d_weights);
/* nll_event_reduce (nll_kernels.cpp:209-212); grid must be 1 */
int sxmc_launch_nll_event_reduce(int grid, int block, sxmc_stream_t s, size_t nthreads,
                                 const double* d_sums, double* d_total_sum);
/* nll_total (nll_kernels.cpp:215-227) */
int sxmc_launch_nll_total(int grid, int block, sxmc_stream_t s, size_t nparameters,
                          const double* d_pars, size_t nsignals, size_t nsources,
                          const double* d_means, const double* d_sigmas,
                          const double* d_events_total, const double* d_nexpected,
                          const unsigned* d_n_mc, const short* d_source_id,
                          const unsigned* d_norms, double* d_nll);
/* The same with correlated constraints (sxmc_group_set_constraint_whitening: law and layout).  d_whitening == NULL:
 * exactly the launch above.  One thread, no staging: any number of parameters. */
int sxmc_launch_nll_total_whitened(int grid, int block, sxmc_stream_t s, size_t nparameters,
                                   const double* d_pars, size_t nsignals, size_t nsources,
                                   const double* d_means, const double* d_sigmas,
                                   const double* d_events_total, const double* d_nexpected,
                                   const unsigned* d_n_mc, const short* d_source_id,
                                   const unsigned* d_norms, double* d_nll, const double* d_whitening);
/* finish_nll_jump_pick_combo (nll_kernels.cpp:230-271); grid must be 1 */
int sxmc_launch_finish_nll_jump_pick_combo(int grid, int block, sxmc_stream_t s,
                                           size_t npartial_sums, const double* d_sums,
                                           size_t nsignals, size_t nsources,
                                           const double* d_means, const double* d_sigmas,
                                           sxmc_rng_state* d_rng, double* d_nll_current,
                                           double* d_nll_proposed, double* d_v_current,
                                           double* d_v_proposed, int* d_accepted,
                                           int* d_counter, float* d_jump_buffer,
                                           int nparameters, const float* d_jump_width,
                                           const double* d_nexpected, const unsigned* d_n_mc,
                                           const short* d_source_id, const unsigned* d_norms,
                                           int debug_mode);
/* The same with a correlated proposal's factor (sxmc_group_set_proposal_factor: law and layout), for walks that have no
 * group to carry it.  d_factor == NULL: exactly the launch above.  SXMC_ERR_SHAPE with a factor and more than 256
 * parameters or signals. */
int sxmc_launch_finish_nll_jump_pick_combo_factor(int grid, int block, sxmc_stream_t s,
                                                  size_t npartial_sums, const double* d_sums,
                                                  size_t nsignals, size_t nsources,
                                                  const double* d_means, const double* d_sigmas,
                                                  sxmc_rng_state* d_rng, double* d_nll_current,
                                                  double* d_nll_proposed, double* d_v_current,
                                                  double* d_v_proposed, int* d_accepted,
                                                  int* d_counter, float* d_jump_buffer,
                                                  int nparameters, const float* d_jump_width,
                                                  const double* d_nexpected, const unsigned* d_n_mc,
                                                  const short* d_source_id, const unsigned* d_norms,
                                                  int debug_mode, const double* d_factor);
/* The same with a proposal factor and a constraint whitening matrix (sxmc_group_set_constraint_whitening: law and
 * layout); either may be NULL, both NULL is exactly the first launch.  SXMC_ERR_SHAPE with either set and more than 256
 * parameters or signals. */
int sxmc_launch_finish_nll_jump_pick_combo_constrained(int grid, int block, sxmc_stream_t s,
                                                       size_t npartial_sums, const double* d_sums,
                                                       size_t nsignals, size_t nsources,
                                                       const double* d_means, const double* d_sigmas,
                                                       sxmc_rng_state* d_rng, double* d_nll_current,
                                                       double* d_nll_proposed, double* d_v_current,
                                                       double* d_v_proposed, int* d_accepted,
                                                       int* d_counter, float* d_jump_buffer,
                                                       int nparameters, const float* d_jump_width,
                                                       const double* d_nexpected, const unsigned* d_n_mc,
                                                       const short* d_source_id, const unsigned* d_norms,
                                                       int debug_mode, const double* d_factor,
                                                       const double* d_whitening);

/* ---------------------------------------------------------------- multi-GPU exchange (RCCL) ----- */
/* Fake experiments shard over the GPUs of a node one experiment per rank with NO data-path collective
 * (sxmc.cpp:59-145 is a loop of independent iterations; every rank holds a replica of the MC tables).  The only
 * exchange is one all-gather, at the end, of the per-experiment intervals (interval.h:22-27: point_estimate,
 * lower, upper, coverage per parameter) from which rank 0 takes the medians (sxmc.cpp:126-145, utils.h:76-90).
 * These entry points are that exchange on RCCL (xGMI between the GPUs of a node): plain float buffers. */
typedef struct sxmc_comm* sxmc_comm_t;
/* One communicator per device, all in THIS process (one host thread per GPU: sxmc::ensemble_multi_gpu).
 * out: ndevices handles, out[i] is rank i on devices[i]. */
int sxmc_comm_init_all(const int* devices, int ndevices, sxmc_comm_t* out);
/* One process per GPU: rank 0 makes the id (128 bytes), passes it to the others by any means (a file, MPI,
 * torch.distributed), and every rank joins with the current device. */
int sxmc_comm_unique_id(char* id, size_t id_bytes);
int sxmc_comm_init_rank(const char* id, size_t id_bytes, int nranks, int rank, sxmc_comm_t* out);
int sxmc_comm_rank(sxmc_comm_t c, int* rank, int* nranks);
/* Rank, rank count and device AS THE COMMUNICATOR REPORTS THEM (ncclCommUserRank / ncclCommCount / ncclCommCuDevice),
 * not what the caller passed in: what a bench line records to show how many ranks RCCL really joined.  Any of the
 * three pointers may be null. */
int sxmc_comm_query(sxmc_comm_t c, int* rank, int* nranks, int* device);
/* *failed = 1 when the communicator has recorded an asynchronous error (a peer died, a link failed). */
int sxmc_comm_async_error(sxmc_comm_t c, int* failed);
/* Fail-fast tear-down: ncclCommAbort -- ends a collective that is still waiting for a peer that will never arrive
 * (instead of sxmc_comm_destroy, which would wait for it) and frees the handle. */
int sxmc_comm_abort(sxmc_comm_t c);
/* d_recv[r * count .. (r + 1) * count) = rank r's d_send[0 .. count) on every rank; device buffers; asynchronous
 * on `s` of the communicator's device. */
int sxmc_comm_allgather_f32(sxmc_comm_t c, const float* d_send, float* d_recv, size_t count, sxmc_stream_t s);
int sxmc_comm_destroy(sxmc_comm_t c);
const char* sxmc_comm_last_error(void);

/* ---------------------------------------------------------------------------------------------------------------
 * MEASUREMENT BUILD ONLY.  libsxmc_hip.so does not export what follows (tests/test_abi.py checks); it is compiled into
 * libsxmc_hip_measure.so (make -C sxmc_amd/csrc VARIANT=_measure EXTRA=-DSXMC_MEASURE=1), the library behind the
 * roofline decompositions in profiles/ and behind the tests that need a look inside (known answers of the generator
 * and of the rounded powers, the margin of the codes' error bound). */
#ifdef SXMC_MEASURE
/* Hooks of the histogram-fill kernels.  RESULTS ARE WRONG when mode != 0.
 * bit 0 = stream the columns, skip arithmetic and histogram; bit 1 = arithmetic and histogram run but every reload
 * hits one cached address; bit 2 = skip only the histogram update; bit 3 = stream the float columns regardless of
 * codes (fused step: the fill's part of the launch alone); bit 4 = drop what the queues of ambiguous rows hold;
 * bit 5 = no LDS additions; bits 8-15 = 1 + 64 s: the roundings' share of the codes' error bound scaled by s;
 * bits 16-23 = 1 + 64 t: the whole threshold scaled by t (fill_kernels.inc.h, "THE BOUND"). */
int sxmc_group_set_debug_mode(sxmc_group_t g, int mode);
/* d_out[k] = d_x[k]^i as the polynomial systematics form it (p = sum_i c_i * pow(x, i), pdfz.cpp:310-314): the power
 * rounded ONCE, like libm's pow for small integer exponents -- not the i - 1 roundings of repeated multiplication.
 * Exact for i <= 1, the plain product for i = 2. */
int sxmc_debug_pow_int(const double* d_x, int n, int i, double* d_out);
/* Raw Philox4x32-10 output of d_state[0], 4 words per draw; advances the state. */
int sxmc_debug_philox_dump(sxmc_rng_state* d_state, unsigned* d_out, int ndraws);
/* THE GATED STEP, an experiment ("one more look"): the group's next sxmc_group_step_async puts its
 * fill on `fill_stream` -- ordered after the previous fill, not after the previous step end -- as step `node` (0 .. 15)
 * of a recording; the fill does what does not depend on the proposal beside the step end and waits for it inside.
 * fill_stream null: back to one stream.  sxmc_measure_stream_fork: `to` waits for what `from` has queued (inside a
 * recording: brings `to` into it). */
int sxmc_measure_set_gated_step(sxmc_group_t g, sxmc_stream_t fill_stream, int node);
int sxmc_measure_stream_fork(sxmc_stream_t from, sxmc_stream_t to);
#endif

#ifdef __cplusplus
}
#endif
#endif /* SXMC_HIP_H */
