"""The contracts of the projections (include/sxmc_hip.h: sxmc_hist_project, sxmc_kde_project) and of fit_spectra
(sxmc_amd/ensemble.py, sxmc_amd/include/sxmc/ensemble.h) restated in numpy f64: the reference their tests compare with.
No device needed.

A kernel-density marginal is analytic.  The kernel of an in-domain sample is a product of Gaussians truncated to the
domain; integrated over every observable but one, the others give their own truncation mass and cancel against the
weight, which leaves, with u = (s - lower) / h, T = (upper - lower) / h and t_j = (e_j - lower) / h for the bin edges,
  share_j = 1/n sum_i [Phi(t_j+1 - u_i) - Phi(t_j - u_i)] / [Phi(T - u_i) - Phi(-u_i)].
ref_kde_marginal takes u from the rows as the prepass leaves them (the scaled coordinate rounded to f32: what the device
reads), ref_kde_marginal_exact from the unrounded f64 samples; they differ by what that rounding can move."""

import numpy as np

from oracle import oracle
from tests.kde_reference import CSCALE, moved_in_domain, phi, ref_bandwidths

U24 = 2.0 ** -24


def bin_edges_t(lower, upper, h, nbins):
    """t_j = (e_j - lower) / h for e_j = lower + j ((upper - lower) / nbins); the two ends are lower and upper
    themselves, so that the shares telescope to the truncation mass."""
    j = np.arange(nbins + 1, dtype=np.float64)
    t = ((lower + j * ((upper - lower) / nbins)) - lower) / h
    t[0] = 0.0
    t[-1] = (upper - lower) / h
    return t


def marginal_from_u(u, lower, upper, h, nbins):
    """(shares [nbins], masses [n]) of in-domain samples at u = (s - lower) / h."""
    u = np.asarray(u, np.float64)
    if u.size == 0:
        return np.zeros(nbins), np.zeros(0)
    t = bin_edges_t(lower, upper, h, nbins)
    mass = phi(t[-1] - u) - phi(-u)
    cdf = phi(t[:, None] - u[None, :])                       # [nbins + 1, n]
    share = ((cdf[1:] - cdf[:-1]) / mass[None, :]).sum(axis=1) / u.size
    return share, mass


def kde_u(samples, nfields, nobs, lower, upper, scale, systs, params, obs, rounded=True, bandwidth_factor=1.0):
    """u of every in-domain moved sample along `obs`, and the bandwidth there.  rounded: through the prepass's f32
    scaled coordinate c = (s - lower) sqrt(log2(e) / 2) / h, as the device reads it back (u = c / sqrt(log2(e) / 2))."""
    lower, upper = np.asarray(lower, np.float64), np.asarray(upper, np.float64)
    h = ref_bandwidths(samples, nfields, nobs, lower, upper, scale)[obs] * bandwidth_factor
    s = moved_in_domain(samples, nfields, nobs, lower, upper, systs, params)[:, obs]
    if not rounded:
        return (s - lower[obs]) / h, h
    c = ((s - lower[obs]) * (CSCALE / h)).astype(np.float32)
    return c.astype(np.float64) / CSCALE, h


def ref_kde_marginal(samples, nfields, nobs, lower, upper, scale, systs, params, obs, nbins, bandwidth_factor=1.0):
    """The contract of sxmc_kde_project from the rows rounded to f32 exactly as the prepass leaves them.
    bandwidth_factor != 1: a reference with a planted error (the projection's bandwidth off by that factor, on rows
    the true bandwidth scaled)."""
    u, h = kde_u(samples, nfields, nobs, lower, upper, scale, systs, params, obs, rounded=True)
    return marginal_from_u(u / bandwidth_factor, lower[obs], upper[obs], h * bandwidth_factor, nbins)[0]


def ref_kde_marginal_exact(samples, nfields, nobs, lower, upper, scale, systs, params, obs, nbins):
    """(shares, u_max, mass_min) from the unrounded f64 samples."""
    u, h = kde_u(samples, nfields, nobs, lower, upper, scale, systs, params, obs, rounded=False)
    share, mass = marginal_from_u(u, lower[obs], upper[obs], h, nbins)
    return share, float(np.abs(u).max(initial=0.0)), float(mass.min(initial=1.0))


def ref_data_hist(x, lower, upper, bins):
    """TH1::Fill, one value at a time: lower <= x < upper (f64 on the float) goes to bin
    int(bins * (x - lower) / (upper - lower)); under- and overflow are not counted, nor is a quotient that rounds up to
    `bins` (TAxis::FindBin sends it to the overflow bin)."""
    out = [0] * bins
    for v in np.asarray(x, np.float32):
        d = float(v)
        if not (d >= lower and d < upper):
            continue
        j = int(bins * (d - lower) / (upper - lower))
        if 0 <= j < bins:
            out[j] += 1
    return np.array(out, np.int64)


def ref_fit_spectra(nobs, lower, upper, nbins, names, signals, systs, params, nsources, events):
    """fit_spectra from the CPU oracle's bins (histogram signals) and ref_kde_marginal (kernel signals).
    signals: dicts (name, samples, nfields, nexpected, n_mc, source_id, dataset, pdf, bandwidth_scale); params: the P
    values, rounded to float as plot_fit holds them.  Returns the list of dicts ensemble.fit_spectra returns, every
    signal with a `kind` besides."""
    pf = np.asarray(params, np.float32).astype(np.float64)
    geom = oracle.HistGeometry(lower, upper, nbins)
    per = []
    for s in signals:
        if s["pdf"] == "kernel":
            moved = moved_in_domain(s["samples"], s["nfields"], nobs, lower, upper, systs, pf[nsources:])
            norm = len(moved)
            marg = [ref_kde_marginal(s["samples"], s["nfields"], nobs, lower, upper, s["bandwidth_scale"], systs,
                                     pf[nsources:], k, nbins[k]) for k in range(nobs)]
        else:
            bins, norm = oracle.bin_samples(geom, s["samples"], s["nfields"], systs, pf[nsources:])
            cube = bins.reshape(nbins).astype(np.int64)
            total = int(cube.sum())
            marg = [cube.sum(axis=tuple(a for a in range(nobs) if a != k)) for k in range(nobs)]
        eff = norm / float(s["n_mc"])
        nexp = s["nexpected"] * eff * float(pf[s["source_id"]])
        if s["pdf"] == "kernel":
            spectra = [m * nexp for m in marg]
        else:
            spectra = [m.astype(np.float64) * (nexp / total) if total else np.zeros(len(m)) for m in marg]
        per.append(dict(name=s["name"], kind=s["pdf"], nexp=nexp, spectra=spectra, dataset=s["dataset"]))
    events = np.asarray(events, np.float32).reshape(-1, nobs + 1)
    out = []
    for ds in sorted({s["dataset"] for s in signals}):
        mine = [p for p in per if p["dataset"] == ds]
        rows = events[events[:, nobs].astype(np.int64) == ds]
        for k in range(nobs):
            fit = np.zeros(nbins[k])
            for p in mine:
                fit = fit + p["spectra"][k]
            out.append(dict(observable=names[k], dataset=ds, lower=float(lower[k]), upper=float(upper[k]),
                            bins=int(nbins[k]),
                            signals=[dict(name=p["name"], kind=p["kind"], nexp=p["nexp"], spectrum=p["spectra"][k])
                                     for p in mine],
                            fit=fit, data=ref_data_hist(rows[:, k], float(lower[k]), float(upper[k]), int(nbins[k]))))
    return out


def midpoint_marginal(pdf_on_grid, width):
    """Midpoint rule: the mean of the pdf values on a bin's sub-grid times the bin's width (per bin: [nbins, m])."""
    return np.asarray(pdf_on_grid, np.float64).mean(axis=1) * width
