"""GPU tests of fit_spectra, the ROOT-free plot_fit (plots.cpp:150-302): the C++ layer (sxmc::fit_spectra +
write_fit_spectra, through tests/cpp/test_fit_spectra.cpp, compiled here) and the Python layer (ensemble.fit_spectra +
io.write_fit_spectra) run on the same inputs, their files compared value for value, and both with
tests/project_reference.ref_fit_spectra (the CPU oracle's bins, the analytic kernel-density marginals): histogram
signals to 1e-14 relative (f64 rounding of two products), kernel-density signals to the projection's tolerances
(tests/test_gpu_project.py) times nexp.  Two fits: 1-D with one histogram and one kernel-density signal, 2-D with
four histogram signals in two data sets, both at parameters off their means.  And run_config's spectra_dir."""
import json
import os
import subprocess

import numpy as np
import pytest

from sxmc_amd import ensemble, io, workloads
from tests.project_reference import U24, ref_fit_spectra, ref_kde_marginal_exact
from tests.test_kde_cpu import ROOT, cpp_flags

pytestmark = pytest.mark.gpu

TYPES = {"shift": 0, "scale": 1, "resolution_scale": 2, "ctscale": 3}


def fit_1d(rng):
    """The tables of tests/cpp/test_kde_walk.cpp's walk, smaller: a falling spectrum (histogram) and a narrow line
    (kernel density) in energy, with its truth field."""
    t = 10.0 * rng.random(20000) * rng.random(20000)
    flat = np.stack([t + 0.2 * rng.normal(size=t.size), t], axis=1).astype(np.float32)
    t = 6.0 + 0.4 * rng.normal(size=1500)
    line = np.stack([t + 0.2 * rng.normal(size=t.size), t], axis=1).astype(np.float32)
    signals = [dict(name="spectrum", samples=flat, nfields=2, nexpected=600.0, n_mc=25000, source_id=0, dataset=0,
                    pdf="hist", bandwidth_scale=None),
               dict(name="line", samples=line, nfields=2, nexpected=300.0, n_mc=1500, source_id=1, dataset=0,
                    pdf="kernel", bandwidth_scale=[0.9])]
    systs = [dict(name="e_scale", type="scale", obs=0, true_obs=0, pars=[0]),
             dict(name="e_res", type="resolution_scale", obs=0, true_obs=1, pars=[1])]
    events = np.concatenate([flat[rng.integers(0, len(flat), 500), :1], line[rng.integers(0, len(line), 250), :1]])
    events = events[(events[:, 0] >= 0.0) & (events[:, 0] < 10.0)]
    events = np.concatenate([events, np.float32([[0.0], [10.0], [-0.5], [11.0]])])   # planted: only lower counts
    events = np.concatenate([events, np.zeros((len(events), 1), np.float32)], axis=1)
    return dict(nobs=1, F=2, names=["energy"], lower=[0.0], upper=[10.0], nbins=[25], signals=signals, systs=systs,
                nsources=2, params=[1.1, 0.85, 0.013, -0.06], events=events.astype(np.float32))


def fit_2d(rng):
    """Two observables and a truth field, four histogram signals over two sources and two data sets."""
    def tab(n, mx, my):
        t = rng.normal(mx, 0.7, n)
        return np.stack([t + 0.15 * rng.normal(size=n), rng.normal(my, 0.4, n), t], axis=1).astype(np.float32)
    tabs = [tab(6000, 1.5, -0.2), tab(4000, 2.6, 0.3), tab(5000, 1.4, -0.1), tab(3000, 2.5, 0.2)]
    signals = [dict(name="s%d" % i, samples=tabs[i], nfields=3, nexpected=[200.0, 120.0, 90.0, 310.0][i],
                    n_mc=[6000, 4100, 5000, 3000][i], source_id=i % 2, dataset=i // 2, pdf="hist", bandwidth_scale=None)
               for i in range(4)]
    systs = [dict(name="x_shift", type="shift", obs=0, true_obs=0, pars=[0]),
             dict(name="y_scale", type="scale", obs=1, true_obs=0, pars=[1]),
             dict(name="x_res", type="resolution_scale", obs=0, true_obs=2, pars=[2])]
    ev = np.concatenate([np.concatenate([tabs[i][rng.integers(0, len(tabs[i]), 150), :2],
                                         np.full((150, 1), i // 2, np.float32)], axis=1) for i in range(4)])
    return dict(nobs=2, F=3, names=["x", "y"], lower=[0.0, -1.0], upper=[4.0, 1.0], nbins=[6, 5], signals=signals,
                systs=systs, nsources=2, params=[0.9, 1.25, 0.07, -0.03, 0.11], events=ev.astype(np.float32))


def write_case(fit, indir):
    lines = ["fields %d" % fit["F"], "observables %d" % fit["nobs"]]
    for k in range(fit["nobs"]):
        lines.append("%s %d %d %.9g %.9g" % (fit["names"][k], k, fit["nbins"][k], fit["lower"][k], fit["upper"][k]))
    lines.append("systematics %d" % len(fit["systs"]))
    for s in fit["systs"]:
        lines.append("%s %d %d %d %d %s" % (s["name"], TYPES[s["type"]], s["obs"], s["true_obs"], len(s["pars"]),
                                            " ".join(str(p) for p in s["pars"])))
    lines.append("sources %d" % fit["nsources"])
    lines += ["source%d" % i for i in range(fit["nsources"])]
    lines.append("signals %d" % len(fit["signals"]))
    for s in fit["signals"]:
        s["samples"].tofile(os.path.join(indir, s["name"] + ".f32"))
        lines.append("%s %d %d %.17g %d %s %s %d %s" % (
            s["name"], s["dataset"], s["source_id"], s["nexpected"], s["n_mc"], s["pdf"], s["name"] + ".f32",
            len(s["samples"]), " ".join("%.17g" % b for b in (s["bandwidth_scale"] or []))))
    lines.append("params %d %s" % (len(fit["params"]), " ".join("%.17g" % p for p in fit["params"])))
    fit["events"].tofile(os.path.join(indir, "data.f32"))
    lines.append("data data.f32 %d" % len(fit["events"]))
    with open(os.path.join(indir, "case.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def workload_of(fit):
    sigs = []
    for s in fit["signals"]:
        g = workloads.Signal(s["samples"], s["nfields"], s["nexpected"], s["source_id"], dataset=s["dataset"],
                             pdf=s["pdf"], bandwidth_scale=s["bandwidth_scale"])
        g.n_mc_total = s["n_mc"]
        g.name = s["name"]
        sigs.append(g)
    nsyst = sum(len(s["pars"]) for s in fit["systs"])
    w = workloads.Workload("fit", fit["nobs"], fit["lower"], fit["upper"], fit["nbins"], sigs, fit["systs"],
                           [0.1] * nsyst, fit["events"], "fit spectra test")
    w.observable_names = fit["names"]
    return w


def read_spectra(directory, fit):
    out = []
    for ds in sorted({s["dataset"] for s in fit["signals"]}):
        for name in fit["names"]:
            with open(os.path.join(directory, "%s_%d.json" % (name, ds))) as f:
                out.append(json.load(f))
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx, ld = cpp_flags()
    path = str(tmp_path_factory.mktemp("fit_spectra_exe") / "test_fit_spectra")
    src = os.path.join(ROOT, "tests", "cpp", "test_fit_spectra.cpp")
    subprocess.run(["g++"] + cxx + ["-o", path, src] + ld, check=True, capture_output=True, text=True, timeout=600)
    return path


@pytest.mark.parametrize("make", [fit_1d, fit_2d], ids=["1d_hist_and_kernel", "2d_two_datasets"])
def test_cpp_and_python_spectra_agree_with_each_other_and_the_reference(make, exe, tmp_path):
    fit = make(np.random.default_rng(11))
    indir, cdir, pdir = (str(tmp_path / n) for n in ("in", "cpp", "py"))
    os.makedirs(indir)
    write_case(fit, indir)
    r = subprocess.run([exe, indir, cdir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "spectra written" in r.stdout, r.stdout + r.stderr
    w = workload_of(fit)
    evs = ensemble.make_evaluators(w)
    spectra = ensemble.fit_spectra(w, evs, fit["params"], fit["events"])
    paths = io.write_fit_spectra(pdir, spectra)
    npairs = len({s["dataset"] for s in fit["signals"]}) * fit["nobs"]
    assert len(paths) == npairs and sorted(os.listdir(pdir)) == sorted(os.listdir(cdir))
    got_c, got_p = read_spectra(cdir, fit), read_spectra(pdir, fit)
    assert got_c == got_p                                                  # value for value
    want = ref_fit_spectra(fit["nobs"], fit["lower"], fit["upper"], fit["nbins"], fit["names"], fit["signals"],
                           fit["systs"], fit["params"], fit["nsources"], fit["events"])
    pf = np.asarray(fit["params"], np.float32).astype(np.float64)
    assert len(want) == npairs
    for g, wnt in zip(got_p, want):
        k = fit["names"].index(g["observable"])
        assert (g["observable"], g["dataset"], g["bins"]) == (wnt["observable"], wnt["dataset"], wnt["bins"])
        assert g["lower"] == wnt["lower"] and g["upper"] == wnt["upper"]
        assert [s["name"] for s in g["signals"]] == [s["name"] for s in wnt["signals"]]
        assert len(g["signals"]) == sum(1 for s in fit["signals"] if s["dataset"] == g["dataset"]) > 0
        total = np.zeros(g["bins"])
        for gs, ws in zip(g["signals"], wnt["signals"]):
            sp, ref = np.asarray(gs["spectrum"]), ws["spectrum"]
            assert sp.shape == (g["bins"],)
            assert abs(gs["nexp"] - ws["nexp"]) <= 1e-14 * abs(ws["nexp"]) and ws["nexp"] > 0
            if ws["kind"] == "hist":
                tol = 1e-14 * np.abs(ref)
            else:
                sig = next(s for s in fit["signals"] if s["name"] == gs["name"])
                args = (sig["samples"], sig["nfields"], fit["nobs"], np.asarray(fit["lower"]), np.asarray(fit["upper"]),
                        sig["bandwidth_scale"], fit["systs"], pf[fit["nsources"]:], k, g["bins"])
                exact, u_max, mass_min = ref_kde_marginal_exact(*args)
                tol = 1e-11 * ws["nexp"]
                assert np.all(np.abs(sp - exact * ws["nexp"]) <= 0.4 * u_max * U24 / mass_min * ws["nexp"])
            print("%s %s: worst |d| %.3g (nexp %.6g)" % (g["observable"], gs["name"], np.abs(sp - ref).max(), gs["nexp"]))
            assert np.all(np.abs(sp - ref) <= tol)
            assert abs(sp.sum() - gs["nexp"]) <= 1e-12 * gs["nexp"]        # the spectrum holds nexp events
            total = total + sp
        assert np.array_equal(np.asarray(g["fit"]), total)                 # the signals, added in their order
        assert np.array_equal(np.asarray(g["data"]), wnt["data"])
        ev = fit["events"]
        mine = ev[ev[:, fit["nobs"]] == g["dataset"]][:, k].astype(np.float64)
        inside = int(((mine >= g["lower"]) & (mine < g["upper"])).sum())
        assert sum(g["data"]) == inside and 0 < inside
    if make is fit_1d:
        assert sum(got_p[0]["data"]) == len(fit["events"]) - 3             # planted: upper and two outside; lower counts
    for e in evs:
        e.close()


def test_run_config_writes_spectra_only_when_asked(tmp_path):
    from tests.test_io_cpu import EXAMPLE
    rng = np.random.default_rng(0)
    work = tmp_path / "work"
    work.mkdir()
    for name, n in (("a.npz", 20000), ("b.npz", 30000)):
        mc = rng.uniform(4, 16, n).astype(np.float32)
        io.write_table(work / name, np.stack([mc + rng.normal(0, 0.5, n).astype(np.float32),
                                              rng.uniform(0, 12, n).astype(np.float32), mc], axis=1),
                       ["energy", "radius", "mc_energy"])
    (work / "fit.json").write_text(EXAMPLE)
    before = sorted(os.listdir(work))
    cwd_before = sorted(os.listdir("."))
    iv0, _, _ = io.run_config(str(work / "fit.json"), nexperiments=2, nsteps=200)
    assert sorted(os.listdir(work)) == before and sorted(os.listdir(".")) == cwd_before      # nothing new
    out = tmp_path / "spectra"
    iv, _, names = io.run_config(str(work / "fit.json"), nexperiments=2, nsteps=200, spectra_dir=str(out))
    assert np.array_equal(iv, iv0)                                          # the fits themselves are unchanged
    assert sorted(os.listdir(out)) == ["0", "1"] and sorted(os.listdir(work)) == before
    for i in range(2):
        assert os.listdir(out / str(i)) == ["energy_0.json"]
        with open(out / str(i) / "energy_0.json") as f:
            g = json.load(f)
        assert g["observable"] == "energy" and g["bins"] == 10 and (g["lower"], g["upper"]) == (5.0, 15.0)
        assert [s["name"] for s in g["signals"]] == ["sig_a", "sig_b"]
        for s, p in zip(g["signals"], (0, 1)):
            assert s["nexp"] > 0 and abs(sum(s["spectrum"]) - s["nexp"]) <= 1e-12 * s["nexp"]
        total = np.asarray(g["signals"][0]["spectrum"]) + np.asarray(g["signals"][1]["spectrum"])
        assert np.array_equal(np.asarray(g["fit"]), total) and sum(g["data"]) > 0
