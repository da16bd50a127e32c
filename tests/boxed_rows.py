"""Tables BUILT to sit where the boxed fill's two arguments are tested (shared by tests/test_boxed_model_cpu.py, the GPU
tests of tests/test_gpu_boxed_threshold.py and tests/boxed_margin_worker.py; the model is tests/boxed_reference.py).

THRESHOLD ROWS (the streamed observable's bound).  A row is wrongly binned from its code only if a transformed bin edge
falls a hair inside a boundary of the row's code cell -- the cell's centre is then a whole half step from the edge, the
rows between boundary and edge lie on the other side of it.  One scalar parameter fixes every edge's position in its
cell, so the rows are every float32 (sub-sampled evenly where there are too many) in the seven code cells around each
edge's pre-image, and the PARAMETER is solved, against the reference's arithmetic in double, so that one chosen edge
sits d float spacings inside the lower or the upper boundary of a cell.  The boxed observable is one mid-bin constant
per bucket and equals its truth field: every box is a point, no granule straddles, the codes decide the rows.

CORNER TABLES (the boxed observable's interval rule).  Clusters of rows with TWO values of x and TWO of t in all four
combinations: whatever granule the layout cuts from a cluster, the corners of its box are rows that exist.  Per cluster
one parameter is solved, by bisection to neighbouring doubles against the reference's arithmetic, so that a named
corner's image crosses a bin edge (or a domain end) exactly there; evaluated there and a few ulps to either side."""
import numpy as np

from tests.boxed_reference import windows

NFIELDS, TRUTH, BOXED = 5, 3, 0
C3_GEOM = ([0.0, 0.0, -1.0], [10.0, 6.0, 1.0], [20, 20, 20])
SPACINGS = (0.5, 1.0, 2.0, 4.0, 16.0, 64.0)

# streamed: the observable binned from codes; unwritten: the one nothing writes (the buckets); free: the parameter solved
THRESHOLD_PROGRAMS = {
    "c3-shift": dict(geom=C3_GEOM, streamed=1, unwritten=2, window=(-0.5, 6.5), free=0, base=[0.0, 0.004, 0.03],
                     systs=[dict(type="shift", obs=1, pars=[0]), dict(type="scale", obs=0, pars=[1]),
                            dict(type="resolution_scale", obs=0, true_obs=3, pars=[2])]),
    "scale-positive": dict(geom=C3_GEOM, streamed=1, unwritten=2, window=(-0.5, 6.5), free=0, base=[0.05, 0.004, 0.03],
                           systs=[dict(type="scale", obs=1, pars=[0]), dict(type="scale", obs=0, pars=[1]),
                                  dict(type="resolution_scale", obs=0, true_obs=3, pars=[2])]),
    # 1 + p < 0: alpha negative, the sides of every cell flip; the domain's pre-image is (-3, 0]
    "scale-negative": dict(geom=C3_GEOM, streamed=1, unwritten=2, window=(-3.5, 0.5), free=0, base=[-3.0, 0.004, 0.03],
                           systs=[dict(type="scale", obs=1, pars=[0]), dict(type="scale", obs=0, pars=[1]),
                                  dict(type="resolution_scale", obs=0, true_obs=3, pars=[2])]),
    "ctscale-streamed": dict(geom=(C3_GEOM[0], C3_GEOM[1], [12, 10, 8]), streamed=2, unwritten=1, window=(-1.25, 1.25),
                             free=0, base=[0.03, 0.05, -0.02],
                             systs=[dict(type="ctscale", obs=2, pars=[0]),
                                    dict(type="resolution_scale", obs=0, true_obs=3, pars=[1]),
                                    dict(type="shift", obs=0, pars=[2])]),
    "shift-after-scale": dict(geom=C3_GEOM, streamed=1, unwritten=2, window=(-0.5, 6.5), free=0,
                              base=[0.07, 0.013, 0.004, 0.03],
                              systs=[dict(type="scale", obs=1, pars=[0]), dict(type="shift", obs=1, pars=[1]),
                                     dict(type="scale", obs=0, pars=[2]),
                                     dict(type="resolution_scale", obs=0, true_obs=3, pars=[3])]),
    "two-resolutions": dict(geom=(C3_GEOM[0], C3_GEOM[1], [20, 6, 5]), streamed=1, unwritten=2, window=(-0.5, 6.5),
                            free=1, base=[0.04, 0.0, -0.03],
                            systs=[dict(type="resolution_scale", obs=0, true_obs=3, pars=[0]),
                                   dict(type="shift", obs=1, pars=[1]),
                                   dict(type="resolution_scale", obs=0, true_obs=3, pars=[2])]),
}

_C3 = THRESHOLD_PROGRAMS["c3-shift"]["systs"]
# free: the parameters a cluster's solve may move (those of the boxed observable); base: where 1 + p and the
# resolution coefficient have the signs the table is about
CORNER_PROGRAMS = {
    "scale+res+": dict(geom=C3_GEOM, streamed=1, unwritten=2, systs=_C3, free=[1, 2], base=[0.01, 0.04, 0.15]),
    "scale+res-": dict(geom=C3_GEOM, streamed=1, unwritten=2, systs=_C3, free=[1, 2], base=[0.01, 0.04, -0.15]),
    "scale-res+": dict(geom=C3_GEOM, streamed=1, unwritten=2, systs=_C3, free=[1, 2], base=[0.01, -2.04, 0.15]),
    "scale-res-": dict(geom=C3_GEOM, streamed=1, unwritten=2, systs=_C3, free=[1, 2], base=[0.01, -2.04, -0.15]),
    "two-resolutions": dict(geom=(C3_GEOM[0], C3_GEOM[1], [20, 6, 5]), streamed=1, unwritten=2,
                            systs=THRESHOLD_PROGRAMS["two-resolutions"]["systs"], free=[0, 2], base=[0.12, 0.01, -0.08]),
}

# THE TABLES MUST NOT TEST NOTHING.  Floors, each a few points below what these builders give with the seeds fixed
# below (the value beside it; tests/test_boxed_model_cpu.py prints them): the share of built threshold rows the unscaled
# model bins from codes, over every solved parameter vector, and the share of a corner table's in-domain rows that sit
# in granules the interval rule decides at the table's base parameters (boxed_reference.decided_row_share).  tests/boxed_margin_worker.py holds the device to the same floors.
TRUSTED_FLOOR = {"c3-shift": 0.79,            # 0.8277
                 "scale-positive": 0.81,      # 0.8467
                 "scale-negative": 0.80,      # 0.8334
                 "ctscale-streamed": 0.80,    # 0.8425
                 "shift-after-scale": 0.82}   # 0.8541
DECIDED_FLOOR = {"scale+res+": 0.70,          # 0.754
                 "scale+res-": 0.72,          # 0.769
                 "scale-res+": 0.70,          # 0.756
                 "scale-res-": 0.68,          # 0.727
                 "two-resolutions": 0.37}     # 0.420


# ------------------------------------------------------------------------------------ the reference's arithmetic
def image(systs, obs, x, t, params):
    """Observable `obs` of a row after the program, as the reference forms it: IEEE double, operation by operation
    (the same statements as reference_bins of tests/test_codes_model_cpu.py, for one observable)."""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        for s in systs:
            if s["obs"] != obs:
                continue
            p = 0.0 + float(params[s["pars"][0]]) * 1.0
            if s["type"] == "shift":
                x = x + p
            elif s["type"] == "scale":
                x = x * (1 + p)
            elif s["type"] == "ctscale":
                x = 1 + (x - 1) * (1 + p)
            else:
                x = x + (p * (x - np.asarray(t, np.float64)))
    return x


def crossing(systs, obs, x, t, params, lo, hi, nb, k):
    """< 0 below edge k, >= 0 at or above it, the way the reference decides: the domain tests on x at the two ends, the
    product (x - lo) * scale that is truncated to the index in between."""
    v = image(systs, obs, x, t, params)
    if k == 0:
        return v - lo
    if k == nb:
        return v - hi
    return (v - lo) * (nb / (hi - lo)) - k


def bisect(fn, a, b, exact=False, iters=200):
    """A root of the monotone fn in [a, b] (None: no sign change); exact: down to neighbouring doubles (lower, upper)."""
    fa, fb = fn(a), fn(b)
    if not (np.isfinite(fa) and np.isfinite(fb)) or (fa < 0) == (fb < 0):
        return None
    for _ in range(iters):
        m = 0.5 * (a + b)
        if m == a or m == b:
            break
        if (fn(m) < 0) == (fa < 0):
            a = m
        else:
            b = m
    return (a, b) if exact else 0.5 * (a + b)


# ---------------------------------------------------------------------------------------- float32, enumerated
def f32_order(x):
    """float32 -> integers in the order of the values (-0.0 just below +0.0)."""
    i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i >= 0, i, -(i & 0x7FFFFFFF) - 1)


def f32_from_order(o):
    o = np.asarray(o, np.int64)
    return np.where(o >= 0, o, (-(o + 1)) | 0x80000000).astype(np.uint32).view(np.float32)


def first_f32_at_or_above(a):
    x = np.float32(a)
    return x if float(x) >= a else np.nextafter(x, np.float32(np.inf))


def last_f32_below(b):
    x = np.float32(b)
    return x if float(x) < b else np.nextafter(x, np.float32(-np.inf))


def floats_between(a, b, cap):
    """Every float32 in [a, b) through its bit pattern; more than `cap`: an eighth of them evenly spaced in the patterns
    (near 0.0 that is mostly tiny values and denormals, all in the one cell that holds 0.0), the rest evenly in value."""
    oa, ob = int(f32_order(first_f32_at_or_above(a))), int(f32_order(last_f32_below(b)))
    if ob < oa:
        return np.zeros(0, np.float32)
    if ob - oa + 1 <= cap:
        return f32_from_order(np.arange(oa, ob + 1))
    by_pattern = np.rint(np.linspace(oa, ob, cap // 8)).astype(np.int64)
    by_value = np.linspace(a, b, cap - cap // 8, endpoint=False).astype(np.float32)
    by_value = by_value[(by_value.astype(np.float64) >= a) & (by_value.astype(np.float64) < b)]
    return f32_from_order(np.unique(np.concatenate([by_pattern, f32_order(by_value)])))


# --------------------------------------------------------------------------------------------- threshold rows
def boxed_constants(lo, hi, nb):
    """Four mid-bin values of the boxed observable."""
    w = (hi - lo) / nb
    return [lo + (int(nb * f) + 0.5) * w for f in (0.15, 0.4, 0.6, 0.85)]


def threshold_table(name, cap=3000, nbackground=20000, seed=20260):
    """The table of THRESHOLD_PROGRAMS[name] and the solved parameter vectors.  Returns a dict: tab (float32, NFIELDS
    columns), built (mask of the built rows), base / step (the streamed field's window), params (list of vectors),
    solved (per vector: edge, cell, side, spacings), spec."""
    spec = THRESHOLD_PROGRAMS[name]
    lo, hi, nb = spec["geom"]
    s, w, systs = spec["streamed"], spec["unwritten"], spec["systs"]
    rng = np.random.default_rng(seed)
    wlo, whi = spec["window"]
    base, step = wlo, (whi - wlo) / 65532.0
    base_params = list(spec["base"])
    sc = nb[s] / (hi[s] - lo[s])
    r_parts, k_parts, cells = [], [], {}
    for k in range(nb[s] + 1):
        pre = bisect(lambda r: crossing(systs, s, r, 0.0, base_params, lo[s], hi[s], nb[s], k), wlo, whi)
        if pre is None:
            continue
        q = int(np.floor((pre - base) / step))
        cells[k] = q
        a, b = max(base + (q - 3) * step, wlo), min(base + (q + 4) * step, whi)
        r = [floats_between(a, b, cap)]
        for j in range(q - 3, q + 5):                              # the floats either side of every cell boundary
            edge = base + j * step
            if a < edge < b:
                r.append(np.array([last_f32_below(edge), first_f32_at_or_above(edge)], np.float32))
        r = np.unique(np.concatenate(r).view(np.uint32)).view(np.float32)
        r_parts.append(r)
        k_parts.append(np.full(r.size, k))
    r_built, k_built = np.concatenate(r_parts), np.concatenate(k_parts)

    params, solved = [], []
    for k, q in cells.items():
        for cell in (q - 1, q, q + 1):
            for side in (0, 1):                                    # inside the lower / the upper boundary
                edge_r = base + (cell + side) * step
                f = first_f32_at_or_above(edge_r) if side == 0 else last_f32_below(edge_r)
                for d in SPACINGS:
                    o = int(f32_order(f)) + (1 if side == 0 else -1) * int(d)
                    t0, t1 = f32_from_order(np.array([o, o + (1 if side == 0 else -1)])).astype(np.float64)
                    target = t0 + (d - int(d)) * (t1 - t0)

                    def miss(p):
                        v = list(base_params)
                        v[spec["free"]] = p
                        return crossing(systs, s, target, 0.0, v, lo[s], hi[s], nb[s], k)
                    p0, p = base_params[spec["free"]], None
                    for delta in (1e-3, 1e-2, 1e-1):
                        p = bisect(miss, p0 - delta, p0 + delta)
                        if p is not None:
                            break
                    if p is None:
                        continue     # (an edge the parameter does not move: 0 under a scale, 1 under a cos-theta scale)
                    v = list(base_params)
                    v[spec["free"]] = float(p)
                    params.append(v)
                    solved.append(dict(edge=k, cell=cell, side=side, spacings=d))

    def other_columns(tab, bucket):
        tab[:, w] = lo[w] + (bucket + 0.5) * (hi[w] - lo[w]) / nb[w]
        xs = np.array(boxed_constants(lo[BOXED], hi[BOXED], nb[BOXED]))
        tab[:, BOXED] = xs[bucket % 4]
        tab[:, TRUTH] = tab[:, BOXED]

    rows = np.zeros((r_built.size, NFIELDS), np.float32)
    rows[:, s] = r_built
    other_columns(rows, k_built % nb[w])
    # ordinary rows between them: about one row in six of a band is ambiguous at every solved vector (the cells within a
    # half step of the edge), and a wave's queue holds a few dozen rows before the whole granule goes to the float path
    bg = np.zeros((nbackground, NFIELDS), np.float32)
    bg[:, s] = rng.uniform(wlo, whi, nbackground)
    bg[0, s], bg[1, s] = wlo, whi                                  # the rows that pin the window
    other_columns(bg, rng.integers(0, nb[w], nbackground))
    tab = np.concatenate([bg, rows])
    order = rng.permutation(tab.shape[0])
    tab = np.ascontiguousarray(tab[order])
    built = order >= nbackground
    b2, s2 = windows(tab, [s], len(nb), lo, hi)
    assert float(b2[0]) == base and float(s2[0]) == step, "the built rows moved the window"
    return dict(name=name, spec=spec, tab=tab, built=built, base=base, step=step, params=params, solved=solved, sc=sc)


# ---------------------------------------------------------------------------------------------- corner tables
CORNERS = ((0, 0), (0, 1), (1, 0), (1, 1))       # (x: low / high, t: low / high)


def corner_table(name, nclusters=40, per_corner=256, seed=20261):
    """The table of CORNER_PROGRAMS[name] and the solved parameter vectors.  Returns a dict: tab, cluster (per row: its
    cluster, -1 for the rows of an interior cluster), params, solved (per vector: cluster, corner, edge, parameter, ulps),
    spec."""
    spec = CORNER_PROGRAMS[name]
    lo, hi, nb = spec["geom"]
    s, w, systs = spec["streamed"], spec["unwritten"], spec["systs"]
    rng = np.random.default_rng(seed)
    base_params = list(spec["base"])
    nbx, lox, hix = nb[BOXED], lo[BOXED], hi[BOXED]
    edges = []
    for j in range(nbx // 2 + 1):                                  # both domain ends first and often
        edges += [j, nbx - j]
    edges = [0, nbx] + edges
    parts, labels, params, solved = [], [], [], []

    def cluster_rows(n, x, t, bucket):
        rows = np.zeros((n, NFIELDS), np.float32)
        rows[:, BOXED], rows[:, TRUTH] = x, t
        rows[:, s] = lo[s] + (rng.integers(0, nb[s], n) + 0.5) * (hi[s] - lo[s]) / nb[s]     # mid-bin: never decides
        rows[:, w] = lo[w] + (bucket + 0.5) * (hi[w] - lo[w]) / nb[w]
        return rows

    for i in range(nclusters):
        k, (ix, it) = edges[i % len(edges)], CORNERS[i % 4]
        dx, dt = rng.uniform(0.01, 0.05, 2)
        delta = rng.choice([-1.0, 1.0]) * rng.uniform(0.2, 0.6)
        off = rng.uniform(-0.003, 0.003)

        def corner_miss(x0):
            return image(systs, BOXED, x0 + ix * dx, x0 + delta + it * dt, base_params) - (lox + k * (hix - lox) / nbx + off)
        x0 = bisect(corner_miss, -40.0, 40.0)
        assert x0 is not None, (name, i)
        xs = np.array([x0, x0 + dx], np.float32)
        ts = np.array([x0 + delta, x0 + delta + dt], np.float32)
        assert xs[0] < xs[1] and ts[0] < ts[1]
        bucket = i % nb[w]
        x = np.repeat(xs[[0, 0, 1, 1]], per_corner)
        t = np.repeat(ts[[0, 1, 0, 1]], per_corner)
        parts.append(cluster_rows(4 * per_corner, x, t, bucket))
        labels.append(np.full(4 * per_corner, i))
        if i % 3 == 0:                                             # an interior beside it: its corners are no rows
            n = 600
            shift = 1.3 * (hix - lox) / nbx
            parts.append(cluster_rows(n, rng.uniform(xs[0], xs[1], n) + shift, rng.uniform(ts[0], ts[1], n) + shift, bucket))
            labels.append(np.full(n, -1))
        # the parameter that carries the named corner's image across edge k, to neighbouring doubles
        for free in (spec["free"][i % 2], spec["free"][1 - i % 2]):
            def miss(p):
                v = list(base_params)
                v[free] = p
                return crossing(systs, BOXED, float(xs[ix]), float(ts[it]), v, lox, hix, nbx, k)
            ab = bisect(miss, base_params[free] - 0.02, base_params[free] + 0.02, exact=True)
            if ab is not None:
                break
        if ab is None:
            continue
        for ulps in (-2, -1, 0, 1, 2, 3):                          # 0: the last double on one side, 1: the first on the other
            p = ab[0]
            for _ in range(abs(ulps)):
                p = np.nextafter(p, np.inf if ulps > 0 else -np.inf)
            v = list(base_params)
            v[free] = float(p)
            params.append(v)
            solved.append(dict(cluster=i, corner=(ix, it), edge=k, parameter=free, ulps=ulps))
    tab = np.concatenate(parts)
    labels = np.concatenate(labels)
    order = rng.permutation(tab.shape[0])
    return dict(name=name, spec=spec, tab=np.ascontiguousarray(tab[order]), cluster=labels[order], params=params,
                solved=solved)
