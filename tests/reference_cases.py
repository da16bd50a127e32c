"""Inputs of the reference-parity records (tests/golden/reference_parity.json).  TEST INFRASTRUCTURE ONLY.

The records are what the fitted code's OWN compiled CPU-mode translation units computed (oracle/ref/: pdfz and the NLL
kernels built unmodified against stand-in headers, driven by oracle/ref/ref_driver.cpp) on the cases generated here.
This file holds

  * the deterministic generators of the two case families (pdfz_cases(), nll_cases()),
  * a plain double-precision model of the sample fill, the point table and the NLL stages in Python floats.  The
    generators use it to PREDICT the inputs on which the fitted code has undefined behaviour and keep them out (a field
    that is NaN when it reaches the domain test, a flat bin index outside the histogram); the tests use its switchable
    variants as negative controls (`x <= upper`, a clamped inner index, `eff` in double, `s >= 0`, `u < exp`,
    `sigma >= 0`, the uniform after the normals), each of which must disagree with the records somewhere,
  * the encodings: the driver's binary case / result files and the JSON spelling of arrays as bit patterns, and
    load(), which pairs the regenerated cases with the recorded results.  To keep the fixture small it names each
    case's inputs by a sha256 digest instead of repeating them: load() regenerates them and requires the digest.

Nothing here reads the fitted code's tree or the driver: the recorder (tests/golden/make_reference_parity.py) and the CPU
test do.  The GPU test uses load() only.
"""
import base64
import hashlib
import json
import math
import struct

import numpy as np

SHIFT, SCALE, RESOLUTION_SCALE, CTSCALE = 0, 1, 2, 3        # the enumeration of the systematic kinds
KIND_NAME = {SHIFT: "shift", SCALE: "scale", RESOLUTION_SCALE: "resolution_scale", CTSCALE: "ctscale"}
MAX_REPLACED_SHARE = 0.02        # of a case's rows (points) that the undefined-behaviour filter may replace
MIN_BUILT_ROWS = 10              # rows of the kind a case was built for that must survive it
MAX_SAMPLES, MAX_POINTS, MAX_EVENTS = 512, 128, 300
SENTINEL = 12345.0               # pre-fill of output buffers: an untouched slot stays visible
F32 = np.float32

# ------------------------------------------------------------------------------------------------ encodings
_DTYPES = {"i32": np.int32, "u32": np.uint32, "f32": np.float32, "f64": np.float64, "i16": np.int16}
_CODE = {"i32": 0, "u32": 1, "f32": 2, "f64": 3, "i16": 4}
_NAME_OF_CODE = {v: k for k, v in _CODE.items()}


def tag_of(a):
    for k, v in _DTYPES.items():
        if a.dtype == v:
            return k
    raise TypeError(a.dtype)


def enc(a):
    """Floats and doubles as "<type>:<base64 of the little-endian bytes>": bit patterns, not decimal numbers.
    Integer arrays as [<type>, values...]."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind in "iu":
        return [tag_of(a)] + [int(v) for v in a.reshape(-1)]
    return tag_of(a) + ":" + base64.b64encode(a.astype(a.dtype.newbyteorder("<")).tobytes()).decode()


def dec(s):
    if isinstance(s, list):
        return np.array(s[1:], dtype=_DTYPES[s[0]])
    t, b = s.split(":", 1)
    return np.frombuffer(base64.b64decode(b), dtype=np.dtype(_DTYPES[t]).newbyteorder("<")).astype(_DTYPES[t])


def write_blobs(path, arrays):
    """The driver's file format: "SXRC", u32 count, then (u32 name length, name, u8 type, u64 elements, bytes)."""
    with open(path, "wb") as f:
        f.write(b"SXRC" + struct.pack("<I", len(arrays)))
        for name, a in arrays.items():
            a = np.ascontiguousarray(a)
            nb = name.encode()
            f.write(struct.pack("<I", len(nb)) + nb + struct.pack("<BQ", _CODE[tag_of(a)], a.size))
            f.write(a.astype(a.dtype.newbyteorder("<")).tobytes())


def read_blobs(path):
    with open(path, "rb") as f:
        raw = f.read()
    assert raw[:4] == b"SXRC"
    (count,), pos, out = struct.unpack_from("<I", raw, 4), 8, {}
    for _ in range(count):
        (ln,) = struct.unpack_from("<I", raw, pos)
        name = raw[pos + 4:pos + 4 + ln].decode()
        code, n = struct.unpack_from("<BQ", raw, pos + 4 + ln)
        pos += 4 + ln + 9
        dt = np.dtype(_DTYPES[_NAME_OF_CODE[code]]).newbyteorder("<")
        out[name] = np.frombuffer(raw, dtype=dt, count=n, offset=pos).astype(dt.newbyteorder("="))
        pos += n * dt.itemsize
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ the pdfz model
def _pow(x, i):
    """C's pow(x, (double) i) through the same libm (math.pow), with C's result where Python raises."""
    try:
        return math.pow(x, float(i))
    except OverflowError:
        return math.inf if (x > 0 or i % 2 == 0) else -math.inf


def geometry(case):
    nb = [int(b) for b in case["nbins"]]
    stride = [1] * len(nb)
    for i in range(len(nb) - 2, -1, -1):
        stride[i] = nb[i + 1] * stride[i + 1]
    scale = [nb[d] / (float(case["upper"][d]) - float(case["lower"][d])) for d in range(len(nb))]
    return nb, stride, stride[0] * nb[0], scale


def transform_row(case, row):
    """The systematics applied to one sample in double, in their order: each reads the fields as they are by then."""
    f = [float(v) for v in row]
    P, off, st = case["params"], case["param_offset"], case["param_stride"]
    for kind, obs, extra, pars in case["systs"]:
        p = 0.0
        for i, q in enumerate(pars):
            p += float(P[off + q * st]) * _pow(f[obs], i)
        if kind == SHIFT:
            f[obs] += p
        elif kind == SCALE:
            f[obs] *= (1 + p)
        elif kind == CTSCALE:
            f[obs] = 1 + (f[obs] - 1) * (1 + p)
        else:
            f[obs] += p * (f[obs] - f[extra])
    return f


def bin_of(case, values, geom, variant=None):
    """(status, flat index, True where an index of a dimension came out equal to its nbins) of the observables
    `values` (doubles).  status: "nan" (a NaN reached the domain test: undefined in the fitted code), "out", "in".
    variant "le_upper": `x <= upper` accepted; "clamp": every dimension's index clamped to nbins - 1."""
    nb, stride, total, scale = geom
    flat, hit = 0, False
    for d in range(len(nb)):
        e = values[d]
        if e != e:
            return "nan", None, False
        lo, hi = float(case["lower"][d]), float(case["upper"][d])
        if e < lo or (e > hi if variant == "le_upper" else e >= hi):
            return "out", None, False
        idx = int((e - lo) * scale[d])
        if idx == nb[d]:
            hit = True
        if variant == "clamp":
            idx = min(idx, nb[d] - 1)
        flat += idx * stride[d]
    return "in", flat, hit


def row_is_undefined(case, row, geom):
    st, flat, _ = bin_of(case, transform_row(case, row), geom)
    return st == "nan" or (st == "in" and not 0 <= flat < geom[2])


def point_is_undefined(case, point, geom):
    st, flat, _ = bin_of(case, [float(v) for v in point[:-1]], geom)
    return st == "nan" or (st == "in" and not 0 <= flat < geom[2])


def model_fill(case, variant=None):
    """(bins, norm, rows whose inner index equalled nbins while binned inside the histogram) by the model."""
    geom = geometry(case)
    bins, norm, hits = np.zeros(geom[2], np.uint32), 0, 0
    for row in case["samples"]:
        st, flat, hit = bin_of(case, transform_row(case, row), geom, variant)
        if st == "in":
            norm += 1
            if 0 <= flat < geom[2]:
                bins[flat] += 1
                hits += bool(hit)
    return bins, norm, hits


def model_read_bins(case):
    geom = geometry(case)
    out = np.zeros(len(case["points"]), np.int32)
    for k, pt in enumerate(case["points"]):
        st, flat, _ = bin_of(case, [float(v) for v in pt[:-1]], geom)
        if float(pt[-1]) != case["dataset"]:
            flat = -2
        out[k] = flat if st == "in" else -1
    return out


# ------------------------------------------------------------------------------------------------ pdfz cases
def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(F32)


def _rand_rows(rng, n, case, spread=0.25):
    """Rows in and around the domain; extra fields near the first observable (a truth column's habit)."""
    lo, hi = np.asarray(case["lower"]), np.asarray(case["upper"])
    nobs, nf = len(lo), case["nfields"]
    span = hi - lo
    t = np.empty((n, nf), np.float64)
    t[:, :nobs] = rng.uniform(lo - spread * span, hi + spread * span, size=(n, nobs))
    for k in range(nobs, nf):
        t[:, k] = t[:, 0] + rng.normal(0, 0.08, n) * span[0]
    return t.astype(F32)


def _inside_rows(rng, n, case):
    return _rand_rows(rng, n, case, spread=-0.2)


def _neighbours(x, rng):
    """x, or its float neighbour below / above, a third each."""
    x = _f32(x)
    r = rng.integers(0, 3, size=x.shape)
    return np.where(r == 0, x, np.where(r == 1, np.nextafter(x, F32(-np.inf)), np.nextafter(x, F32(np.inf))))


def _edge_rows(rng, n, case):
    """Rows with one observable exactly on lower, on upper, on a bin edge, or on a float neighbour of those."""
    t = _inside_rows(rng, n, case)
    nobs = len(case["nbins"])
    for i in range(n):
        d = int(rng.integers(0, nobs))
        nb = int(case["nbins"][d])
        k = [0, nb, int(rng.integers(0, nb + 1))][int(rng.integers(0, 3))]
        lo, hi = float(case["lower"][d]), float(case["upper"][d])
        edge = hi if k == nb else lo + k * ((hi - lo) / nb)
        t[i, d] = _neighbours(np.array([edge]), rng)[0]
    return t


def _solve_field(case, row, obs, target):
    """A double x for field `obs` of `row` whose transformed observable `obs` is `target`, by bisection over the
    domain widened by its span (None where the map is not monotone there or does not reach the target)."""
    lo, hi = float(case["lower"][obs]), float(case["upper"][obs])
    a, b = lo - (hi - lo), hi + (hi - lo)

    def g(x):
        r = [float(v) for v in row]
        r[obs] = x
        return transform_row(case, r)[obs] - target
    ga, gb = g(a), g(b)
    if not (ga == ga and gb == gb) or ga * gb > 0:
        return None
    for _ in range(1200):                      # (until the bracket is two neighbouring doubles: a root near 1e-300 too)
        m = 0.5 * (a + b)
        if m == a or m == b:
            break
        gm = g(m)
        if gm != gm:
            return None
        if (gm > 0) == (gb > 0):
            b, gb = m, gm
        else:
            a, ga = m, gm
    return 0.5 * (a + b)


def _moved_edge_rows(rng, n, case, obs_choices):
    """Rows that the systematics move ONTO a bin edge (or lower / upper) of a written observable: the field is solved
    for in double, rounded to float and stepped to its float neighbours.  Returns (rows, indices of the solved rows)."""
    t = _inside_rows(rng, n, case)
    built = []
    for i in range(n):
        d = int(obs_choices[int(rng.integers(0, len(obs_choices)))])
        nb = int(case["nbins"][d])
        k = int(rng.integers(0, nb + 1))
        lo, hi = float(case["lower"][d]), float(case["upper"][d])
        edge = hi if k == nb else lo + k * ((hi - lo) / nb)
        x = _solve_field(case, t[i], d, edge)
        if x is None or not np.isfinite(F32(x)):
            continue
        t[i, d] = _neighbours(np.array([x]), rng)[0]
        built.append(i)
    return t, built


SPECIALS = np.array([-0.0, 0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754944e-38, np.inf, -np.inf, 1e30, -1e30, 3e38, -3e38,
                     9.9e29, 1.01e30], dtype=np.float64).astype(F32)


def _special_rows(rng, n, case):
    t = _inside_rows(rng, n, case)
    for i in range(n):
        t[i, int(rng.integers(0, case["nfields"]))] = SPECIALS[i % SPECIALS.size]
    return t


def _points(rng, case, n=32):
    """Evaluation points: inside, outside, on lower / upper / edges and their float neighbours, both data sets and a
    data-set id that is no integer."""
    nobs = len(case["nbins"])
    base = dict(case, nfields=nobs)
    pts = np.concatenate([_rand_rows(rng, n // 3, base), _edge_rows(rng, n - n // 3, base)])
    ds = np.where(rng.uniform(size=n) < 0.75, float(case["dataset"]), float(1 - case["dataset"]))
    ds[-1] = 0.5
    return np.concatenate([pts, ds[:, None].astype(F32)], axis=1).astype(F32)


def _syst(kind, obs, pars, extra=0):
    return (int(kind), int(obs), int(extra), [int(p) for p in pars])


def _make(name, kind, rng, nobs, nfields, nbins, lower, upper, systs, params, rows_spec, dataset=0, param_offset=0,
          param_stride=1, out_offset=0, out_stride=1, norm_offset=0, norm_len=1, npoints=32, moved_obs=None):
    """One case.  rows_spec: list of (row kind, count); the rows of kind `kind` are the ones the case is built for."""
    nparams = 1 + max([max(s[3]) for s in systs] + [0])
    pbuf = np.full(param_offset + nparams * param_stride + 1, 777.0)      # slots between strides must never be read
    for q in range(nparams):
        pbuf[param_offset + q * param_stride] = params[q] if q < len(params) else 0.0
    case = dict(name=name, kind=kind, nobs=nobs, nfields=nfields, nbins=[int(b) for b in nbins],
                lower=[float(v) for v in lower], upper=[float(v) for v in upper], systs=list(systs), params=pbuf,
                param_offset=param_offset, param_stride=param_stride, out_offset=out_offset, out_stride=out_stride,
                norm_offset=norm_offset, norm_len=norm_len, dataset=dataset)
    assert nfields <= 10 and nobs <= nfields
    parts, built = [], []
    at = 0
    for rk, n in rows_spec:
        if rk == "random":
            t, b = _rand_rows(rng, n, case), range(n)
        elif rk == "edge":
            t, b = _edge_rows(rng, n, case), range(n)
        elif rk == "special":
            t, b = _special_rows(rng, n, case), range(n)
        elif rk == "moved_edge":
            t, b = _moved_edge_rows(rng, n, case, moved_obs if moved_obs is not None else sorted({s[1] for s in systs
                                                                                                 if s[1] < nobs}))
        else:
            t, b = rk(rng, n, case)                      # a case's own builder: (rows, built indices)
            rk = kind
        if rk == kind:
            built += [at + i for i in b]
        parts.append(t)
        at += n
    samples = np.concatenate(parts).astype(F32)
    assert samples.shape[0] <= MAX_SAMPLES
    geom = geometry(case)
    replaced = []
    for i in range(samples.shape[0]):
        if row_is_undefined(case, samples[i], geom):
            for _ in range(200):
                cand = _inside_rows(rng, 1, case)[0]
                if not row_is_undefined(case, cand, geom):
                    break
            else:
                raise AssertionError("no defined replacement row for " + name)
            samples[i] = cand
            replaced.append(i)
    case["samples"] = samples
    case["built"] = [i for i in built if i not in set(replaced)]
    case["replaced"] = replaced
    pts = _points(rng, case, npoints)
    preplaced = []
    for k in range(pts.shape[0]):
        if point_is_undefined(case, pts[k], geom):
            pts[k, :nobs] = _f32([0.5 * (case["lower"][d] + case["upper"][d]) for d in range(nobs)])
            preplaced.append(k)
    assert pts.shape[0] <= MAX_POINTS
    case["points"] = pts
    case["points_replaced"] = preplaced
    case["out_len"] = out_offset + pts.shape[0] * out_stride + 2
    return case


def _find_inner_hit_axis(rng):
    """(lower, upper, nbins) of an axis on which the double just below upper gets the index nbins: the product
    (x - lower) * (nbins / (upper - lower)) rounds up to nbins.  Searched, deterministically."""
    while True:
        lo = float(F32(rng.uniform(0.1, 3)))          # (positive: the shift to the double below upper is then exact)
        hi = lo + float(F32(rng.uniform(0.5, 4)))
        nb = int(rng.choice([3, 5, 6, 7, 11, 13]))
        x = math.nextafter(hi, -math.inf)
        if int((x - lo) * (nb / (hi - lo))) == nb:
            return lo, hi, nb


def _inner_hit_case(name, rng, nobs, hit_dim):
    """Rows whose index in dimension `hit_dim` (not the first) comes out equal to nbins[hit_dim] while the flat index
    stays inside the histogram: the fitted code is defined there and bins the row into the NEXT row of the dimension
    before.  A float cannot sit that close below upper, a shifted double can: every built row has the same value x in
    the hit dimension and the shift is (the double below upper) - x, exact."""
    lo, hi, nb = _find_inner_hit_axis(rng)
    lower, upper, nbins = [0.0] * nobs, [1.0] * nobs, [4, 5, 3, 2, 2][:nobs]
    lower[hit_dim], upper[hit_dim], nbins[hit_dim] = lo, hi, nb
    below = math.nextafter(hi, -math.inf)
    for frac in np.arange(0.37, 0.9, 0.01):                    # a float x from which the shift lands exactly there
        x = float(F32(lo + frac * (hi - lo)))
        shift = below - x
        if x + shift == below:
            break
    assert x + shift == below

    def rows(rng_, n, case):
        t = _inside_rows(rng_, n, case)
        t[:, hit_dim] = F32(x)
        # keep the dimensions before it off their last bin, so the flat index stays inside
        for d in range(hit_dim):
            t[:, d] = _f32(rng_.uniform(case["lower"][d], case["lower"][d] + 0.7 * (case["upper"][d] - case["lower"][d]),
                                        size=n))
        return t, range(n)
    return _make(name, "inner_nbins", rng, nobs, nobs + 1, nbins, lower, upper, [_syst(SHIFT, hit_dim, [0])], [shift],
                 [(rows, 24), ("random", 40)])


def pdfz_cases():
    rng = np.random.default_rng(20240611)
    C = []
    unit = lambda n: ([0.0] * n, [1.0] * n)                                             # noqa: E731

    # 1-5 observables, nfields from nobs to nobs + 3, both data sets
    for nobs, extra, nbins in [(1, 0, [17]), (2, 1, [5, 7]), (3, 2, [4, 3, 5]), (4, 3, [3, 4, 2, 3]),
                               (5, 0, [3, 2, 4, 2, 3]), (5, 3, [2, 3, 2, 3, 2])]:
        lo, hi = unit(nobs)
        systs = [_syst(SHIFT, nobs - 1, [0])] + ([_syst(RESOLUTION_SCALE, 0, [1], nobs + extra - 1)] if extra else [])
        C.append(_make("dims-%dobs-%dfields" % (nobs, nobs + extra), "random", rng, nobs, nobs + extra, nbins, lo, hi,
                       systs, [0.03, -0.2], [("random", 96), ("edge", 32)], dataset=nobs % 2))

    # bin counts: 1, a prime, an axis of a few thousand bins
    for name, nbins in [("nbins-1", [1]), ("nbins-prime", [13]), ("nbins-3001", [3001]), ("nbins-1x7", [1, 7]),
                        ("nbins-2003x3", [2003, 3])]:
        lo, hi = unit(len(nbins))
        C.append(_make(name, "edge", rng, len(nbins), len(nbins) + 1, nbins, lo, hi, [_syst(SCALE, 0, [0])], [0.0],
                       [("edge", 160), ("random", 32)]))

    # each kind of systematic with 1, 2 and 3 coefficients
    coef = {SHIFT: [0.04, 0.05, -0.03], SCALE: [-0.03, 0.02, 0.04], CTSCALE: [0.11, -0.05, 0.02],
            RESOLUTION_SCALE: [0.21, -0.1, 0.07]}
    for kind in (SHIFT, SCALE, CTSCALE, RESOLUTION_SCALE):
        for nc in (1, 2, 3):
            pars = [[0], [1, 0], [2, 0, 1]][nc - 1]                  # (the coefficient order is not the slot order)
            vals = [0.0] * 3
            for i, q in enumerate(pars):
                vals[q] = coef[kind][i]
            C.append(_make("%s-%dcoef" % (KIND_NAME[kind], nc), "moved_edge", rng, 2, 3, [9, 4], [0.0, 0.0],
                           [1.0, 1.0], [_syst(kind, 0, pars, 2)], vals, [("moved_edge", 96), ("random", 32)]))

    # two and three systematics on the same observable, in both orders
    two = [_syst(SHIFT, 0, [0]), _syst(SCALE, 0, [1])]
    three = [_syst(RESOLUTION_SCALE, 0, [2], 1), _syst(CTSCALE, 0, [1]), _syst(SHIFT, 0, [0])]
    for name, systs in [("order-shift-scale", two), ("order-scale-shift", two[::-1]),
                        ("order-res-ct-shift", three), ("order-shift-ct-res", three[::-1])]:
        C.append(_make(name, "moved_edge", rng, 1, 2, [11], [0.0], [1.0], systs, [0.06, -0.04, 0.15],
                       [("moved_edge", 96), ("random", 32)]))

    # resolution scale against ANOTHER observable that an earlier systematic has already moved
    C.append(_make("res-truth-is-moved-obs", "moved_edge", rng, 2, 2, [8, 6], [0.0, 0.0], [1.0, 1.0],
                   [_syst(SCALE, 1, [0]), _syst(RESOLUTION_SCALE, 0, [1], 1)], [0.3, -0.25],
                   [("moved_edge", 96), ("random", 32)], moved_obs=[0]))
    # a systematic on a field that is no observable: it moves the truth column the next one reads
    C.append(_make("syst-on-extra-field", "moved_edge", rng, 1, 3, [10], [0.0], [1.0],
                   [_syst(SHIFT, 2, [0]), _syst(SCALE, 1, [2]), _syst(RESOLUTION_SCALE, 0, [1], 2)],
                   [0.05, 0.4, 3.0], [("moved_edge", 96), ("random", 32)], moved_obs=[0]))

    # offsets and strides of the three buffers, data set 1
    c3 = [_syst(SHIFT, 1, [0]), _syst(SCALE, 0, [1]), _syst(RESOLUTION_SCALE, 0, [2], 3)]
    C.append(_make("buffers-strided", "random", rng, 3, 5, [6, 5, 4], *unit(3), c3, [0.02, -0.01, 0.07],
                   [("random", 128)], dataset=1, param_offset=2, param_stride=3, out_offset=5, out_stride=2,
                   norm_offset=3, norm_len=6))
    C.append(_make("buffers-offset-only", "random", rng, 2, 4, [7, 3], *unit(2), c3[1:], [0.0, 0.05, -0.3],
                   [("random", 128)], dataset=0, param_offset=1, param_stride=1, out_offset=3, out_stride=1,
                   norm_offset=1, norm_len=2))

    # -0.0, denormals, infinities, values around 1e30
    C.append(_make("special-values-plain", "special", rng, 2, 3, [8, 3], [0.0, -1.0], [1.0, 1.0], [], [0.0],
                   [("special", 240), ("random", 272)]))
    C.append(_make("special-values-systs", "special", rng, 2, 4, [8, 3], [0.0, -1.0], [1.0, 1.0],
                   [_syst(SCALE, 0, [0]), _syst(RESOLUTION_SCALE, 1, [1], 3), _syst(SHIFT, 0, [2])],
                   [0.5, 0.25, 1e-41], [("special", 240), ("random", 272)]))

    # ... and a scale to exactly zero: 0 * inf is a NaN at the domain test, which the filter must take out
    C.append(_make("special-values-scaled-to-zero", "special", rng, 2, 3, [8, 3], [0.0, -1.0], [1.0, 1.0],
                   [_syst(SCALE, 0, [0])], [-1.0], [("special", 90), ("random", 422)]))

    # domains far from zero, and a tiny one
    for off in (3.0e4, 1.0e6, -2.5e5):
        C.append(_make("far-domain-%g" % off, "edge", rng, 3, 5, [20, 6, 5], [off, off - 1.0, 0.0],
                       [off + 1.0, off + 1.0, 1.0], [_syst(SHIFT, 1, [0]), _syst(SCALE, 0, [1]),
                                                     _syst(RESOLUTION_SCALE, 0, [2], 3)], [0.02, 1e-7, 0.07],
                       [("edge", 128), ("random", 64)]))
    C.append(_make("tiny-domain", "edge", rng, 1, 2, [4], [1.0], [1.0 + 2.0 ** -20], [_syst(SHIFT, 0, [0])], [2.0 ** -23],
                   [("edge", 128), ("random", 64)]))

    # parameters: zero, small, wild, negative
    for name, p in [("pars-zero", [0.0, 0.0, 0.0]), ("pars-small", [1e-9, -1e-12, 1e-300]),
                    ("pars-wild-30", [0.0, 30.0, 0.0]), ("pars-wild-40", [0.0, 0.0, 40.0]),
                    ("pars-wild-mixed", [0.0, -25.0, 12.0]), ("pars-wild-1e4", [0.0, 1e4, -1e4]),
                    ("pars-wild-1e300", [0.0, 1e300, 0.0]), ("pars-minus-one", [0.0, -1.0, 0.0]),
                    ("pars-negative", [-0.3, -0.4, -1.0])]:
        # (the solved rows keep some samples inside the domain at the wild magnitudes, on the edges of obs 0)
        C.append(_make(name, "random", rng, 3, 5, [20, 6, 5], *unit(3), c3, p, [("random", 96), ("moved_edge", 64)],
                       moved_obs=[0]))

    # an inner index equal to nbins with the flat index inside the histogram
    C.append(_inner_hit_case("inner-index-2d", rng, 2, 1))
    C.append(_inner_hit_case("inner-index-3d-middle", rng, 3, 1))
    C.append(_inner_hit_case("inner-index-4d-last", rng, 4, 3))
    assert len({c["name"] for c in C}) == len(C)
    return C


def pdfz_blobs(case):
    """The driver's pdfz case file."""
    systs = []
    for kind, obs, extra, pars in case["systs"]:
        assert len(pars) <= 3
        systs += [kind, obs, extra, len(pars)] + pars + [0] * (3 - len(pars))
    return dict(
        meta=np.array([case["nfields"], case["nobs"], case["dataset"], case["param_offset"], case["param_stride"],
                       case["out_offset"], case["out_stride"], case["norm_offset"]], np.int32),
        samples=case["samples"].reshape(-1), lower=np.array(case["lower"], np.float64),
        upper=np.array(case["upper"], np.float64), nbins=np.array(case["nbins"], np.int32),
        systs=np.array(systs, np.int32), points=case["points"].reshape(-1), params=np.asarray(case["params"], np.float64),
        out=np.full(case["out_len"], SENTINEL, np.float32), norm=np.full(case["norm_len"], 55, np.uint32))


def digest(blobs):
    """sha256 over a case file's arrays (name, type, bytes): the fixture names a case's inputs by it."""
    h = hashlib.sha256()
    for name in sorted(blobs):
        a = np.ascontiguousarray(blobs[name])
        h.update(name.encode() + b"\0" + tag_of(a).encode() + a.astype(a.dtype.newbyteorder("<")).tobytes())
    return h.hexdigest()[:32]


def pdfz_to_json(case, res):
    """The fixture's entry: the inputs by digest (pdfz_cases() regenerates them), the driver's results as bit patterns
    (the histogram sparse)."""
    nz = np.flatnonzero(res["bins"]).astype(np.int32)
    return dict(
        name=case["name"], kind=case["kind"], inputs=digest(pdfz_blobs(case)), rows=int(case["samples"].shape[0]),
        built=len(case["built"]), replaced=len(case["replaced"]), points_replaced=len(case["points_replaced"]),
        results=dict(total_nbins=int(res["total_nbins"][0]), bin_volume=enc(res["bin_volume"]), bins_at=enc(nz),
                     bins_count=enc(res["bins"][nz]), norm=enc(res["norm"]), out=enc(res["out"]),
                     read_bins=enc(res["read_bins"])))


def pdfz_results(j):
    r = j["results"]
    bins = np.zeros(r["total_nbins"], np.uint32)
    bins[dec(r["bins_at"])] = dec(r["bins_count"])
    return dict(bins=bins, norm=dec(r["norm"]), out=dec(r["out"]), read_bins=dec(r["read_bins"]),
                bin_volume=dec(r["bin_volume"]), total_nbins=r["total_nbins"])


def oracle_systs(case):
    return [dict(type=k, obs=o, extra_field=e, pars=p) for k, o, e, p in case["systs"]]


# ------------------------------------------------------------------------------------------------ the NLL model
def _log(x):
    return math.log(x) if x < math.inf else math.inf


def model_chunks(c, variant=None, sentinel=None):
    """nll_event_chunks in CPU mode (one lane over all events).  variant "eff_double": the efficiency kept in double;
    "s_ge_0": events with s == 0 contribute log(0)."""
    ne, ns = c["ne"], c["ns"]
    lut, pars = c["lut"], c["pars"]
    total = 0.0
    with np.errstate(all="ignore"):
        for i in range(ne):
            s = 0.0
            for j in range(ns):
                v = lut[j * ne + i]
                eff = np.float64(1.0) * np.float64(c["norms"][j]) / np.float64(c["n_mc"][j])
                if variant != "eff_double":
                    eff = np.float64(F32(eff))
                vv = 0.0 if v != v else float(v)
                s += float(pars[c["source_id"][j]]) * float(c["nexpected"][j]) * float(eff) * vv
            if s > 0:
                total += _log(s)
            elif variant == "s_ge_0" and s == 0:
                total += -math.inf
    return sentinel if total != total else total


def model_total(c, variant=None):
    """nll_total.  variant "sigma_ge_0": the Gaussian constraint applied for sigma >= 0."""
    with np.errstate(all="ignore"):
        total = -float(c["events_total"][0])
        if total != total:
            return 1e18
        pars = c["pars"]
        for i in range(c["nsignals"]):
            total += float(np.float64(pars[c["source_id"][i]]) * np.float64(c["nexpected"][i])
                           * np.float64(c["norms"][i]) / np.float64(c["n_mc"][i]))
        for i in range(c["nparameters"]):
            if i < c["nsources"] and pars[i] < 0:
                return 1e18
            sg = c["sigmas"][i]
            if sg > 0 or (variant == "sigma_ge_0" and sg == 0):
                x = float((np.float64(pars[i]) - np.float64(c["means"][i])) / np.float64(sg))
                total += 0.5 * x * x
        return total


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def model_decide(u, nc, np_, debug=False, variant=None):
    """variant "u_lt": `u < exp(nc - np)`."""
    if debug or np_ < nc:
        return True
    e = _exp(nc - np_)
    return u < e if variant == "u_lt" else u <= e


def model_combo(c, variant=None):
    """finish_nll_jump_pick_combo, c["nsteps"] times on carried state, the draws taken from the script c["rng"]: the
    driver's (trace, itrace, jump_buffer).  variant "uniform_last": the step's uniform drawn AFTER its normals."""
    P, npart = c["nparameters"], c["npartial"]
    jw = c["jump_width"]
    free = [i for i in range(P) if jw[i] > 0]
    script = [float(v) for v in c["rng"]]
    cur, prop = [float(v) for v in c["v_current"]], [float(v) for v in c["v_proposed"]]
    nll_cur, acc, cnt = float(c["nll_current"][0]), int(c["accepted"][0]), int(c["counter"][0])
    jb = c["jump_buffer"].copy()
    trace, itrace, draws = [], [], 0
    for s in range(c["nsteps"]):
        total = 0.0
        for v in c["sums"][s * npart:(s + 1) * npart]:
            total += float(v)
        nll_prop = model_total(dict(c, pars=np.array(prop), events_total=[total]))
        z = None
        if variant == "uniform_last":
            z = [script.pop(0) for _ in free]
        u = script.pop(0)
        if model_decide(u, nll_cur, nll_prop, bool(c["debug"])):
            nll_cur, cur, acc = nll_prop, list(prop), acc + 1
        with np.errstate(over="ignore"):
            jb[cnt * (P + 1):cnt * (P + 1) + P] = np.array(cur).astype(F32)
            jb[cnt * (P + 1) + P] = F32(nll_cur)
        cnt += 1
        if z is None:
            z = [script.pop(0) for _ in free]
        prop = list(cur)
        for i, zi in zip(free, z):
            prop[i] = cur[i] + float(jw[i]) * zi
        draws += 1 + len(free)
        trace += [nll_cur, nll_prop] + cur + prop
        itrace += [acc, cnt, draws]
    return np.array(trace), np.array(itrace, np.int32), jb


# ------------------------------------------------------------------------------------------------ NLL cases
def _nll_inputs(rng, ne, ns, nsources, nsyst=2):
    lut = rng.uniform(0.0, 2.0, size=ns * ne).astype(F32)
    P = nsources + nsyst
    n_mc = rng.integers(1000, 100000, ns).astype(np.uint32)
    return dict(ne=ne, ns=ns, nsignals=ns, nsources=nsources, nparameters=P, lut=lut,
                pars=np.concatenate([rng.uniform(0.5, 1.5, nsources), rng.normal(0, 0.1, nsyst)]),
                means=np.concatenate([np.ones(nsources), np.zeros(nsyst)]),
                sigmas=np.concatenate([np.where(np.arange(nsources) % 3 == 0, 0.3, 0.0), np.full(nsyst, 0.1)]),
                nexpected=rng.uniform(10, 100, ns), n_mc=n_mc,
                norms=(n_mc * rng.uniform(0.3, 1.0, ns)).astype(np.uint32),
                source_id=(np.arange(ns) % nsources).astype(np.int16))


def _norms_0_full(c):
    """No sample of a signal inside the domain, or every one."""
    c["norms"][::2] = 0
    c["norms"][1::2] = c["n_mc"][1::2]


def _ratio(c):
    """norms / n_mc that round differently as float and as double."""
    k = np.arange(c["ns"]) % 6
    c["n_mc"][:] = np.array([3, 7, 10, 1000003, 49, 4194303])[k]
    c["norms"][:] = np.array([1, 5, 3, 777777, 13, 2796201])[k]


def _chunk_mode(rng, c, mode):
    ne, ns = c["ne"], c["ns"]
    lut = c["lut"]
    pick = lambda frac: rng.uniform(size=lut.size) < frac                                # noqa: E731
    if mode == "nan0":
        lut[pick(0.15)] = np.nan
        lut[pick(0.15)] = 0.0
    elif mode == "denormal":
        lut[pick(0.3)] = F32(1e-42)
        lut[pick(0.1)] = F32(1.1754944e-38)
    elif mode == "inf":
        lut[pick(0.1)] = np.inf
    elif mode == "negative":
        lut[pick(0.5)] *= F32(-1.5)
    elif mode == "zero-event":                 # an event that no signal can make: s is exactly 0
        for i in range(0, ne, 3):
            lut[i::ne] = np.where(np.arange(ns) % 2 == 0, 0.0, np.nan)
    elif mode == "norms-0-full":
        _norms_0_full(c)
    elif mode == "ratio":
        _ratio(c)
    elif mode == "par-negative":
        c["pars"][0] = -0.4
    elif mode == "par-zero":
        c["pars"][0] = 0.0
        lut[:ne][pick(0.2)[:ne]] = np.inf      # 0 * inf inside an event's sum
    elif mode == "par-nan":
        c["pars"][0] = np.nan
    elif mode == "all-empty":
        lut[:] = np.nan
    else:
        assert mode == "ordinary"


CHUNK_MODES = ["ordinary", "nan0", "denormal", "inf", "negative", "zero-event", "norms-0-full", "ratio", "par-negative",
               "par-zero", "par-nan", "all-empty"]
NLL_NS = [1, 2, 15, 16, 17, 33]


def nll_cases():
    """List of dicts: name, op, and the op's inputs.  ops: chunks, reduce, total, decider, pick, combo."""
    rng = np.random.default_rng(20240612)
    C = []
    shapes = [(ne, ns) for ne in (1, 2, 63) for ns in NLL_NS] + [(300, 1), (300, 17)]
    for k, (ne, ns) in enumerate(shapes):
        nsources = [1, ns, ns // 2 + 1][k % 3]
        mode = CHUNK_MODES[k % len(CHUNK_MODES)]
        c = _nll_inputs(rng, ne, ns, nsources)
        _chunk_mode(rng, c, mode)
        C.append(dict(c, name="chunks-ne%d-ns%d-%s" % (ne, ns, mode), op="chunks", sums=np.array([SENTINEL])))
    # every mode at the shape where a signal group of sixteen is one over
    for mode in CHUNK_MODES:
        c = _nll_inputs(rng, 21, 17, 5)
        _chunk_mode(rng, c, mode)
        C.append(dict(c, name="chunks-modes-%s" % mode, op="chunks", sums=np.array([SENTINEL])))

    # reduce: 1, 2, 1000 partial sums
    big = rng.normal(0, 1e3, 1000)
    C.append(dict(name="reduce-1", op="reduce", sums=np.array([-3.25])))
    C.append(dict(name="reduce-2-cancel", op="reduce", sums=np.array([1e16, -1e16 + 2.0])))
    C.append(dict(name="reduce-1000", op="reduce", sums=big))
    C.append(dict(name="reduce-1000-cancel", op="reduce", sums=np.concatenate([big[:500] * 1e10, -big[:500] * 1e10])
                  + rng.uniform(0, 1, 1000)))
    C.append(dict(name="reduce-inf", op="reduce", sums=np.array([1.0, np.inf, 2.0])))
    C.append(dict(name="reduce-inf-minus-inf", op="reduce", sums=np.array([np.inf, 1.0, -np.inf])))
    C.append(dict(name="reduce-nan", op="reduce", sums=np.array([1.0, np.nan, 2.0])))

    # total
    def total_case(name, ns, nsources, events_total=123.456, edit=None):
        c = _nll_inputs(rng, 1, ns, nsources)
        c.update(name="total-" + name, op="total", events_total=np.array([events_total]), nll=np.array([SENTINEL]))
        if edit:
            edit(c)
        del c["lut"]
        C.append(c)

    def setv(key, idx, val):
        def f(c):
            c[key][idx] = val
        return f
    for k, ns in enumerate(NLL_NS):
        total_case("ordinary-ns%d" % ns, ns, [1, ns, ns // 2 + 1][k % 3])
    total_case("events-nan", 2, 2, np.nan)
    total_case("events-plus-inf", 2, 2, np.inf)
    total_case("events-minus-inf", 2, 2, -np.inf)
    total_case("source-negative", 15, 6, edit=setv("pars", 3, -1e-300))
    total_case("source-minus-zero", 15, 6, edit=setv("pars", 3, -0.0))
    total_case("source-zero", 16, 16, edit=setv("pars", 0, 0.0))
    total_case("source-nan", 17, 5, edit=setv("pars", 2, np.nan))
    total_case("syst-negative", 17, 5, edit=setv("pars", 6, -0.5))
    total_case("syst-nan", 33, 9, edit=setv("pars", 10, np.nan))
    total_case("sigma-zero-all", 2, 2, edit=lambda c: c["sigmas"].fill(0.0))
    total_case("sigma-zero-off-mean", 16, 7, edit=lambda c: (setv("sigmas", 8, 0.0)(c), setv("pars", 8, 0.25)(c)))
    total_case("sigma-zero-on-mean", 16, 7, edit=lambda c: (setv("sigmas", 8, 0.0)(c), setv("pars", 8, 0.0)(c)))
    total_case("sigma-negative", 15, 15, edit=setv("sigmas", 15, -0.1))
    total_case("sigma-tiny", 15, 15, edit=setv("sigmas", 16, 1e-300))
    total_case("sigma-denormal", 2, 1, edit=setv("sigmas", 1, 5e-324))
    total_case("norms-0-full", 33, 33, edit=_norms_0_full)
    total_case("ratio", 17, 17, edit=_ratio)
    total_case("negative-source-after-nan-sigma", 2, 2, edit=lambda c: (setv("sigmas", 0, np.nan)(c),
                                                                        setv("pars", 1, -2.0)(c)))

    # decider, u scripted
    below1 = math.nextafter(1.0, 0.0)

    def decider(name, nc, np_, u, counter=0, accepted=0, P=3):
        C.append(dict(name="decider-" + name, op="decider", nparameters=P, rng=np.array([u]),
                      nll_current=np.array([nc]), nll_proposed=np.array([np_]),
                      v_current=np.arange(1, P + 1) * 0.5, v_proposed=np.arange(1, P + 1) * 0.5 + 0.125 + 1e-9,
                      accepted=np.array([accepted], np.int32), counter=np.array([counter], np.int32),
                      jump_buffer=np.full((counter + 2) * (P + 1), SENTINEL, F32)))
    decider("downhill", 10.0, 9.0, below1)
    decider("equal", 10.0, 10.0, below1)
    decider("equal-u-zero", 10.0, 10.0, 0.0)
    for dn, (nc, np_) in {"uphill-half": (10.0, 10.5), "uphill-3": (-7.25, -4.25), "uphill-tiny": (1e5, 1e5 + 1e-9)}.items():
        e = math.exp(nc - np_)
        decider(dn + "-u-below", nc, np_, math.nextafter(e, 0.0))
        decider(dn + "-u-at", nc, np_, e)
        decider(dn + "-u-above", nc, np_, math.nextafter(e, 2.0))
    decider("uphill-u-zero", 10.0, 800.0, 0.0)                      # exp underflows to a denormal or 0: 0 <= it
    decider("uphill-far-u-zero", 10.0, 2000.0, 0.0)                 # exp is exactly 0: 0 <= 0
    decider("uphill-u-largest", 10.0, 10.0 + 1e-15, below1)
    decider("both-1e18", 1e18, 1e18, below1)
    decider("from-1e18", 1e18, 55.0, below1)
    decider("to-1e18", 55.0, 1e18, 0.0)
    decider("inf-minus-inf", np.inf, np.inf, 0.0)
    decider("minus-inf-both", -np.inf, -np.inf, 0.0)
    decider("proposed-nan", 10.0, np.nan, 0.0)
    decider("current-nan", np.nan, 10.0, 0.0)
    decider("row-at-counter-3", 10.0, 9.0, 0.5, counter=3, accepted=2)
    decider("row-at-counter-2-rejected", 10.0, 60.0, 0.5, counter=2, accepted=1, P=1)
    decider("overflowing-float-row", 1e300, 1e200, 0.5)

    # proposals: widths positive, 0, negative, NaN
    C.append(dict(name="pick-mixed", op="pick", n=6, rng=np.array([0.5, -1.25, 3.0]),
                  jump_width=np.array([0.1, 0.0, -1.0, np.nan, 0.33333334, 1e-30], F32),
                  v_current=np.array([1.0, 2.0, 3.0, 4.0, -5.0, 1e10]), v_proposed=np.full(6, SENTINEL)))
    C.append(dict(name="pick-all-fixed", op="pick", n=3, rng=np.zeros(0), jump_width=np.array([-1.0, -1.0, 0.0], F32),
                  v_current=np.array([1.0, np.nan, np.inf]), v_proposed=np.full(3, SENTINEL)))
    C.append(dict(name="pick-float-width-promoted", op="pick", n=2, rng=np.array([0.7071067811865476, -3.0]),
                  jump_width=np.array([0.1, 16777217.0], F32), v_current=np.array([0.3, 1e-3]),
                  v_proposed=np.full(2, SENTINEL)))

    # whole steps, three in a row on carried state
    def combo(name, ns, nsources, widths, u, debug=False, nll_current=1e9, sums_edit=None, edit=None, npartial=5):
        c = _nll_inputs(rng, 1, ns, nsources)
        del c["lut"]
        P = c["nparameters"]
        jw = np.array((widths * P)[:P], F32)
        nfree = int(np.count_nonzero(jw > 0))
        sums = rng.uniform(-50, 50, size=(3, npartial))
        if sums_edit:
            sums_edit(sums)
        script = []
        for s in range(3):
            script += [u[s]] + list(rng.normal(0, 1, nfree))
        c.update(name="combo-" + name, op="combo", npartial=npartial, nsteps=3, debug=int(debug), sums=sums.reshape(-1),
                 rng=np.array(script), nll_current=np.array([nll_current]), nll_proposed=np.array([SENTINEL]),
                 v_current=c["pars"].copy(), v_proposed=c["pars"] * 1.01, accepted=np.zeros(1, np.int32),
                 counter=np.zeros(1, np.int32), jump_buffer=np.full(4 * (P + 1), SENTINEL, F32), jump_width=jw)
        del c["pars"]
        if edit:
            edit(c)
        C.append(c)
    combo("accept-reject-accept", 2, 2, [0.01], [0.5, below1, 0.0], nll_current=-1e3,
          sums_edit=lambda s: (s.__setitem__((0, 0), 2e3), s.__setitem__((1, 0), -1e3), s.__setitem__((2, 0), 5e3)))
    # debug mode accepts a step that the Metropolis rule rejects: the second is uphill by thousands, u the largest
    combo("debug", 15, 6, [0.02, 0.0], [below1, below1, below1], debug=True, nll_current=-1e3,
          sums_edit=lambda s: (s.__setitem__((0, 0), 2e3), s.__setitem__((1, 0), -1e3), s.__setitem__((2, 0), 5e3)))
    combo("parameter-0-fixed", 17, 5, [-1.0, 0.05, 0.05], [0.3, 0.6, 0.9])
    combo("all-fixed", 2, 1, [-1.0], [0.1, 0.2, 0.3])
    combo("nan-sum-then-recover", 16, 16, [0.01], [0.5, 0.5, 0.5], sums_edit=lambda s: s.__setitem__((0, 2), np.nan))
    combo("negative-rate-proposed", 33, 9, [0.01], [0.5, 0.5, 0.5],
          edit=lambda c: c["v_proposed"].__setitem__(4, -0.01))
    assert len({c["name"] for c in C}) == len(C)
    return C


_NLL_META = {
    "chunks": lambda c: [0, c["ne"], c["ns"]],
    "reduce": lambda c: [1, c["sums"].size],
    "total": lambda c: [2, c["nparameters"], c["nsignals"], c["nsources"]],
    "decider": lambda c: [3, c["nparameters"]],
    "pick": lambda c: [4, c["n"]],
    "combo": lambda c: [5, c["nparameters"], c["nsignals"], c["nsources"], c["npartial"], c["nsteps"], c["debug"]],
}


def nll_arrays(case):
    return {k: v for k, v in case.items() if isinstance(v, np.ndarray)}


def nll_blobs(case):
    b = dict(meta=np.array(_NLL_META[case["op"]](case), np.int32))
    b.update(nll_arrays(case))
    return b


def nll_to_json(case, res):
    return dict(name=case["name"], op=case["op"], inputs=digest(nll_blobs(case)),
                results={k: enc(v) for k, v in res.items()})


def load(path):
    """The fixture as dict(pdfz=[(case, results)], nll=[(case, results)], raw=the file): the cases regenerated here
    and required to be the recorded ones by name and digest, the results decoded."""
    with open(path) as f:
        fx = json.load(f)
    out = dict(raw=fx)
    for family, cases, blobs_of, results_of in (
            ("pdfz", pdfz_cases(), pdfz_blobs, pdfz_results),
            ("nll", nll_cases(), nll_blobs, lambda j: {k: dec(v) for k, v in j["results"].items()})):
        assert [c["name"] for c in cases] == [j["name"] for j in fx[family]], family + ": not the recorded cases"
        for c, j in zip(cases, fx[family]):
            assert digest(blobs_of(c)) == j["inputs"], c["name"] + ": the generated inputs are not the recorded ones"
        out[family] = [(c, results_of(j)) for c, j in zip(cases, fx[family])]
    return out
