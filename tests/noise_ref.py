"""Reference arithmetic for the NOISE rows (csrc/acme_source.h, acme_batch_set_source_noise) that shares no code with the
library: Philox4x32-10 in Python's unbounded integers (and the same rounds over uint64 arrays where speed matters), the uniform
draw as an exact double, the Gaussian draw from mpmath at 120 bits at the exact u1 and the exact angle, the final fma with one
rounding.  Shared by test_noise_sources.py (CPU emulator) and test_gpu_noise_sources.py (MI355X)."""
import functools

import numpy as np

import source_ref as sr
from exact_ref import U, fma_fast

M0, M1 = 0xD2511F53, 0xCD9E8D57          # the round's multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # the key's increments
MASK = 0xFFFFFFFF

# the published Random123 known answers of philox4x32_10: (counter, key, output)
KNOWN_ANSWERS = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                 ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                 ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def philox(counter, key):
    """Philox4x32-10 in unbounded integers: counter (c0 ... c3), key (k0, k1) -> (r0 ... r3)"""
    c0, c1, c2, c3 = (int(c) for c in counter)
    k0, k1 = (int(k) for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def words(stream, row, q):
    """the block of (stream, row, q) for an array of counters q (integers below 2^64): r0 ... r3 as uint64 arrays.  The same
    rounds as ``philox`` on uint64 lanes (a product of two 32-bit words fits)"""
    q = np.asarray(q, dtype=np.uint64)
    m = np.uint64(MASK)
    s = int(stream) % 2 ** 64                           # (the stream as an unsigned 64-bit value)
    c0, c1 = q & m, q >> np.uint64(32)
    c2, c3 = np.full(q.shape, row, dtype=np.uint64), np.zeros(q.shape, dtype=np.uint64)
    k0, k1 = s & MASK, s >> 32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def counters(n0, T, hold):
    """q = n div hold for the clocks n0 ... n0 + T - 1 (below 2^63), a uint64 array"""
    return (np.uint64(int(n0)) + np.arange(T, dtype=np.uint64)) // np.uint64(int(hold))


def draw53(r0, r1):
    """x = r0 + 2^32 (r1 mod 2^21)"""
    return r0 + ((r1 & np.uint64(0x1FFFFF)) << np.uint64(32))


def uniform_u(x):
    """U = (2 x + 1 - 2^53) 2^-53 as doubles: an odd integer of magnitude below 2^53 times a power of two, so exact"""
    s = (np.uint64(2) * x + np.uint64(1)).astype(np.int64) - np.int64(2 ** 53)
    return s.astype(np.float64) * 2.0 ** -53


def uniform_value(amp, offset, u):
    """fma(amp, U, offset) with one rounding, for an array of U"""
    amp, offset = float(amp), float(offset)
    if offset == 0.0:
        return amp * u                                  # (a product alone is rounded once)
    return np.array([fma_fast(amp, float(v), offset) for v in u.ravel()]).reshape(u.shape)


def exact_gauss(x, r2):
    """(R, g) = (sqrt(-2 log u1), R sin th) at u1 = (x + 1) 2^-53 and th = 2 pi kappa / 2^32, kappa = r2 taken to
    (-2^31, 2^31], as mpmath numbers of 120 bits"""
    import mpmath
    with mpmath.workprec(120):
        u1 = mpmath.mpf(int(x) + 1) / 2 ** 53
        k = int(r2) - 2 ** 32 if 2 * int(r2) > 2 ** 32 else int(r2)
        R = mpmath.sqrt(-2 * mpmath.log(u1))
        return R, R * mpmath.sin(2 * mpmath.pi * k / 2 ** 32)


def gauss_bound(amp, offset, R, g):
    """Bound on |rendered - fma(amp, g, offset) evaluated exactly| for one GAUSSIAN element:
    (|amp| (12 R + 3 |g|) + |amp g| + |offset|) 2^-53 with R and g the exact values.  12 R: the sine's error as
    source_ref.sine_bound has it (angle 7.4, sin 4, rounded up), an absolute error on a value of magnitude at most 1, scaled by
    R.  3 |g|: log within one unit in the last place (2 x 2^-53 relative) halved by the square root, plus the square root's
    and the product's own roundings, rounded up.  The last two terms: the final fma, as in sine_bound.  Derived, not
    measured."""
    return (abs(amp) * (12.0 * float(R) + 3.0 * abs(float(g))) + abs(float(amp) * float(g)) + abs(offset)) * U


def gauss_error(got, amp, offset, g):
    """|got - (amp g + offset)| with the right-hand side at 120 bits, as a float"""
    import mpmath
    with mpmath.workprec(120):
        return float(abs(mpmath.mpf(float(got)) - (mpmath.mpf(float(amp)) * g + mpmath.mpf(float(offset)))))


# ---- rows as the tests describe them ---------------------------------------------------------------------------------------------
def noise(dist="gaussian", hold=1, stream=None, seed=0, amp=None, offset=None):
    """a NOISE row's description, next to source_ref's dicts of the other kinds"""
    return dict(kind="noise", dist=dist, hold=hold, stream=stream, seed=seed, amp=amp, offset=offset)


def streams(k, N):
    return [seed_stream(k["seed"], i) for i in range(N)] if k["stream"] is None else [int(s) for s in k["stream"]]


def seed_stream(seed, i):
    return int(seed) * 2 ** 32 + i


def row_words(k, row, N, T, n0):
    """per instance the (x, r2) of every sample: lists of N uint64 arrays [T]"""
    q = counters(n0, T, k["hold"])
    out = []
    for s in streams(k, N):
        r0, r1, r2, _ = words(s, row, q)
        out.append((draw53(r0, r1), r2))
    return out


def uniform_row(k, row, N, T, n0):
    """[N, T]: every element of a UNIFORM row, exactly"""
    amp, off = sr.par(k.get("amp"), N, 1.0), sr.par(k.get("offset"), N, 0.0)
    return np.stack([uniform_value(amp[i], off[i], uniform_u(x)) for i, (x, _) in enumerate(row_words(k, row, N, T, n0))])


def gauss_row_float(k, row, N, T, n0):
    """[N, T]: a GAUSSIAN row in plain double arithmetic with the header's formulas (for statistics, not for bounds)"""
    amp, off = sr.par(k.get("amp"), N, 1.0), sr.par(k.get("offset"), N, 0.0)
    out = []
    for i, (x, r2) in enumerate(row_words(k, row, N, T, n0)):
        kap = r2.astype(np.int64) - np.where(2 * r2.astype(np.int64) > 2 ** 32, 2 ** 32, 0)
        out.append(amp[i] * (np.sqrt(-2.0 * np.log((x + np.uint64(1)).astype(np.float64) * 2.0 ** -53)) * np.sin(2 * np.pi * (kap / 2.0 ** 32))) + off[i])
    return np.stack(out)


def check_gauss_row(got, k, row, N, n0, samples):
    """got [N, T] against mpmath for the (instance, sample) pairs of ``samples``; returns the worst error in units of its
    bound (asserts it is at most 1)"""
    amp, off = sr.par(k.get("amp"), N, 1.0), sr.par(k.get("offset"), N, 0.0)
    w = row_words(k, row, N, got.shape[1], n0)
    worst = 0.0
    for i, t in samples:
        R, g = exact_gauss(w[i][0][t], w[i][1][t])
        err, bound = gauss_error(got[i, t], amp[i], off[i], g), gauss_bound(amp[i], off[i], R, g)
        worst = max(worst, err / bound)
        assert err <= bound, (i, t, n0, float(got[i, t]), err / U, bound / U)
    return worst


def apply_sources(r, kinds):
    """arm ``kinds`` on a ModelRunner: source_ref.apply_sources that also forwards a NOISE row's keywords"""
    for row, k in enumerate(kinds):
        if k is None:
            continue
        if k["kind"] == "noise":
            r.set_source(row, "noise", amp=k.get("amp"), offset=k.get("offset"), dist=k["dist"], hold=k["hold"], stream=k["stream"],
                         seed=k["seed"])
        else:
            sr.apply_sources(r, [None] * row + [k])
    return r


# ---- the defining property: a source run is acme_batch_run on the rendered u, bit for bit ------------------------------------------
def _call(r, fn, u, T, ny, mem, keep, arrays, wait=False):
    """one run entry point of the C ABI on host or "device" arrays; returns y [N, T, ny] or None"""
    if mem == 0:
        ub = None if u is None else np.ascontiguousarray(u)
        y = np.full((r.n, T, ny), np.nan) if keep else None
        r.lib.check(fn(r.h, None if ub is None else ub.ctypes.data, None if y is None else y.ctypes.data, T, 0, None))
        if wait:
            r.wait(check=False)
        return y
    ud = arrays.put(u)
    yd = arrays.empty((r.n, T, ny)) if keep else None
    r.lib.check(fn(r.h, arrays.ptr(ud), arrays.ptr(yd), T, 1, None))
    if wait:
        r.wait(check=False)
    r.reports()                 # (synchronises)
    return arrays.get(yd) if keep else None


def check_defining_property(lib, model, N, kinds, u_var, T, mem=0, keep=True, k=1, held=(), split=None, use_async=False,
                            measure=None, arrays=None, clock=0, more=0):
    """source_ref.check_defining_property with the rows armed by this module's apply_sources: two batches of ``model``, one with
    the sources ``kinds`` run through acme_batch_run_sources (in one call, in calls of ``split`` and T - split samples, or
    asynchronously), its twin through acme_batch_run on what acme_batch_render_sources wrote.  Outputs (when stored), state,
    report counters and measurement accumulators are compared with ==; both then advance ``more`` samples further the same
    way.  Returns the rendered u."""
    from acme_jl_amd.runner import ModelRunner
    arrays = arrays or sr.HostArrays()
    a, b = ModelRunner(model, N, lib=lib), ModelRunner(model, N, lib=lib)
    apply_sources(a, kinds)
    if clock:
        a.source_clock = clock
    if measure is None and not keep:
        measure = dict(f0=(441, 44100), harmonics=3)
    consts = [row for row, kd in enumerate(kinds) if kd is not None and kd["kind"] == "const"]
    for r in (a, b):
        if k > 1:           # (the twin holds the CONST rows explicitly: the library holds them whatever held_rows says)
            r.set_oversampling(k, held_rows=held if r is a else sorted(set(held) | set(consts)))
        if measure:
            r.set_measurement(**measure)
    L = lib.L
    ny = model.ny
    n_done = 0
    first = None
    for seg in ([T] if not more else [T, more]):
        uv = None if u_var is None else np.ascontiguousarray(u_var[:, n_done:n_done + seg])
        assert a.source_clock == clock + n_done
        u = a.render_sources(seg, uv)
        assert a.source_clock == clock + n_done, "render_sources must not advance the clock"
        y_ref = _call(b, L.acme_batch_run, u, seg, ny, mem, keep, arrays)
        cuts = [0, seg] if not split or n_done else [0, split, seg]
        ys = []
        for lo, hi in zip(cuts, cuts[1:]):
            part = None if uv is None else np.ascontiguousarray(uv[:, lo:hi])
            fn = L.acme_batch_run_sources_async if use_async else L.acme_batch_run_sources
            ys.append(_call(a, fn, part, hi - lo, ny, mem, keep, arrays, wait=use_async))
        n_done += seg
        assert a.source_clock == clock + n_done
        if keep:
            y = np.concatenate(ys, axis=1)
            assert not np.isnan(y_ref).any()
            assert np.array_equal(y, y_ref), ("y", np.argwhere(y != y_ref)[:4])
        for sa, sb, what in zip(a.get_state(), b.get_state(), "xpz"):
            assert np.array_equal(sa, sb), what
        ra, rb = a.report_arrays(), b.report_arrays()
        for key in ra:
            assert np.array_equal(ra[key], rb[key]), key
        if measure:
            (ma, ca), (mb, cb) = sr.raw_measurement(a), sr.raw_measurement(b)
            assert ca == cb == n_done
            assert np.array_equal(ma, mb, equal_nan=True), "measurement"
            assert np.isfinite(mb).all()
        if first is None:
            first = u
    return first


@functools.lru_cache(maxsize=None)
def property_cases(N=3):
    """(name, model, N, kinds): the diode clipper and superover with a GAUSSIAN row on the signal row (levels per instance) and
    CONST pots"""
    from helpers import HS, load
    g = noise("gaussian", amp=np.logspace(-1.5, -0.5, N), seed=5)
    pots = [dict(kind="const", offset=v) for v in ((np.arange(N) + 0.5) / N, np.full(N, 0.4), np.full(N, 0.7))]
    return [("diodeclipper", load("diodeclipper", HS), N, [g]), ("superover_var", load("superover_var", HS), N, [g] + pots)]


def layout_kinds(N, hold=3):
    """six rows whose first nu make the case of nu rows: noise rows of both distributions and three holds (1, ``hold``,
    4096 + 5), a caller's row and a TABLE row among them"""
    rng = np.random.default_rng(3)
    return [noise("gaussian", amp=rng.standard_normal(N), offset=rng.standard_normal(N), seed=9),
            noise("uniform", hold=hold, amp=rng.standard_normal(N), seed=9),
            None,
            dict(kind="table", table=rng.standard_normal(29), amp=rng.standard_normal(N)),
            noise("gaussian", hold=4096 + 5, stream=-np.arange(N)),
            noise("uniform", offset=rng.standard_normal(N))]


# ---- statistics ------------------------------------------------------------------------------------------------------------------
def standardised_statistics(a, b, var):
    """a, b [N, T]: rows 0 and 1 of N instances, draws of mean 0 and variance ``var`` (amp 1, offset 0).  The statistics of the
    issue, each divided by its standard error under independence.  Per row, pooled over its N T samples: the mean
    (se sqrt(var / (N T))), the variance about 0 (se sqrt((m4 - var^2) / (N T)), m4 = 9/5 var^2 for the uniform and 3 var^2
    for the Gaussian draw -- chosen by var) and the autocorrelation at lags 1, 2, 7 (the lagged products of every instance,
    se 1 / sqrt(N (T - lag))).  Per row the largest cross-correlation between two instances, and per instance the correlation
    of row 0 with row 1 (se 1 / sqrt(T) each).  Beside the pooled mean and variance, which dilute one instance that is off by
    sqrt(N), the same two per instance (se with T in place of N T).  The autocorrelation is not also taken per instance: the
    reference formulas themselves reach 4.71 there (stream 0, row 0, lag 2 at clock 0; it falls to 0.65 over four times the
    length: chance among 288 values, not structure).  Returns {name: largest magnitude}."""
    N, T = a.shape
    m4 = 3.0 * var * var if var == 1.0 else 9.0 / 5.0 * var * var
    out = {"mean": 0.0, "variance": 0.0, "autocorrelation": 0.0, "cross-correlation": 0.0, "row correlation": 0.0}
    for x in (a, b):
        out["mean"] = max(out["mean"], abs(x.mean() / np.sqrt(var / (N * T))))
        out["instance mean"] = max(out.get("instance mean", 0.0), np.abs(x.mean(axis=1) / np.sqrt(var / T)).max())
        out["instance variance"] = max(out.get("instance variance", 0.0), np.abs(((x * x).mean(axis=1) - var) / np.sqrt((m4 - var * var) / T)).max())
        out["variance"] = max(out["variance"], abs(((x * x).mean() - var) / np.sqrt((m4 - var * var) / (N * T))))
        for lag in (1, 2, 7):
            rho = (x[:, lag:] * x[:, :-lag]).sum() / (var * N * (T - lag))
            out["autocorrelation"] = max(out["autocorrelation"], abs(rho * np.sqrt(N * (T - lag))))
        c = x @ x.T / (var * T)
        out["cross-correlation"] = max(out["cross-correlation"], np.abs(c[~np.eye(N, dtype=bool)] * np.sqrt(T)).max())
    out["row correlation"] = np.abs((a * b).sum(axis=1) / (var * T) * np.sqrt(T)).max()
    return {k: float(v) for k, v in out.items()}
