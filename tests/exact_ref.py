"""References for the resampling (csrc/acme_resample.h) and measurement (csrc/acme_measure.h) kernels that share no code
with the library: a pass-through model that makes the library transparent, the headers' sums as exactly evaluated fma
chains, the same sums in extended precision with their running error bounds, and twiddles from big-integer phase reduction
and mpmath.  Shared by test_exact_kernels.py (CPU emulator) and test_gpu_exact_kernels.py (MI355X).

Both headers state their arithmetic exactly -- every sum ONE chain of fma over ascending index starting from 0 --, so an
expected value can be computed here exactly, and a kernel that reads one wrong tap, sample, row or instance differs from it
by far more than a rounding."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53          # unit roundoff of a double


# ---- the transparent model --------------------------------------------------------------------------------------------------
def wire_model(channels, fs):
    """``channels`` times a voltage source into a voltage probe and nothing else: nx = nn = 0 and y = u, so an oversampled
    run of it is decimate(interpolate(u)) and a measured run measures the data the test chose."""
    from acme_jl_amd.circuit import voltageprobe, voltagesource
    from acme_jl_amd.examples import build
    from acme_jl_amd.model import DiscreteModel
    els = []
    for c in range(channels):
        els.append((f"in{c}", voltagesource(), {"-": "gnd"}))
        els.append((f"out{c}", voltageprobe(), {"+": (f"in{c}", "+"), "-": "gnd"}))
    return DiscreteModel(build(els), Fraction(1, fs), "HomotopySolver{SimpleSolver}")


def scaled_rows(rng, N, T, rows):
    """random data [N, T, rows] whose scale is spread over 1e-3 ... 1e3 across instances and rows but uniform within a
    row: one lost or shifted sample is then far above the rounding of its row's sums"""
    return rng.standard_normal((N, T, rows)) * 10.0 ** rng.integers(-3, 4, (N, 1, rows))


# ---- fma ----------------------------------------------------------------------------------------------------------------------
def fma(a, b, c):
    """a b + c with ONE rounding (the definition; Python 3.10 has no math.fma)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def fma_fast(a, b, c):
    """``fma`` for finite doubles without Fraction's gcds (six times as fast): every denominator of as_integer_ratio is a
    power of two, so a b + c is one integer over one power of two, and int / int is correctly rounded.
    test_exact_kernels.py holds it to ``fma`` bit for bit."""
    an, ad = a.as_integer_ratio()
    bn, bd = b.as_integer_ratio()
    cn, cd = c.as_integer_ratio()
    d = ad * bd
    if cd >= d:
        return (an * bn * (cd // d) + cn) / cd
    return (an * bn + cn * (d // cd)) / d


def chain(taps, vals):
    """sum of taps[j] vals[j] as one fma chain over ascending j starting from 0"""
    acc = 0.0
    for t, v in zip(taps, vals):
        acc = fma_fast(t, v, acc)
    return acc


# ---- resampler: the header's formulas as exact chains ------------------------------------------------------------------------
def scaled_up_taps(k, up):
    """g = k h_up as the library forms it: one rounded product per tap"""
    return float(k) * np.asarray(up, dtype=np.float64)


def chain_interp(u, k, g, held, positions):
    """u [N, T, nu] at the base rate -> the model-rate input rows at ``positions`` [(instance, model-rate sample m)], as
    [len(positions), nu]:  u_os[m] = sum_{j < Lu} g[j] s[m - j] with s[m] = u[m / k] where k divides m and 0 elsewhere, so
    with m = t k + p the terms that remain are g[p + k q] u[t - q] in ascending q; held rows: u[m // k].  A sample before
    the first is the first."""
    g = [float(v) for v in g]
    nu = u.shape[2]
    out = np.empty((len(positions), nu))
    for n, (i, m) in enumerate(positions):
        t, p = divmod(m, k)
        for r in range(nu):
            if r in held:
                out[n, r] = u[i, t, r]
                continue
            taps = g[p::k]
            out[n, r] = chain(taps, [float(u[i, max(t - q, 0), r]) for q in range(len(taps))])
    return out


class LazyInterp:
    """chain_interp on demand: ``self[i, m]`` is the model-rate row [nu] of instance i at sample m (computed once)"""

    def __init__(self, u, k, g, held):
        self.args, self.memo = (u, k, g, tuple(held)), {}

    def __getitem__(self, im):
        if im not in self.memo:
            self.memo[im] = chain_interp(*self.args, [im])[0]
        return self.memo[im]


def chain_decim(y_os, k, h, positions):
    """y_os[i, m] -> the model-rate output row [ny] (an array [N, k T, ny] or a LazyInterp) -> the base-rate outputs at
    ``positions`` [(instance, base-rate sample n)], as [len(positions), ny]:  y[n] = sum_{j < Ld} h[j] y_os[n k + k - 1 - j]
    in ascending j.  A sample before the first is the first."""
    h = [float(v) for v in h]
    out = None
    for n, (i, t) in enumerate(positions):
        rows = [y_os[i, max(t * k + k - 1 - j, 0)] for j in range(len(h))]
        if out is None:
            out = np.empty((len(positions), len(rows[0])))
        for r in range(out.shape[1]):
            out[n, r] = chain(h, [float(v[r]) for v in rows])
    return out


def chain_resample(u, k, g, h, held):
    """the whole of decimate(interpolate(u)) as exact chains, [N, T, nu] (small cases only)"""
    N, T, nu = u.shape
    u_os = chain_interp(u, k, g, held, [(i, m) for i in range(N) for m in range(k * T)]).reshape(N, k * T, nu)
    return chain_decim(u_os, k, h, [(i, t) for i in range(N) for t in range(T)]).reshape(N, T, nu)


# ---- resampler: extended precision and its error bound -----------------------------------------------------------------------
def _ld_compose(u, k, g, h, held):
    """decimate(interpolate(u)) in np.longdouble, vectorised over instances, samples and rows (one pass per tap)"""
    N, T, nu = u.shape
    g, h = np.asarray(g, dtype=np.longdouble), np.asarray(h, dtype=np.longdouble)
    lu, ld = len(g), len(h)
    du = (lu - 1) // k
    ext = np.concatenate([np.repeat(u[:, :1], du, axis=1), u], axis=1).astype(np.longdouble)
    u_os = np.zeros((N, T, k, nu), dtype=np.longdouble)
    for p in range(k):
        for q, j in enumerate(range(p, lu, k)):
            u_os[:, :, p] += g[j] * ext[:, du - q:du - q + T]
    for r in held:
        u_os[:, :, :, r] = u[:, :, None, r]
    u_os = u_os.reshape(N, k * T, nu)
    ext = np.concatenate([np.repeat(u_os[:, :1], ld - 1, axis=1), u_os], axis=1)
    y = np.zeros((N, T, nu), dtype=np.longdouble)
    for j in range(ld):
        y += h[j] * ext[:, ld - 1 + k - 1 - j::k][:, :T]
    return y


def ld_resample(u, k, g, h, held):
    """decimate(interpolate(u)) with the header's formulas in np.longdouble [N, T, nu]"""
    return _ld_compose(u, k, g, h, held)


def ld_bound(u, k, g, h, held):
    """Bound on |library - ld_resample| at every element: the same composition applied to |g|, |h|, |u|, times
    (ceil(Lu / k) + Ld + 2) 2^-53.  The standard bound for two stacked fma chains: an interpolated sample is a chain of at
    most ceil(Lu / k) terms, off by at most ceil(Lu / k) 2^-53 sum |g| |u|; the decimation chain of Ld terms adds at most
    Ld 2^-53 sum |h| |y_os| and carries its inputs' errors with weights |h|; the 2 covers the second-order terms and the
    extended-precision reference's own rounding (2^-64 per operation).  Derived, not measured."""
    terms = -(-len(g) // k) + len(h) + 2
    return terms * U * _ld_compose(np.abs(u), k, np.abs(g), np.abs(h), held)


# ---- measurement: twiddles ----------------------------------------------------------------------------------------------------
_TW = {}        # (reduced phase, f_den) -> (cos hi, cos lo, sin hi, sin lo)


def _twiddle(kk, f_den):
    """cos / sin of 2 pi kk / f_den, 0 <= kk < f_den, each as an unevaluated sum hi + lo of doubles (106 bits), from mpmath
    at 120 bits.  Cached by the phase folded into the first half turn (cos is even, sin odd about it)."""
    import mpmath
    fold = min(kk, f_den - kk)
    key = (fold, f_den)
    if key not in _TW:
        with mpmath.workprec(120):
            c, s = mpmath.cos_sin(2 * mpmath.pi * mpmath.mpf(fold) / f_den)
            ch, sh = float(c), float(s)
            _TW[key] = (ch, float(c - ch), sh, float(s - sh))
    ch, cl, sh, sl = _TW[key]
    return (ch, cl, sh, sl) if fold == kk else (ch, cl, -sh, -sl)


def exact_twiddles(f_num, f_den, H, n):
    """cos / sin [H, n] of 2 pi ((h f_num m) mod f_den) / f_den, h = 1 ... H, m = 0 ... n - 1 as np.longdouble (hi + lo:
    good to the format's 2^-64): the phase reduced in Python's unbounded integers, no int64 anywhere"""
    c, s = np.empty((H, n), dtype=np.longdouble), np.empty((H, n), dtype=np.longdouble)
    for h in range(1, H + 1):
        for m in range(n):
            ch, cl, sh, sl = _twiddle((h * f_num * m) % f_den, f_den)
            c[h - 1, m] = np.longdouble(ch) + np.longdouble(cl)
            s[h - 1, m] = np.longdouble(sh) + np.longdouble(sl)
    return c, s


# ---- measurement: moments and harmonics --------------------------------------------------------------------------------------
def exact_moments(seg):
    """seg [N, n, rows], the window's samples -> (sum, sq, min, max), each [N, rows], as the header forms them:
    sum the plain left-to-right double sum, sq = fma(y, y, sq) as the exact chain, min / max with the NaN rule (a NaN
    replaces the accumulator, and nothing replaces a NaN: both comparisons with it are false)"""
    N, n, rows = seg.shape
    s = np.zeros((N, rows))
    for t in range(n):
        s = s + seg[:, t]                      # (elementwise double additions in sample order)
    sq, mn, mx = np.zeros((N, rows)), np.full((N, rows), np.inf), np.full((N, rows), -np.inf)
    for i in range(N):
        for r in range(rows):
            q, lo, hi = 0.0, math.inf, -math.inf
            for v in seg[i, :, r].tolist():
                q = fma_fast(v, v, q) if math.isfinite(v) and math.isfinite(q) else v * v + q
                if v < lo or v != v:
                    lo = v
                if v > hi or v != v:
                    hi = v
            sq[i, r], mn[i, r], mx[i, r] = q, lo, hi
    return s, sq, mn, mx


def reported(acc, count):
    """what acme_batch_get_measurement reports from the accumulators sum and sq: mean = sum inv, rms = sqrt(sq inv) with
    inv = 1 / count rounded once (include/acme_hip.h)"""
    inv = 1.0 / float(count)
    return acc[0] * inv, np.sqrt(acc[1] * inv)


def ld_harmonics(seg, f0, H):
    """(C [N, rows, H], S [N, rows, H], l1 [N, rows]): C_h = sum y cos th, S_h = sum y sin th over the window in
    np.longdouble with exact_twiddles, and sum |y|"""
    c, s = exact_twiddles(f0[0], f0[1], H, seg.shape[1])
    x = seg.astype(np.longdouble)
    return np.einsum("itr,ht->irh", x, c), np.einsum("itr,ht->irh", x, s), np.abs(x).sum(axis=1)


def harmonic_bound(n, l1):
    """Bound on |C_h - ld_harmonics| and |S_h - ld_harmonics| for a window of n samples: (n + 16) 2^-53 sum |y_t|.
    n: the fma chain, each of its n roundings at most 2^-53 of a partial sum that sum |y_t| bounds.  16, in units of
    2^-53 |y_t| per term: the angle's two roundings (the quotient k / f_den and its product with 2 pi, at |th| <= pi: pi
    each) and the rounding of the constant 2 pi (0.35 units relative: 1.1) make 7.4; cos / sin of the rounded angle 4, which
    allows 4 ulp of a value below 1 (glibc states 1 ulp for both; the HIP documentation installed with the toolchain
    states no figure for the device's double cos / sin, so none replaces the 16); the report's scaling (1 / count and the
    product with it, undone here in extended precision) 2 of |C_h| <= sum |y_t|: 13.4 in all."""
    return (n + 16) * U * l1


def unscale(out, count):
    """acme_batch_get_measurement's A_h = (2 / count) (C_h - j S_h) [N, rows, 4 + 2H] -> (C_h, S_h) in np.longdouble"""
    o = out.astype(np.longdouble)
    return o[:, :, 4::2] * count / 2, -o[:, :, 5::2] * count / 2
