"""Reference arithmetic for the sources (csrc/acme_source.h, acme_batch_set_source_*) that shares no code with the library:
the phase in Python's unbounded integers, the sine from mpmath at that exact phase, CONST and TABLE rows as exactly evaluated
fma.  Shared by test_sources.py (CPU emulator) and test_gpu_sources.py (MI355X)."""
import numpy as np

from exact_ref import U, fma_fast, wire_model  # noqa: F401  (wire_model: re-exported for the tests)

PRIME_DEN = 2 ** 31 - 1          # a prime (Mersenne), the largest f_den the interface takes
CLOCKS = (0, 2 ** 31 - 1, 2 ** 31 + 1, 2 ** 40, 2 ** 62)


def kappa(f_num, phase, f_den, n):
    """(f_num n + phase) mod f_den taken to (-f_den / 2, f_den / 2], in unbounded integers"""
    k = (int(f_num) * int(n) + int(phase)) % int(f_den)
    return k - int(f_den) if 2 * k > f_den else k


def exact_sine(f_num, phase, f_den, n):
    """sin(2 pi kappa / f_den) at the exact kappa, an mpmath number of 120 bits"""
    import mpmath
    with mpmath.workprec(120):
        return mpmath.sin(2 * mpmath.pi * mpmath.mpf(kappa(f_num, phase, f_den, n)) / int(f_den))


def sine_bound(amp, offset):
    """Bound on |rendered - fma(amp, exact sine, offset) evaluated exactly| for one SINE element:
    (12 |amp| + |amp| + |offset|) 2^-53.  The angle's two roundings and the constant 2 pi: 7.4 units of 2^-53 at |th| <= pi,
    which sin (slope at most 1) carries to its value; the device's sin of the rounded angle: 4 units (the allowance of
    exact_ref.harmonic_bound, for the same reason); rounded up to 12 |amp|.  The final fma: one rounding of a result of at most
    |amp| + |offset|.  Derived, not measured."""
    return (12.0 * abs(amp) + abs(amp) + abs(offset)) * U


def sine_error(got, amp, offset, f_num, phase, f_den, n):
    """|got - (amp sin(2 pi kappa / f_den) + offset)| with the right-hand side at 120 bits, as a float"""
    import mpmath
    with mpmath.workprec(120):
        want = mpmath.mpf(float(amp)) * exact_sine(f_num, phase, f_den, n) + mpmath.mpf(float(offset))
        return float(abs(mpmath.mpf(float(got)) - want))


def exact_table_value(amp, offset, w, n):
    """fma(amp, w[n mod P], offset) with one rounding"""
    return fma_fast(float(amp), float(w[int(n) % len(w)]), float(offset))


def expected_rows(kinds, N, T, n0):
    """[N, T, len(kinds)] of exact values for CONST / TABLE rows (NaN for the others) and the list of (row, spec) of the SINE
    rows; ``kinds``: per row None (caller's row) or a dict(kind=..., amp, offset, f_den, f_num, phase, table) with per-instance
    arrays (or None = default)"""
    out = np.full((N, T, len(kinds)), np.nan)
    for r, k in enumerate(kinds):
        if k is None or k["kind"] == "sine":
            continue
        amp, off = par(k.get("amp"), N, 1.0), par(k.get("offset"), N, 0.0)
        for i in range(N):
            if k["kind"] == "const":
                out[i, :, r] = off[i]
            else:
                w = np.asarray(k["table"], dtype=np.float64)
                out[i, :, r] = [exact_table_value(amp[i], off[i], w, n0 + t) for t in range(T)]
    return out


def par(a, N, default):
    return np.full(N, default) if a is None else np.broadcast_to(np.asarray(a), (N,))


def check_sine_row(got, k, N, n0, samples):
    """got [N, T] against mpmath at the exact phase for the (instance, sample) pairs of ``samples``; returns the worst
    error in units of its bound (asserts it is at most 1)"""
    amp, off = par(k.get("amp"), N, 1.0), par(k.get("offset"), N, 0.0)
    fn, ph = par(k.get("f_num"), N, 0), par(k.get("phase"), N, 0)
    worst = 0.0
    for i, t in samples:
        err, bound = sine_error(got[i, t], amp[i], off[i], fn[i], ph[i], k["f_den"], n0 + t), sine_bound(amp[i], off[i])
        worst = max(worst, err / bound)
        assert err <= bound, (i, t, n0, float(got[i, t]), err / U, bound / U)
    return worst


def apply_sources(r, kinds):
    """arm ``kinds`` (as expected_rows takes them) on a ModelRunner"""
    for row, k in enumerate(kinds):
        if k is not None:
            r.set_source(row, k["kind"], amp=k.get("amp"), offset=k.get("offset"), f_den=k.get("f_den"), f_num=k.get("f_num"),
                         phase=k.get("phase"), table=k.get("table"))
    return r


# ---- the defining property: a source run is acme_batch_run on the rendered u, bit for bit --------------------------------------
class HostArrays:
    """"device memory" of the CPU emulator: host arrays.  test_gpu_sources.py has the same four calls over torch tensors."""

    def put(self, a):
        return None if a is None else np.ascontiguousarray(a)

    def empty(self, shape):
        return np.full(shape, np.nan)

    def ptr(self, a):
        return None if a is None else a.ctypes.data

    def get(self, a):
        return a


def raw_measurement(r):
    import ctypes as C
    from acme_jl_amd.runner import _dp
    H, rows = r._meas
    out = np.empty((r.n, len(rows), 4 + 2 * H))
    count = C.c_longlong(0)
    r.lib.check(r.lib.L.acme_batch_get_measurement(r.h, _dp(out), C.byref(count)))
    return out, count.value


def _call(r, fn, u, T, ny, mem, keep, arrays, wait=False):
    """one run entry point of the C ABI (fn: acme_batch_run, _run_sources, _run_sources_async) on host or "device" arrays;
    returns y [N, T, ny] or None"""
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
    """Two batches of ``model``: one with the sources ``kinds`` run through acme_batch_run_sources (in one call, or in calls of
    ``split`` and T - split samples, or asynchronously), its twin through acme_batch_run on what acme_batch_render_sources
    wrote.  Outputs (when stored), state, reports and measurement (armed when ``measure`` is given or y is not stored) are
    compared with ==; on an oversampled batch (factor ``k``, ``held`` rows) the twin also holds the CONST rows, as the library
    does by itself; then both advance ``more`` samples further the same way, which the histories of an oversampled batch
    and the carried clock must survive.  Returns the rendered u."""
    from acme_jl_amd.runner import ModelRunner
    arrays = arrays or HostArrays()
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
            (ma, ca), (mb, cb) = raw_measurement(a), raw_measurement(b)
            assert ca == cb == n_done
            assert np.array_equal(ma, mb, equal_nan=True), "measurement"
            assert np.isfinite(mb).all()
        if n_done == T:
            first = u
    return first
