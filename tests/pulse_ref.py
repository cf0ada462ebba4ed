"""Reference arithmetic for the PULSE and BURST rows (csrc/acme_source.h, acme_batch_set_source_pulse / _burst) that shares no
code with the library: the envelope's j in Python's unbounded integers, a ramp sample as ONE division of two exactly converted
integers, the pulse's value as an exactly evaluated fma; the burst against the SINE row rendered beside it where the envelope is
1, against its offset where it is 0, against mpmath within source_ref.sine_bound on the ramps.  Shared by test_pulse_sources.py
(CPU emulator) and test_gpu_pulse_sources.py (MI355X)."""
import functools

import numpy as np

import source_ref as sr
from exact_ref import fma_fast

PMAX = 2 ** 31 - 1


# ---- rows as the tests describe them ---------------------------------------------------------------------------------------------
def pulse(period, on, delay=0, rise=0, fall=0, amp=None, offset=None):
    """a PULSE row's description, next to source_ref's dicts of the other kinds"""
    return dict(kind="pulse", period=period, delay=delay, rise=rise, on=on, fall=fall, amp=amp, offset=offset)


def burst(period, on, f_den, f_num=None, phase=None, delay=0, rise=0, fall=0, amp=None, offset=None):
    return dict(pulse(period, on, delay, rise, fall, amp, offset), kind="burst", f_den=f_den, f_num=f_num, phase=phase)


def sine_of(k):
    """the SINE row with a BURST row's tone, amp and offset"""
    return dict(kind="sine", f_den=k["f_den"], f_num=k["f_num"], phase=k["phase"], amp=k["amp"], offset=k["offset"])


def shape(k, N):
    """the five integers per instance: a list of N tuples (P, delay, rise, on, fall) of Python integers"""
    cols = [[int(v) for v in sr.par(k[name], N, 0)] for name in ("period", "delay", "rise", "on", "fall")]
    return list(zip(*cols))


# ---- the envelope ------------------------------------------------------------------------------------------------------------------
def envelope_index(k, N, T, n0):
    """j = (n - delay_i) mod P_i for the clocks n0 ... n0 + T - 1: [N, T] int64, the clock's reduction in unbounded integers"""
    out = np.empty((N, T), dtype=np.int64)
    for i, (P, delay, _, _, _) in enumerate(shape(k, N)):
        j0 = (int(n0) - delay) % P                      # (Python's %: non-negative)
        out[i] = (j0 + np.arange(T, dtype=np.int64)) % P
    return out


def envelope(k, N, T, n0):
    """(e, j): e [N, T] exactly as the issue defines it -- the integers converted exactly (they are below 2^31), one correctly
    rounded division per ramp sample, 1.0 and 0.0 elsewhere"""
    j = envelope_index(k, N, T, n0)
    e = np.zeros((N, T))
    for i, (_, _, rise, on, fall) in enumerate(shape(k, N)):
        ji = j[i]
        up, flat, down = ji < rise, (ji >= rise) & (ji < rise + on), (ji >= rise + on) & (ji < rise + on + fall)
        e[i, flat] = 1.0
        if up.any():
            e[i, up] = ji[up].astype(np.float64) / float(rise)
        if down.any():
            e[i, down] = (rise + on + fall - ji[down]).astype(np.float64) / float(fall)
    return e, j


def pulse_row(k, N, T, n0):
    """[N, T]: every element of a PULSE row, fma(amp_i, e, offset_i) with one rounding (e = 1: the sum amp + offset, e = 0:
    the offset; both are what the fma gives, and one rounding each)"""
    amp, off = sr.par(k.get("amp"), N, 1.0), sr.par(k.get("offset"), N, 0.0)
    e, _ = envelope(k, N, T, n0)
    out = np.empty((N, T))
    for i in range(N):
        a, o = float(amp[i]), float(off[i])
        memo = {0.0: o + 0.0 * a, 1.0: a + o}
        row = out[i]
        for t, v in enumerate(e[i].tolist()):
            w = memo.get(v)
            if w is None:
                w = memo[v] = fma_fast(a, v, o)
            row[t] = w
    return out


def ramp_samples(k, N, T, n0):
    """per instance the window samples on a ramp with 0 < e < 1 (where the burst is neither the sine row nor the offset)"""
    e, _ = envelope(k, N, T, n0)
    return [np.flatnonzero((e[i] > 0.0) & (e[i] < 1.0)) for i in range(N)]


def check_burst_row(got, sine, k, N, T, n0, rng, edges=(), random=100):
    """got [N, T] of a BURST row, sine [N, T] of the SINE row with its tone rendered in the same batch: == the sine row wherever
    e = 1, == the offset wherever e = 0, both sets non-empty for every instance; on the ramps against mpmath within
    source_ref.sine_bound(g, offset) with g = amp e rounded once -- at each ramp run's first and last sample, at ``edges`` (slice
    and tile edges) where they are ramp samples, and at ``random`` random ramp samples.  Returns the worst ratio to the bound."""
    amp, off = sr.par(k.get("amp"), N, 1.0), sr.par(k.get("offset"), N, 0.0)
    fn, ph = sr.par(k.get("f_num"), N, 0), sr.par(k.get("phase"), N, 0)
    e, _ = envelope(k, N, T, n0)
    worst = 0.0
    for i in range(N):
        one, zero = e[i] == 1.0, e[i] == 0.0
        assert one.any() and zero.any(), (i, "the case must show both plateaus")
        assert np.array_equal(got[i, one], sine[i, one]), (i, np.flatnonzero(one & (got[i] != sine[i]))[:4])
        assert (got[i, zero] == off[i]).all(), (i, np.flatnonzero(zero & (got[i] != off[i]))[:4])
        ramp = np.flatnonzero(~one & ~zero)
        if len(ramp) == 0:
            continue
        cut = np.flatnonzero(np.diff(ramp) > 1)
        ends = set(ramp[np.r_[0, cut + 1]].tolist()) | set(ramp[np.r_[cut, len(ramp) - 1]].tolist())
        near = set(t for t in edges if 0 <= t < T and not one[t] and not zero[t])
        pick = sorted(ends | near | set(rng.choice(ramp, size=min(random, len(ramp)), replace=False).tolist()))
        for t in pick:
            g = float(amp[i]) * float(e[i, t])          # (one rounded product)
            err, bound = sr.sine_error(got[i, t], g, off[i], fn[i], ph[i], k["f_den"], n0 + t), sr.sine_bound(g, off[i])
            worst = max(worst, err / bound)
            assert err <= bound, (i, t, n0, float(got[i, t]), err / sr.U, bound / sr.U)
    return worst


# ---- arming --------------------------------------------------------------------------------------------------------------------------
def apply_sources(r, kinds):
    """arm ``kinds`` on a ModelRunner: PULSE and BURST rows with their keywords, NOISE rows through noise_ref, the others
    through source_ref"""
    import noise_ref as nr
    for row, k in enumerate(kinds):
        if k is None:
            continue
        if k["kind"] in ("pulse", "burst"):
            tone = dict(f_den=k["f_den"], f_num=k["f_num"], phase=k["phase"]) if k["kind"] == "burst" else {}
            r.set_source(row, k["kind"], amp=k.get("amp"), offset=k.get("offset"), period=k["period"], delay=k["delay"], rise=k["rise"],
                         on=k["on"], fall=k["fall"], **tone)
        else:
            nr.apply_sources(r, [None] * row + [k])
    return r


# ---- the defining property: a source run is acme_batch_run on the rendered u, bit for bit ------------------------------------------
def check_defining_property(lib, model, N, kinds, u_var, T, mem=0, keep=True, k=1, held=(), split=None, use_async=False,
                            measure=None, arrays=None, clock=0, more=0):
    """source_ref.check_defining_property with the rows armed by this module's apply_sources: two batches of ``model``, one with
    the sources ``kinds`` run through acme_batch_run_sources (in one call, in calls of ``split`` and T - split samples, or
    asynchronously), its twin through acme_batch_run on what acme_batch_render_sources wrote.  Outputs (when stored), state,
    report counters and measurement accumulators are compared with ==; both then advance ``more`` samples further the same
    way.  Returns the rendered u."""
    from acme_jl_amd.runner import ModelRunner
    from noise_ref import _call
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
def property_cases(N=3, scale=1, clock=0):
    """(name, model, N, kinds): the diode clipper and superover with a BURST on the signal row (levels, burst lengths and edges
    per instance) and the pots as one CONST, one PULSE ramp-and-hold (a step of P = 2^31 - 1 that starts 5 samples after
    ``clock`` and ramps over 50 ``scale`` samples), one CONST.  ``scale`` stretches the envelopes to the run's length (1: the
    emulator's runs of some 60 samples)"""
    from helpers import FS, HS, load
    s = scale
    b = burst(period=40 * s, on=np.array([9, 12, 15])[:N] * s, f_den=FS, f_num=(3000 + 700 * np.arange(N)) // s, phase=np.arange(N) * 100,
              delay=np.array([3, 0, 7])[:N] * s, rise=np.array([4, 0, 6])[:N] * s, fall=np.array([5, 3, 0])[:N] * s, amp=np.logspace(-1, 0.5, N))
    at = (clock + 5) % PMAX
    ramp = pulse(period=PMAX, on=PMAX - at - 50 * s, delay=at, rise=50 * s, amp=np.linspace(0.3, 0.5, N), offset=0.25)
    pots = [dict(kind="const", offset=(np.arange(N) + 0.5) / N), ramp, dict(kind="const", offset=np.full(N, 0.7))]
    return [("diodeclipper", load("diodeclipper", HS), N, [b]), ("superover_var", load("superover_var", HS), N, [b] + pots)]


# ---- the cases of the exact and the layout tests -----------------------------------------------------------------------------------
def exact_pulses(n0, T):
    """one PULSE row of 9 instances that differ in all five integers (the issue's periods and shapes) for a render of T samples
    from clock n0: P = 1 with on 0 and 1; P = 2; P = 97, 511, 513 (below and around a thread's stride of 512: the running j wraps
    on every step); P = 4099 (longer than a tile); P = 10007 (longer than a slice); P = 2^31 - 1 with its delay inside the run (the
    step).  Among them rise = fall = 1, on = 0 with ramps (a triangle), rise + on + fall = P (never low), all three zero (always
    the offset), a delay of P - 1; a negative amp and offset = -0.0"""
    step_at = (n0 + T // 3) % PMAX
    rows = [  # P, delay, rise, on, fall
        (1, 0, 0, 0, 0),                        # all three zero: always the offset
        (1, 0, 0, 1, 0),                        # always high
        (2, 1, 1, 1, 0),                        # delay P - 1; rise + on + fall = P: never low but at j = 0 of the ramp
        (97, 96, 1, 40, 1),                     # rise = fall = 1, delay P - 1
        (511, 17, 200, 0, 250),                 # a triangle
        (513, 500, 100, 313, 100),              # rise + on + fall = P
        (4099, 4000, 1500, 700, 1899),          # never low, longer than a tile
        (10007, 77, 3001, 2000, 4999),
        (PMAX, step_at, 1000, PMAX - step_at - 1000, 0)]      # the step with a ramp of 1000 samples
    cols = [np.array(c, dtype=np.int64) for c in zip(*rows)]
    amp = np.array([1.0, -2.5, 0.1, 1e-3, -7.0, 3.0, 0.3, 1.0 / 3.0, 1e3])
    off = np.array([0.5, -0.0, 1.0 / 3.0, -0.0, 2.0, -1e-3, 0.7, -0.1, 1.0])
    return pulse(period=cols[0], delay=cols[1], rise=cols[2], on=cols[3], fall=cols[4], amp=amp, offset=off)


def exact_bursts(N, n0, T):
    """one BURST row whose every instance shows both plateaus and both ramps inside a render of T samples from clock n0, with
    per-instance tones; periods around the stride, longer than a tile and the step"""
    rows = [(97, 5, 20, 30, 25), (513, 500, 100, 200, 100), (4099, 4000, 1500, 700, 1000), (PMAX, (n0 + 100) % PMAX, 3000, 2000, 2500),
            (2000, 0, 0, 1000, 0), (511, 17, 200, 0, 250), (1500, 3, 1, 700, 1)]
    rows = (rows * (N // len(rows) + 1))[:N]
    cols = [np.array(c, dtype=np.int64) for c in zip(*rows)]
    rng = np.random.default_rng(5)
    amp = rng.standard_normal(N) * 10.0 ** rng.integers(-2, 3, N)
    return burst(period=cols[0], delay=cols[1], rise=cols[2], on=cols[3], fall=cols[4], f_den=sr.PRIME_DEN,
                 f_num=sr.PRIME_DEN - 1 - 1000003 * np.arange(N), phase=12345 + 7 * np.arange(N), amp=amp, offset=rng.standard_normal(N))


def layout_kinds(N):
    """six rows whose first nu make the case of nu rows: pulse and burst rows with a caller's row, a TABLE row and a SINE row
    among them"""
    rng = np.random.default_rng(3)
    i = np.arange(N)
    return [pulse(period=97 + 100 * i, on=20 + i, delay=5 * i, rise=7 + i, fall=1 + 2 * i, amp=rng.standard_normal(N), offset=rng.standard_normal(N)),
            burst(period=513 + i, on=100, f_den=44100, f_num=1000 + 37 * i, phase=i, delay=500, rise=50 + i, fall=30, amp=rng.standard_normal(N)),
            None,
            dict(kind="table", table=rng.standard_normal(29), amp=rng.standard_normal(N)),
            dict(kind="sine", f_den=44100, f_num=1000 + 37 * i, phase=i, amp=rng.standard_normal(N), offset=rng.standard_normal(N)),
            pulse(period=4099, on=1000 + i, delay=4000 - i, rise=0, fall=0, offset=rng.standard_normal(N))]
