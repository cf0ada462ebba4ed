"""Shared by the emulator and GPU tests of the measurement histogram (acme_batch_set_measurement_histogram): the reference
every histogram is held to -- numpy on the stored y of an identical run without a histogram, the contract's rule with the
difference and the product as two separate float64 operations and the scale the getter hands back -- and the checks, each
taking ``mk(model, n)``, which makes a fresh runner on the library under test (the emulator's or the GPU's).  Every comparison
is equality of integer arrays; every read also asserts that the B + 3 counters of each pair sum to ``count``."""
import ctypes as C
import functools

import numpy as np
import pytest

import exact_ref as X
import source_ref as sr
from helpers import FS, HS
from test_measurement import clipper, raw, two_output_clipper

CAP = 268435456             # ACME_MAX_HISTOGRAM
MAX_BINS = 4096             # ACME_MAX_HIST_BINS
START, LENGTH = 3, 4096 + 777               # the geometry's window: a chunk boundary inside, a length that is no multiple of 64
T_GEO = START + LENGTH + 24
BINS = [1, 2, 63, 64, 65, 1000, 4096]
SIGNALS = ["constant", "alternating", "sine", "noise", "missed ranges"]


# ---- the reference ------------------------------------------------------------------------------------------------------------
def rule(v, lo, hi, s, B, mode="signed"):
    """the contract for ONE sample in Python floats: the counter 0 ... B + 2 (UNDER, BIN[0 ... B - 1], OVER, NAN)"""
    x = abs(v) if mode == "abs" else v
    if x != x:
        return B + 2
    if x < lo:
        return 0
    if x >= hi:
        return B + 1
    t = x - lo
    q = t * s
    return min(int(q), B - 1) + 1


def replay(yw, lo, hi, s, B, mode="signed"):
    """the contract on the window's samples so far yw [N, count, nrows]: the counters [N, nrows, B + 3]"""
    N, count, nrows = yw.shape
    x = np.abs(yw) if mode == "abs" else yw
    lo_, hi_, s_ = (np.asarray(a, dtype=np.float64)[:, None, None] for a in (lo, hi, s))
    with np.errstate(invalid="ignore", over="ignore"):
        t = x - lo_                                         # (two operations, each rounded on its own)
        q = t * s_
        inside = (x >= lo_) & (x < hi_)
        k = np.minimum(np.trunc(np.where(inside, q, 0.0)).astype(np.int64), B - 1)
        slot = np.where(x != x, B + 2, np.where(x < lo_, 0, np.where(x >= hi_, B + 1, k + 1)))
    pair = (np.arange(N)[:, None, None] * nrows + np.arange(nrows)[None, None, :]) * (B + 3)
    return np.bincount((pair + slot).ravel(), minlength=N * nrows * (B + 3)).reshape(N, nrows, B + 3).astype(np.int64)


def got(r):
    """the getter's arrays through ``measurement_histogram()``: (counters [N, nrows, B + 3], count, lo, hi, scale); asserts
    the sum of every pair's counters and the scale's two roundings"""
    h = r.measurement_histogram()
    full = np.concatenate([h.under[..., None], h.counts, h.over[..., None], h.nan[..., None]], axis=-1)
    assert full.dtype == np.int64 and (full >= 0).all()
    assert (full.sum(axis=-1) == h.count).all(), (full.sum(axis=-1), h.count)
    assert np.array_equal(h.scale, np.float64(h.bins) / (h.hi - h.lo))     # d = hi - lo; s = B / d
    return full, h.count, h.lo, h.hi, h.scale


def assert_histogram(r, yw, B, mode, what=""):
    full, count, lo, hi, s = got(r)
    assert count == yw.shape[1], (what, count, yw.shape)
    want = replay(yw, lo, hi, s, B, mode)
    assert full.shape == want.shape, (what, full.shape, want.shape)
    assert np.array_equal(full, want), (what, np.argwhere(full != want)[:6])
    return full


def window(y, start, length, rows=None):
    """the measured samples of the stored y [N, T, ny]: [N, count, nrows]"""
    stop = y.shape[1] if not length else min(y.shape[1], start + length)
    return y[:, start:stop][:, :, list(range(y.shape[2])) if rows is None else rows]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(a.view(np.int64) == b.view(np.int64)))


# ---- 1. exact pins ------------------------------------------------------------------------------------------------------------
def below(x):
    return float(np.nextafter(x, -np.inf))


TINY = 5e-324               # the smallest subnormal
FINITE = [-1.0, below(-1.0), 1.0, below(1.0), 0.0, -0.0, TINY, -TINY, -0.5, below(-0.5), 0.7, below(0.7), below(-0.7), 0.25, -0.25,
          2.0, -2.0]
# (bins, lo, hi, mode) -> {value: counter}: what the contract's edge cases say, written out by hand
PINS = [
    (3, -1.0, 1.0, "signed", {-1.0: 1, below(-1.0): 0, 1.0: 4, below(1.0): 3, 0.0: 2, -0.0: 2, 2.0: 4, -2.0: 0,
                              np.inf: 4, -np.inf: 0}),
    (3, -1.0, 1.0, "abs", {-1.0: 4, below(-1.0): 4, 1.0: 4, below(1.0): 3, 0.0: 2, -0.0: 2, -2.0: 4, np.inf: 4, -np.inf: 4}),
    (4, -1.0, 1.0, "signed", {-0.5: 2, below(-0.5): 1, 0.0: 3, -0.0: 3, -1.0: 1}),      # an interior edge: x == lo + 1 / s
    (8, 0.0, 1.0, "signed", {0.0: 1, -0.0: 1, TINY: 1, -TINY: 0, 1.0: 9, below(1.0): 8, 0.25: 3, -0.25: 0}),
    (8, 0.0, 1.0, "abs", {0.0: 1, -0.0: 1, TINY: 1, -TINY: 1, -0.25: 3, -0.5: 5, -1.0: 9}),
    (7, -0.7, 0.7, "signed", {below(0.7): 7, 0.7: 8, -0.7: 1, below(-0.7): 0}),
    (10, -0.7, 0.7, "signed", {below(0.7): 10, 0.7: 11, -0.7: 1, below(-0.7): 0}),
]


def check_exact_pins(mk):
    """y = u through the pass-through model.  Instance 0 and 4 carry the finite pins sample after sample, instances 1, 2, 3
    are +inf, -inf and NaN throughout (a non-finite instance of its own, so that the finite ones stay what they are)"""
    # the clamp case, in numpy as the issue states it: just below hi the product rounds up to B
    for B, lo, hi in ((3, -1.0, 1.0), (7, -0.7, 0.7), (10, -0.7, 0.7)):
        s = np.float64(B) / (np.float64(hi) - np.float64(lo))
        assert (np.float64(below(hi)) - np.float64(lo)) * s == float(B), (B, lo, hi)
    T = len(FINITE)
    u = np.zeros((5, T, 1))
    u[0, :, 0] = u[4, :, 0] = FINITE
    u[1], u[2], u[3] = np.inf, -np.inf, np.nan
    for B, lo, hi, mode, pins in PINS:
        r = mk(X.wire_model(1, FS), 5).set_measurement().set_measurement_histogram(B, lo, hi, mode)
        y = r.run(u, time_major=True, check=False)
        # (the model's y = 0.0 + u reads -0.0 as +0.0, and an instance is NaN from the sample after its first non-finite
        # one on: the infinities are ONE sample each, the first)
        assert np.array_equal(y[[0, 4]], u[[0, 4]]) and same_bits(np.delete(y[0], 5, axis=0), np.delete(u[0], 5, axis=0))
        assert y[1, 0, 0] == np.inf and y[2, 0, 0] == -np.inf and np.isnan(y[3]).all()
        n_inf = [0, int((y[1] == np.inf).sum()), int((y[2] == -np.inf).sum())]
        assert np.isnan(y[1, n_inf[1]:]).all() and np.isnan(y[2, n_inf[2]:]).all()
        full = assert_histogram(r, y, B, mode, (B, lo, hi, mode))
        _, count, glo, ghi, gs = got(r)
        assert count == T and (glo == lo).all() and (ghi == hi).all() and (gs == B / (hi - lo)).all()
        want = np.zeros(B + 3, dtype=np.int64)
        for v in FINITE:
            want[rule(v, lo, hi, float(gs[0]), B, mode)] += 1
        assert np.array_equal(full[0, 0], want) and np.array_equal(full[4, 0], want), (B, lo, hi, mode, full[0, 0], want)
        for v, slot in pins.items():
            assert rule(v, lo, hi, float(gs[0]), B, mode) == slot, (B, lo, hi, mode, v, slot)
            if np.isinf(v):
                i = 1 if v > 0 else 2
                one = np.zeros(B + 3, dtype=np.int64)
                one[slot], one[B + 2] = n_inf[i], T - n_inf[i]
                assert np.array_equal(full[i, 0], one), (B, mode, v, full[i, 0])
        nan = np.zeros(B + 3, dtype=np.int64)
        nan[B + 2] = T
        assert np.array_equal(full[3, 0], nan)
    # -0.0 with lo = 0 is bin 0: by the rule itself, and through the library whichever zero the model hands on
    assert rule(-0.0, 0.0, 1.0, 8.0, 8) == 1 and replay(np.full((1, 3, 1), -0.0), [0.0], [1.0], [8.0], 8)[0, 0].tolist() == [0, 3] + [0] * 9
    r = mk(X.wire_model(1, FS), 1).set_measurement().set_measurement_histogram(8, 0.0, 1.0)
    r.measure(np.full((1, 70, 1), -0.0), time_major=True)
    assert got(r)[0][0, 0].tolist() == [0, 70] + [0] * 9
    # every pinned value as a run of its own: T samples of it land in exactly the pinned counter
    for B, lo, hi, mode, pins in PINS:
        vals = [v for v in pins if np.isfinite(v)]
        uu = np.ascontiguousarray(np.broadcast_to(np.array(vals)[:, None, None], (len(vals), 70, 1)))
        r = mk(X.wire_model(1, FS), len(vals)).set_measurement().set_measurement_histogram(B, lo, hi, mode)
        r.measure(uu, time_major=True)
        full = got(r)[0]
        for i, v in enumerate(vals):
            one = np.zeros(B + 3, dtype=np.int64)
            one[pins[v]] = 70
            assert np.array_equal(full[i, 0], one), (B, lo, hi, mode, v, pins[v], np.flatnonzero(full[i, 0]))


# ---- 2. geometry, 3. rows -----------------------------------------------------------------------------------------------------
def signal(mk, name, N, T):
    """(u [N, T, 1], lo, hi): scalars, or the per-instance arrays of "missed ranges" """
    t = np.arange(T)
    amp = np.linspace(0.05, 1.3, N)[:, None]                # (beyond the range 1 from 0.77 N on: UNDER and OVER fill)
    if name == "constant":
        u = np.broadcast_to(amp * np.where(np.arange(N) % 2 == 0, 1.0, -1.0)[:, None], (N, T))
    elif name == "alternating":
        u = np.where(t[None] % 2 == 0, amp, -0.37 * amp)
    elif name in ("sine", "missed ranges"):
        u = amp * np.sin(2 * np.pi * 997.0 / FS * t)[None]
    elif name == "noise":
        r = mk(X.wire_model(1, FS), N)
        r.set_source(0, "noise", amp=amp[:, 0], dist="uniform", hold=1, seed=11)
        u = r.render_sources(T)[:, :, 0]
    else:
        raise KeyError(name)
    u = np.ascontiguousarray(np.asarray(u, dtype=np.float64)[:, :, None])
    if name != "missed ranges":
        return u, -1.0, 1.0
    # i mod 3 == 0: the instance's own span; 1: a range above every sample (all UNDER); 2: one below (all OVER)
    k = np.arange(N) % 3
    lo = np.where(k == 0, -amp[:, 0], np.where(k == 1, 10.0, -11.0))
    hi = np.where(k == 0, amp[:, 0], np.where(k == 1, 11.0, -10.0))
    return u, lo, hi


@functools.lru_cache(maxsize=None)
def _plain_run(mk, name, two, N, T, start, length, rows):
    """the run without a histogram every case of a shape shares: (model, u, lo, hi, y, raw measurement); never modified"""
    m = two_output_clipper() if two else X.wire_model(1, FS)
    u, lo, hi = signal(mk, name, N, T)
    r = mk(m, N).set_measurement(start=start, length=length, rows=None if rows is None else list(rows))
    y = r.run(u, time_major=True)
    return m, u, lo, hi, y, raw(r)


def check_geometry(mk, N, B, name, T=T_GEO, start=START, length=LENGTH, rows=None, two=False, cuts=(2000, 4100),
                   modes=("signed", "abs")):
    """one call over the whole run in each of ``modes``, then three split calls with the counters after each"""
    m, u, lo, hi, y, plain = _plain_run(mk, name, two, N, T, start, length, None if rows is None else tuple(rows))
    arm = lambda mode: mk(m, N).set_measurement(start=start, length=length, rows=rows).set_measurement_histogram(B, lo, hi, mode)
    whole = {}
    for mode in modes:
        r = arm(mode)
        r.measure(u, time_major=True)
        with_hist = raw(r)
        assert with_hist[1] == plain[1] and np.array_equal(with_hist[0], plain[0])      # the measurement's own results
        whole[mode] = assert_histogram(r, window(y, start, length, rows), B, mode, f"one call, {mode}")
    if name == "constant" and not two:                      # every sample of a pair in ONE counter
        assert all(((w == length).sum(axis=-1) == 1).all() and ((w != 0).sum(axis=-1) == 1).all() for w in whole.values())
    if name == "missed ranges" and not two and "signed" in whole:
        k = np.arange(N) % 3
        assert (whole["signed"][k == 1, :, 0] == length).all() and (whole["signed"][k == 2, :, B + 1] == length).all()
        assert not whole["signed"][k == 0, :, 0].any() and not whole["signed"][:, :, B + 2].any()   # (|u| <= amp: none below -amp)
    r = arm(modes[0])
    edges = [0, *cuts, T]
    for a, b in zip(edges[:-1], edges[1:]):
        r.measure(np.ascontiguousarray(u[:, a:b]), time_major=True)
        assert_histogram(r, window(y[:, :b], start, length, rows), B, modes[0], f"calls up to {b}")
    assert np.array_equal(got(r)[0], whole[modes[0]])


# ---- 4. paths -----------------------------------------------------------------------------------------------------------------
SOS = np.array([[0.5, 0.25, 0.125, -0.3, 0.1], [1.0, -1.0, 0.0, -0.995, 0.0]])


def check_paths(mk, dev, k, T, monkeypatch, B, mode="signed", weighted=False, N=70, S=3, length=None):
    """the pass-through model driven by what a per-instance sine source renders, oversampled by k: the counters read after
    every path == those after a host run with y stored == the replay (``weighted``: of ``MeasurementWeighting.apply`` on the
    stored y).  ``dev``: the device-memory calls (put, run(r, u, keep, T))"""
    from acme_jl_amd.runner import MeasurementWeighting
    m = X.wire_model(1, k * FS)
    amp = np.logspace(-2, 0.7, N)
    src = dict(kind="sine", f_den=441, f_num=1 + np.arange(N) % 40, amp=amp, phase=np.arange(N) % 441)
    length = T - 100 if length is None else length
    lo, hi = (np.zeros(N), 0.9 * amp) if mode == "abs" else (-0.9 * amp, 0.8 * amp)     # a range per instance: the level's

    def fresh(sourced=False, pi=False):
        r = mk(m, N).set_oversampling(k)
        if sourced:
            r = sr.apply_sources(r, [src])
        if pi:      # (the per-instance form: its table's budget sets the chunk length)
            r.set_measurement(start=S, length=length, f_den=441, f_num=1 + np.arange(N), harmonics=2)
        else:
            r.set_measurement(start=S, length=length)
        if weighted:
            r.set_measurement_weighting(SOS)
        return r.set_measurement_histogram(B, lo, hi, mode)

    u = sr.apply_sources(mk(m, N).set_oversampling(k), [src]).render_sources(T)
    r = fresh()
    y = r.run(u, time_major=True)
    assert np.isfinite(y).all()
    seen = MeasurementWeighting(SOS).apply(y.transpose(0, 2, 1)).transpose(0, 2, 1) if weighted else y
    ref = assert_histogram(r, window(seen, S, length), B, mode)
    assert (ref[:, :, 1:B + 1].sum() > 0) and ref[:, :, B + 1].sum() > 0        # (bins and OVER both in use)
    results = {"y NULL": got(fresh().measure(u, time_major=True))[0]}
    # split calls: before the start, inside the first tile, on a tile and on a chunk boundary, beyond the window's end
    for cut in sorted({c for c in (S - 1, S + 1, S + 64, S + 150, S + 4096, S + length + 10) if 0 < c < T}):
        r = fresh()
        assert np.array_equal(r.run(np.ascontiguousarray(u[:, :cut]), time_major=True), y[:, :cut])
        r.measure(np.ascontiguousarray(u[:, cut:]), time_major=True)
        results[f"split at {cut}"] = got(r)[0]
    t1 = min(S + 137, T - 1)
    ud = dev.put(u)
    r = fresh()
    assert np.array_equal(dev.run(r, ud, True, T), y)
    results["device"] = got(r)[0]
    r = fresh()
    dev.run(r, ud, False, T)
    results["device, y NULL"] = got(r)[0]
    r = fresh()
    dev.run(r, dev.put(u[:, :t1]), False, t1)
    dev.run(r, dev.put(u[:, t1:]), False, T - t1)
    results["device, y NULL, split"] = got(r)[0]
    r = fresh()
    ya = np.zeros_like(y)
    r.run_async(u, ya)
    r.wait()
    assert np.array_equal(ya, y)
    results["async"] = got(r)[0]
    r = fresh()
    r.run_async(u, None)
    r.wait()
    results["async, y NULL"] = got(r)[0]
    r = fresh(sourced=True)
    assert np.array_equal(r.run_sources(T), y)
    results["sources"] = got(r)[0]
    results["sources, y NULL"] = got(fresh(sourced=True).measure(T=T))[0]
    monkeypatch.setenv("ACME_OS_SLICE", "150")
    results["slices of 150"] = got(fresh().measure(u, time_major=True))[0]
    r = fresh()
    assert np.array_equal(r.run(u, time_major=True), y)
    results["slices of 150, y stored"] = got(r)[0]
    # ... with chunks of one tile (the per-instance form under a table budget of one byte), the calls cut again
    monkeypatch.setenv("ACME_MEAS_TABLE_BUDGET", "1")
    b = fresh(pi=True)
    assert b.measurement_plan()["chunk"] == 64
    b.measure(np.ascontiguousarray(u[:, :t1]), time_major=True)
    b.measure(np.ascontiguousarray(u[:, t1:]), time_major=True)
    results["slices of 150, chunks of one tile, split"] = got(b)[0]
    monkeypatch.delenv("ACME_MEAS_TABLE_BUDGET")
    monkeypatch.delenv("ACME_OS_SLICE")
    # both shapes of the kernel, whatever the launch would choose
    for agg in "01":
        monkeypatch.setenv("ACME_HIST_AGG", agg)
        results[f"ACME_HIST_AGG={agg}"] = got(fresh().measure(u, time_major=True))[0]
    monkeypatch.delenv("ACME_HIST_AGG")
    # a weighting that merely coexists changes nothing beyond feeding v: the unweighted histogram is what it was
    for name, g in results.items():
        assert np.array_equal(g, ref), name
    if k > 1:
        return
    # run_const on a constant row against run on the materialised input
    uc = np.logspace(-2, 0.7, N)[:, None]
    r = fresh()
    yc = r.run(np.ascontiguousarray(np.broadcast_to(uc[:, None, :], (N, T, 1))), time_major=True)
    rc = fresh()
    assert np.array_equal(rc.run_const(np.zeros((N, T, 0)), uc, [0]), yc)
    rn = fresh().measure_const(np.zeros((N, T, 0)), uc, [0])
    for q in (rc, rn):
        assert np.array_equal(got(q)[0], got(r)[0])


# ---- 5. coexistence ------------------------------------------------------------------------------------------------------------
def check_coexistence(mk, N, T, start=5, B=65):
    m = X.wire_model(1, FS)
    u = X.scaled_rows(np.random.default_rng(2000 + N), N, T, 1)
    tgt = np.random.default_rng(9).standard_normal((2, 1, 77)) * 3.0
    which, lag = np.arange(N) % 2, np.arange(N) % 77
    groups = np.arange(N) % 4
    arm = lambda: mk(m, N).set_measurement(start=start, length=T - 50, f0=(10, 441), harmonics=3)
    adds = {"fold": lambda r: r.set_measurement_fold(50), "spectrum": lambda r: r.set_measurement_spectrum(64, 32),
            "cross": lambda r: r.set_measurement_cross(0, 64, 32),
            "target": lambda r: r.set_measurement_target(tgt, which=which, lag=lag, preemphasis=0.95),
            "ensemble": lambda r: r.set_measurement_ensemble(groups, stride=3)}
    ens = lambda r: [getattr(r.measurement_ensemble(), k) for k in ("sum", "sumsq", "min", "max", "argmin", "argmax")]
    reads = {"fold": lambda r: [r.measurement_fold(raw=True).mean], "spectrum": lambda r: [r.measurement_spectrum(raw=True).power],
             "cross": lambda r: [r.measurement_cross(raw=True).sxx, r.measurement_cross(raw=True).syy,
                                 r.measurement_cross(raw=True).sxy.real, r.measurement_cross(raw=True).sxy.imag],
             "target": lambda r: [r.measurement_target(raw=True).sums], "ensemble": ens}
    without = arm()
    for add in adds.values():
        add(without)
    y = without.run(u, time_major=True)
    every = arm()
    for add in adds.values():
        add(every)
    every.set_measurement_histogram(B, -2.0, 2.0)
    every.measure(u, time_major=True)
    assert raw(every)[1] == raw(without)[1] and np.array_equal(raw(every)[0], raw(without)[0])
    for name in adds:       # bit for bit what they are without the histogram
        for a, b in zip(reads[name](every), reads[name](without)):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64)), name
    want = assert_histogram(every, window(y, start, T - 50), B, "signed")
    alone = arm().set_measurement_histogram(B, -2.0, 2.0)
    alone.measure(u, time_major=True)
    assert np.array_equal(got(alone)[0], want)


# ---- 6. life cycle and refusals ------------------------------------------------------------------------------------------------
def check_life_cycle(mk, N=7, T=300, start=9, length=250):
    from acme_jl_amd.runner import AcmeError
    m = X.wire_model(1, FS)
    u = np.random.default_rng(5).uniform(-1.2, 1.2, (N, T, 1))
    lo, hi = -np.linspace(0.5, 1.0, N), np.linspace(0.6, 1.1, N)
    r = mk(m, N).set_measurement(start=start, length=length).set_measurement_histogram(40, lo, hi, "abs")
    y = r.run(u, time_major=True)                           # (the pass-through model has no state: a rerun repeats y)
    first = assert_histogram(r, window(y, start, length), 40, "abs")
    # a reset zeroes the counters and keeps bins, mode and the ranges
    r.reset_measurement()
    full, count, glo, ghi, gs = got(r)
    assert count == 0 and not full.any() and np.array_equal(glo, lo) and np.array_equal(ghi, hi) and np.array_equal(gs, 40.0 / (hi - lo))
    r.measure(u, time_major=True)
    assert np.array_equal(got(r)[0], first) and r.measurement_histogram().mode == "abs"
    # a histogram set again replaces the earlier one (after a reset: nothing has been fed)
    r.reset_measurement().set_measurement_histogram(3, -1.0, 1.0)
    r.measure(u, time_major=True)
    again = assert_histogram(r, window(y, start, length), 3, "signed")
    assert again.shape == (N, 1, 6) and (got(r)[2] == -1.0).all()
    # re-arming and clear remove it
    L = r.lib.L
    r.set_measurement(start=start, length=length)
    with pytest.raises(AcmeError, match="no measurement histogram"):
        r.measurement_histogram()
    assert L.acme_batch_get_measurement_histogram(r.h, None, None, None) == -1 and "no measurement histogram" in L.acme_last_error().decode()
    r.set_measurement_histogram(3, -1.0, 1.0).clear_measurement()
    assert L.acme_batch_get_measurement_histogram(r.h, None, None, None) == -1 and "no measurement histogram" in L.acme_last_error().decode()
    with pytest.raises(AcmeError, match="no measurement is armed"):
        r.set_measurement_histogram(3, -1.0, 1.0)
    # an unbounded window, and a start beyond the run: nothing counted
    r = mk(m, N).set_measurement(start=start).set_measurement_histogram(5, -1.0, 1.0)
    r.measure(u, time_major=True)
    assert_histogram(r, window(y, start, 0), 5, "signed")
    r = mk(m, N).set_measurement(start=T + 5).set_measurement_histogram(5, -1.0, 1.0)
    r.measure(u, time_major=True)
    assert got(r)[1] == 0 and not got(r)[0].any()


def check_set_matrices_carries_the_histogram(mk):
    from helpers import sweep_inputs
    from test_emu_parity import superover_models_with_their_own_diodes
    models = superover_models_with_their_own_diodes(3, HS)
    u = np.ascontiguousarray(sweep_inputs("superover_var", 3, 60, seed=2).transpose(0, 2, 1))
    r = mk(models[0], 3, models=[models[0]] * 3).set_measurement(start=10, length=45)
    lo, hi = [-1.0, -0.5, -0.1], [1.0, 0.5, 0.1]
    r.set_measurement_histogram(16, lo, hi)
    ya = r.run(np.ascontiguousarray(u[:, :25]), time_major=True)
    r.set_models(1, [models[0]])
    r.set_models(2, [models[2]])                            # (the batch moves to the plain shape: a new batch takes the measurement over)
    yb = r.run(np.ascontiguousarray(u[:, 25:]), time_major=True)
    assert_histogram(r, window(np.concatenate([ya, yb], axis=1), 10, 45), 16, "signed")
    assert np.array_equal(got(r)[2], lo) and np.array_equal(got(r)[3], hi)


def check_errors(mk):
    """every refusal with its code and the argument's name in the message"""
    from acme_jl_amd.runner import AcmeError, DimensionMismatch, _dp
    m = X.wire_model(1, FS)
    u = np.zeros((3, 10, 1))

    def refused(r, code, what, bins, mode, lo, hi, lo_i=None, hi_i=None):
        la = None if lo_i is None else np.asarray(lo_i, dtype=np.float64)
        ha = None if hi_i is None else np.asarray(hi_i, dtype=np.float64)
        rc = r.lib.L.acme_batch_set_measurement_histogram(r.h, bins, mode, lo, hi, None if la is None else _dp(la),
                                                          None if ha is None else _dp(ha))
        msg = r.lib.L.acme_last_error().decode()
        assert rc == code and all(w in msg for w in what), (bins, mode, lo, hi, lo_i, hi_i, rc, msg)
    r = mk(m, 3)
    refused(r, -1, ["no measurement is armed"], 8, 0, -1.0, 1.0)
    r.set_measurement(start=1)
    for bins in (0, -1, MAX_BINS + 1):
        refused(r, -1, ["bins", str(MAX_BINS)], bins, 0, -1.0, 1.0)
    for mode in (-1, 2):
        refused(r, -1, ["mode"], 8, mode, -1.0, 1.0)
    for bad in (np.nan, np.inf, -np.inf):
        refused(r, -1, ["lo", "finite"], 8, 0, bad, 1.0)
        refused(r, -1, ["hi", "finite"], 8, 0, -1.0, bad)
        refused(r, -1, ["lo_i", "instance 1", "finite"], 8, 0, 0.0, 0.0, [-1.0, bad, -1.0], [1.0, 1.0, 1.0])
        refused(r, -1, ["hi_i", "instance 2", "finite"], 8, 0, 0.0, 0.0, [-1.0, -1.0, -1.0], [1.0, 1.0, bad])
    refused(r, -1, ["lo >= hi"], 8, 0, 1.0, 1.0)
    refused(r, -1, ["lo >= hi"], 8, 0, 1.0, -1.0)
    refused(r, -1, ["lo_i >= hi_i", "instance 2"], 8, 0, 0.0, 0.0, [-1.0, -1.0, 0.5], [1.0, 1.0, 0.5])
    refused(r, -1, ["hi - lo", "overflows"], 8, 0, -1.5e308, 1.5e308)
    refused(r, -1, ["hi_i - lo_i", "instance 0", "overflows"], 8, 0, 0.0, 0.0, [-1.5e308, 0.0, 0.0], [1.5e308, 1.0, 1.0])
    refused(r, -1, ["hi_i", "NULL"], 8, 0, -1.0, 1.0, [-1.0, -1.0, -1.0], None)
    refused(r, -1, ["lo_i", "NULL"], 8, 0, -1.0, 1.0, None, [1.0, 1.0, 1.0])
    assert r.lib.L.acme_batch_get_measurement_histogram(r.h, None, None, None) == -1   # (a refused histogram leaves none behind)
    # the arrays win over the scalars when both are given (the scalars are ignored, even unusable ones)
    r.set_measurement(start=1)
    assert r.lib.L.acme_batch_set_measurement_histogram(r.h, 8, 0, np.nan, np.nan, _dp(np.array([-1.0, -2.0, -3.0])),
                                                        _dp(np.array([1.0, 2.0, 3.0]))) == 0
    rng = np.empty((3, 3))
    assert r.lib.L.acme_batch_get_measurement_histogram(r.h, None, _dp(rng), None) == 0
    assert np.array_equal(rng, [[-1.0, 1.0, 4.0], [-2.0, 2.0, 2.0], [-3.0, 3.0, 8.0 / 6.0]])
    r.measure(u, time_major=True)
    refused(r, -1, ["samples have been fed"], 8, 0, -1.0, 1.0)
    r.reset_measurement()
    # a series and a histogram exclude each other, whichever is set first
    r.set_measurement_histogram(8, -1.0, 1.0)
    assert r.lib.L.acme_batch_set_measurement_series(r.h, 4, 4, 2) == -2 and "histogram" in r.lib.L.acme_last_error().decode()
    with pytest.raises(AcmeError, match="histogram"):
        r.set_measurement_series(4, 4, 2)
    r.set_measurement(start=1).set_measurement_series(4, 4, 2)
    refused(r, -2, ["series"], 8, 0, -1.0, 1.0)
    # the Python layer's own refusals
    r.set_measurement(start=1)
    with pytest.raises(DimensionMismatch):
        r.set_measurement_histogram(8, [0.0, 0.0], 1.0)
    with pytest.raises(DimensionMismatch):
        r.set_measurement_histogram(8, 0.0, [1.0, 1.0])
    with pytest.raises(ValueError, match="mode"):
        r.set_measurement_histogram(8, 0.0, 1.0, mode="log")


def check_cap(mk, N, accept):
    """one counter a pair beyond N nrows (B + 3) = ACME_MAX_HISTOGRAM is refused, by the arming call alone; ``accept``: the
    cap itself is accepted (2 GiB of counters) and cleared at once"""
    B = CAP // N - 3
    assert N * (B + 3) == CAP and 1 <= B < MAX_BINS
    r = mk(X.wire_model(1, FS), N).set_measurement()
    rc = r.lib.L.acme_batch_set_measurement_histogram(r.h, B + 1, 0, -1.0, 1.0, None, None)
    msg = r.lib.L.acme_last_error().decode()
    assert rc == -1 and "N nrows (B + 3)" in msg and str(CAP) in msg, (rc, msg)
    if not accept:
        return
    r.set_measurement_histogram(B, -1.0, 1.0)
    count = C.c_longlong(-1)
    assert r.lib.L.acme_batch_get_measurement_histogram(r.h, None, None, C.byref(count)) == 0 and count.value == 0
    r.clear_measurement()


# ---- 7. a non-finite instance ---------------------------------------------------------------------------------------------------
def check_nan_instance(mk, N=4, T=50, bad=20):
    """the recipe of test_measurement: a NaN in one instance's input.  From that sample on the instance counts in NAN; its
    neighbours are untouched"""
    from test_measurement import clipper_u
    m, u = clipper(), clipper_u(N, T)
    ok = mk(m, N).set_measurement(length=T).set_measurement_histogram(32, -1.0, 1.0)
    ok.measure(u, time_major=True)
    clean = got(ok)[0]
    u[1, bad, 0] = np.nan
    r = mk(m, N).set_measurement(length=T).set_measurement_histogram(32, -1.0, 1.0)
    y = r.run(u, time_major=True, check=False)
    assert r.report_arrays()["first_nonfinite"].tolist()[1] >= 0
    assert np.isnan(y[1, bad:]).all() and np.isfinite(y[[0, 2, 3]]).all() and np.isfinite(y[1, :bad]).all()
    full = assert_histogram(r, y, 32, "signed")
    assert full[1, 0, 34] == T - bad and full[1, 0, :34].sum() == bad
    assert np.array_equal(full[[0, 2, 3]], clean[[0, 2, 3]]) and not full[[0, 2, 3], :, 34].any()


# ---- 9. a real circuit ----------------------------------------------------------------------------------------------------------
def check_use_level(mk, N=16, T=441 * 6, B=200):
    """the diode clipper over a level sweep (a 1 kHz sine source), the rectified output binned over [0, the input's peak): the
    harder the drive, the smaller the share of the window the output spends in the top tenth of ITS range and the larger the
    share it spends near the clipping level; the median from the bins agrees with numpy's on the stored y to a bin width"""
    m = clipper()
    amp = np.logspace(-1, 0.7, N)
    src = dict(kind="sine", f_den=441, f_num=np.full(N, 10), amp=amp)
    start, length = 441, T - 441                            # whole periods behind one period of settling
    y = sr.apply_sources(mk(m, N), [src]).run_sources(T)
    r = sr.apply_sources(mk(m, N), [src]).set_measurement(start=start, length=length)
    r.set_measurement_histogram(B, 0.0, amp, mode="abs")
    r.measure(T=T)
    h = r.measurement_histogram()
    yw = window(y, start, length)
    assert_histogram(r, yw, B, "abs")
    assert h.count == length and not h.nan.any() and not h.under.any() and not h.over.any()     # |y| < the input's peak
    top = h.counts[:, 0, B - B // 10:].sum(axis=-1) / h.count
    assert (np.diff(top) <= 0).all() and top[0] > top[-1] == 0.0, top
    level = 0.8 * np.abs(yw[-1]).max()                      # near the clipping level: 80 % of the hardest driven output's peak
    near = h.fraction_above(level)[:, 0]
    assert (np.diff(near) >= 0).all() and near[0] == 0.0 and near[-1] > 0.5, near
    exact = (np.abs(yw[:, :, 0]) >= level).mean(axis=1)
    assert (np.abs(near - exact) <= h.counts[:, 0].max(axis=-1) / h.count).all()               # off by one bin's share at most
    med = h.percentile(50)[:, 0]
    assert (np.abs(med - np.median(np.abs(yw[:, :, 0]), axis=1)) <= 1.0 / h.scale).all()
    return h, top, near


# ---- the result object ----------------------------------------------------------------------------------------------------------
def check_object(mk):
    from acme_jl_amd.runner import MeasurementHistogram
    N, T = 3, 8
    u = np.array([[-0.9, -0.6, -0.4, -0.1, 0.1, 0.4, 0.6, 0.9], [0.05] * 8, [-3.0, 3.0, 0.1, 0.1, 0.3, 0.3, 0.6, np.nan]])[:, :, None]
    r = mk(X.wire_model(1, FS), N).set_measurement().set_measurement_histogram(4, -1.0, [1.0, 1.0, 1.0])
    r.measure(np.ascontiguousarray(u), time_major=True, check=False)
    h = r.measurement_histogram()
    assert h.bins == 4 and h.count == T and h.mode == "signed" and h.rows == (0,) and h.counts.shape == (N, 1, 4)
    assert h.counts[:, 0].tolist() == [[2, 2, 2, 2], [0, 0, 8, 0], [0, 0, 4, 1]]
    assert h.under[:, 0].tolist() == [0, 0, 1] and h.over[:, 0].tolist() == [0, 0, 1] and h.nan[:, 0].tolist() == [0, 0, 1]
    assert h.edges(0).tolist() == [-1.0, -0.5, 0.0, 0.5, 1.0] and h.scale.tolist() == [2.0] * 3
    assert h.pdf()[0, 0].tolist() == [0.5] * 4 and h.pdf()[2, 0].tolist() == [0.0, 0.0, 8.0 / 7.0, 2.0 / 7.0]
    assert h.cdf()[0, 0].tolist() == [0.0, 0.25, 0.5, 0.75, 1.0]
    assert np.allclose(h.cdf()[2, 0], np.array([1, 1, 1, 5, 6]) / 7.0, rtol=0, atol=1e-16)
    assert h.percentile(50)[:, 0].tolist()[:2] == [0.0, 0.25] and h.percentile(25)[0, 0] == -0.5
    assert h.percentile([0, 100])[:, 0, 0].tolist() == [-1.0, 1.0]
    p = h.percentile([5, 50, 99])[:, 2, 0]                  # 7 valued samples: 1 under, 4 + 1 inside, 1 over
    assert np.isnan(p[0]) and np.isnan(p[2]) and p[1] == 0.0 + (3.5 - 1.0) / 4.0 * 0.5
    assert h.fraction_below(0.0)[:, 0].tolist() == [0.5, 0.0, 1.0 / 7.0] and h.fraction_above(0.5)[0, 0] == 0.25
    assert h.fraction_below(0.25)[0, 0] == 0.625 and h.fraction_below([-1.0, 1.0, 1.0])[:, 0].tolist() == [0.0, 1.0, 6.0 / 7.0]
    # outside the range the answer is known where UNDER / OVER hold nothing, and NaN where they do
    assert h.fraction_below(2.0)[:2, 0].tolist() == [1.0, 1.0] and np.isnan(h.fraction_below(2.0)[2, 0])
    assert h.fraction_below(-2.0)[:2, 0].tolist() == [0.0, 0.0] and np.isnan(h.fraction_above(-2.0)[2, 0])
    j = MeasurementHistogram.concatenate([h, h])
    assert j.counts.shape == (6, 1, 4) and j.count == T and np.array_equal(j.lo, np.tile(h.lo, 2)) and np.array_equal(j.counts[3:], h.counts)
    other = MeasurementHistogram(h.counts, h.under, h.over, h.nan, T + 1, h.lo, h.hi, h.scale, h.mode, h.rows)
    with pytest.raises(ValueError, match="differ"):
        MeasurementHistogram.concatenate([h, other])
