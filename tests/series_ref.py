"""Shared by the emulator and GPU tests of measurement series (acme_batch_set_measurement_series): the raw getter, which
windows a test compares, and the reference every window is held to -- the single-window form of the same measurement, armed
at start + w hop with length win on an identical run, bit for bit (accumulators, hence every reported number, and count).

``mk(model, n)`` makes a fresh runner on the library under test (the emulator's or the GPU's)."""
import ctypes as C

import numpy as np

import exact_ref as X
import measure_pi_ref as PI
import multitone_ref as MT
import source_ref as sr
from helpers import FS
from test_measurement import clipper, clipper_u, raw, two_output_clipper

M31 = 2 ** 31 - 1

# (win, hop, W) of the boundary geometry, with start = 301 and T = 9000
GEOMETRY = [(64, 64, 100),       # boundaries inside every tile, because of start
            (441, 441, 25),      # windows straddle tiles and chunks; the series outlasts the run
            (5, 7, 40),          # several windows and gaps inside one tile
            (1, 1, 70),          # one-sample windows
            (100, 257, 30),      # gaps
            (10, 5000, 2),       # a gap longer than a chunk
            (5000, 5000, 2),     # a window longer than a chunk; the second window partial
            (441, 441, 3)]       # the series ends mid-run and later samples are ignored


def raw_series(r, first=0, n=None):
    """(out [n, N, nrows, 4 + 2H], counts [n]) straight from acme_batch_get_measurement_series"""
    from acme_jl_amd.runner import _dp
    H, rows = r._meas
    n = r._series[1][2] - first if n is None else n
    out = np.empty((n, r.n, len(rows), 4 + 2 * H))
    counts = np.zeros(n, dtype=np.int64)
    r.lib.check(r.lib.L.acme_batch_get_measurement_series(r.h, first, n, _dp(out), counts.ctypes.data_as(C.POINTER(C.c_longlong))))
    return out, counts


def expected_counts(start, win, hop, W, T):
    """samples of window w among the first T since arming"""
    return np.clip(T - start - np.arange(W) * hop, 0, win)


def pick_windows(counts, win):
    """the windows a test compares: all of at most 8; otherwise 8 or more that include window 0, the last complete window,
    the partial window and one window past the end of the run (count 0) where the series has them"""
    W = len(counts)
    if W <= 8:
        return list(range(W))
    full, part, none = (np.flatnonzero(c) for c in (counts == win, (counts > 0) & (counts < win), counts == 0))
    must = {0} | {int(v[k]) for v, k in ((full, -1), (part, 0), (none, 0)) if len(v)}
    return sorted(must | {int(v) for v in np.linspace(0, W - 1, 8).round()})


def assert_series_is_single_windows(got, arm, feed, start, win, hop, T):
    """window w of ``got`` (raw_series) == raw() of ``arm(start + w hop, win)`` after ``feed``, with equal counts; the counts
    are those of T samples.  Returns the windows compared."""
    out, counts = got
    assert np.array_equal(counts, expected_counts(start, win, hop, len(counts), T)), counts
    picked = pick_windows(counts, win)
    for w in picked:
        q = arm(start + w * hop, win)
        feed(q)
        o, c = raw(q)
        assert c == counts[w], (w, c, counts[w])
        assert np.array_equal(o, out[w], equal_nan=True), (w, np.argwhere(o != out[w])[:8])
        if c == 0:
            assert np.isnan(out[w][:, :, 0]).all() and np.isposinf(out[w][:, :, 2]).all() and np.isneginf(out[w][:, :, 3]).all()
    return picked


# ---- 1. boundary geometry ---------------------------------------------------------------------------------------------------
def check_geometry(mk, m, N, T, start, H, series, rows=None, cut=False):
    """``cut``: a reference run ends with its window (the same run as far as the window can see; the emulator's time)"""
    win, hop, W = series
    u = clipper_u(N, T)
    spec = dict(f0=(10, 441) if H else None, harmonics=H, rows=rows)
    r = mk(m, N).set_measurement(start=start, **spec).set_measurement_series(win, hop, W)
    r.measure(u, time_major=True)
    def feed(q):
        end = min(T, q._series[0] + win) if cut else T
        q.measure(np.ascontiguousarray(u[:, :end]), time_major=True)
    assert_series_is_single_windows(raw_series(r), lambda s, n: mk(m, N).set_measurement(start=s, length=n, **spec),
                                    feed, start, win, hop, T)


# ---- 2. forms ---------------------------------------------------------------------------------------------------------------
FORM_SERIES = [(441, 441, 9), (5, 7, 40)]


def check_per_instance(mk, f_num, kinds, T, start=3, H=10, f_den=441, wire=False):
    """``wire``: the pass-through model on random rows in place of the diode clipper, every reference window fed its own
    samples only (the emulator: N x T of the clipper per reference window would take minutes)"""
    N = len(f_num)
    m, u = (X.wire_model(1, FS), X.scaled_rows(np.random.default_rng(N), N, T, 1)) if wire else (clipper(), clipper_u(N, T))
    for win, hop, W in FORM_SERIES:
        r = mk(m, N).set_measurement(start=start, f_den=f_den, f_num=f_num, harmonics=H)
        assert PI.wave_kinds(r) == kinds
        r.set_measurement_series(win, hop, W)
        assert PI.wave_kinds(r) == kinds                    # (the plan is the armed form's, unchanged)
        r.measure(u, time_major=True)

        def arm(s, n):
            q = mk(m, N).set_measurement(start=0 if wire else s, length=n, f_den=f_den, f_num=f_num, harmonics=H)
            q.seg = (s, min(T, s + n))
            return q

        def feed(q):
            if not wire:
                q.measure(u, time_major=True)
            elif q.seg[0] < q.seg[1]:           # (y = u without state: the window's own samples are an identical run of it)
                q.measure(np.ascontiguousarray(u[:, q.seg[0]:q.seg[1]]), time_major=True)
        assert_series_is_single_windows(raw_series(r), arm, feed, start, win, hop, T)


def check_bins(mk, f_num, kinds, T, start=3, f_den=441, coef=MT.COEF6, wire=False):
    """COEF6: both tones, the difference either way round (one wraps below zero) and a bin at k = 0 (C the sum, S = 0)"""
    N = f_num.shape[1]
    m = X.wire_model(1, FS) if wire else clipper()
    kb = MT.bin_frequencies(coef, f_num, f_den)
    assert (kb == 0).any() and (np.asarray(coef) @ f_num < 0).any()
    src = dict(kind="multisine", f_den=f_den, f_num=f_num, amp=np.stack([np.logspace(-1, 0.4, N)] * 2))

    def arm(s, n):
        return sr.apply_sources(mk(m, N), [src]).set_measurement_bins(coef, tones_from_source=0, start=s, length=n)
    feed = lambda q: q.measure(T=T)
    if wire:        # (y = u without state: a reference window is fed its own samples of the rendered input, as check_per_instance)
        u = sr.apply_sources(mk(m, N), [src]).render_sources(T)

        def ref(s, n):
            q = mk(m, N).set_measurement_bins(coef, f_den=f_den, f_num=f_num, start=0, length=n)
            q.seg = (s, min(T, s + n))
            return q
        feed = lambda q: q.seg[0] < q.seg[1] and q.measure(np.ascontiguousarray(u[:, q.seg[0]:q.seg[1]]), time_major=True)
    for win, hop, W in FORM_SERIES:
        r = arm(start, 0)
        assert PI.wave_kinds(r) == kinds
        r.set_measurement_series(win, hop, W).measure(T=T)
        got = raw_series(r)
        picked = assert_series_is_single_windows(got, ref if wire else arm, feed, start, win, hop, T)
        for w in picked:
            if got[1][w]:
                for b, i in np.argwhere(kb == 0):
                    assert np.array_equal(got[0][w, i, :, 4 + 2 * b], 2.0 * got[0][w, i, :, 0]) and not got[0][w, i, :, 5 + 2 * b].any()


# ---- 4. exact pins ------------------------------------------------------------------------------------------------------------
def check_exact(mk, N=7, T=8237, start=37, series=(300, 1000, 9), H=10, f_num=1234567):
    """the pass-through model at f_den = 2^31 - 1: per window the moments bit for bit and C_h / S_h within
    exact_ref.harmonic_bound of the window's segment (the last window partial).  Returns the worst |error| / bound."""
    win, hop, W = series
    u = X.scaled_rows(np.random.default_rng(2311), N, T, 2)
    r = mk(X.wire_model(2, FS), N).set_measurement(start=start, f0=(f_num, M31), harmonics=H).set_measurement_series(win, hop, W)
    assert np.array_equal(r.run(u, time_major=True), u)
    out, counts = raw_series(r)
    assert np.array_equal(counts, expected_counts(start, win, hop, W, T)) and 0 < counts[-1] < win
    worst = 0.0
    for w in range(W):
        s = start + w * hop
        worst = max(worst, PI.check_exact_per_instance(out[w], int(counts[w]), u[:, s:s + counts[w]], M31, np.full(N, f_num), H))
    return worst


# ---- 7. no-series invariance -------------------------------------------------------------------------------------------------
def check_no_series_invariance(mk, N, T):
    """a batch armed without a series, and one armed after a series has been set and removed: the existing forms' results"""
    m, u = clipper(), clipper_u(N, T)
    f_num = np.array([10, 20, 30])[np.arange(N) % 3]
    arms = {"shared": lambda r: r.set_measurement(start=5, f0=(10, 441), harmonics=10),
            "per instance": lambda r: r.set_measurement(start=5, f_den=441, f_num=f_num, harmonics=10),
            "bins": lambda r: r.set_measurement_bins(np.array([[1], [2], [3]]), start=5, f_den=441, f_num=f_num[None])}
    for name, arm in arms.items():
        a = arm(mk(m, N))
        y = a.run(u, time_major=True)
        b = arm(mk(m, N)).set_measurement_series(64, 100, 12)
        arm(b)                                              # (arming removes the series)
        assert np.array_equal(b.run(u, time_major=True), y)
        c = arm(mk(m, N)).set_measurement_series(64, 100, 12).clear_measurement()
        arm(c).measure(u, time_major=True)
        (oa, ca), (ob, cb), (oc, cc) = raw(a), raw(b), raw(c)
        assert ca == cb == cc == T - 5, name
        assert np.array_equal(oa, ob) and np.array_equal(oa, oc), name


# ---- 3. paths -----------------------------------------------------------------------------------------------------------------
PATH_SERIES, PATH_START = (100, 257, 30), 1203      # window w over 1203 + 257 w ... + 100: the start lies beyond a first call of 1000


def check_paths(mk, dev, k, T, monkeypatch, N=70):
    """one series, H = 10, the diode clipper at N = 70 driven by what a per-instance sine source renders: the series read after
    every path == the one after a host run with y stored.  ``dev``: the device-memory calls (put, run_device(r, u, y or None, T))."""
    from fractions import Fraction
    from acme_jl_amd import examples
    from acme_jl_amd.model import DiscreteModel
    from helpers import HS
    win, hop, W = PATH_SERIES
    H, S = 10, PATH_START
    m = clipper() if k == 1 else DiscreteModel(examples.diodeclipper(), Fraction(1, k * FS), HS)
    src = dict(kind="sine", f_den=441, f_num=np.full(N, 10), amp=np.logspace(-2, 0.7, N))

    def fresh(sourced=False):
        r = mk(m, N).set_oversampling(k)
        if sourced:
            return sr.apply_sources(r, [src]).set_measurement(start=S, harmonics=H, f0_from_source=0).set_measurement_series(win, hop, W)
        return r.set_measurement(start=S, f0=(10, 441), harmonics=H).set_measurement_series(win, hop, W)
    u = sr.apply_sources(mk(m, N).set_oversampling(k), [src]).render_sources(T)
    r = fresh()
    y = r.run(u, time_major=True)
    ref = raw_series(r)
    assert np.isfinite(y).all() and np.array_equal(ref[1], expected_counts(S, win, hop, W, T)) and ref[1][0] == win
    results = {"y NULL": raw_series(fresh().measure(u, time_major=True))}
    # split calls: before the start, behind a window's last sample, inside a gap, on a window's first sample, inside a window
    cuts = [1000, S + hop + win, S + hop + 180, S + 2 * hop, S + 3 * hop + 40]
    assert cuts[-1] < T
    r = fresh()
    for j, (a, b) in enumerate(zip([0] + cuts, cuts + [T])):
        part = np.ascontiguousarray(u[:, a:b])
        if j % 2:
            r.measure(part, time_major=True)
        else:
            assert np.array_equal(r.run(part, time_major=True), y[:, a:b])
    results["split"] = raw_series(r)
    ud = dev.put(u)
    r = fresh()
    yd = dev.run(r, ud, True, T)
    assert np.array_equal(yd, y)
    results["device"] = raw_series(r)
    r = fresh()
    dev.run(r, ud, False, T)
    results["device, y NULL"] = raw_series(r)
    r = fresh()
    t1 = cuts[-1]
    dev.run(r, dev.put(u[:, :t1]), False, t1)
    dev.run(r, dev.put(u[:, t1:]), False, T - t1)
    results["device, y NULL, split"] = raw_series(r)
    r = fresh()
    ya = np.zeros_like(y)
    r.run_async(u, ya)
    r.wait()
    assert np.array_equal(ya, y)
    results["async"] = raw_series(r)
    r = fresh()
    r.run_async(u, None)
    r.wait()
    results["async, y NULL"] = raw_series(r)
    r = fresh(sourced=True)
    assert np.array_equal(r.run_sources(T), y)
    results["sources"] = raw_series(r)
    results["sources, y NULL"] = raw_series(fresh(sourced=True).measure(T=T))
    monkeypatch.setenv("ACME_OS_SLICE", "150")
    results["slices of 150"] = raw_series(fresh().measure(u, time_major=True))
    r = fresh()
    assert np.array_equal(r.run(u, time_major=True), y)
    results["slices of 150, y stored"] = raw_series(r)
    monkeypatch.delenv("ACME_OS_SLICE")
    for name, (out, counts) in results.items():
        assert np.array_equal(counts, ref[1]), name
        assert np.array_equal(out, ref[0], equal_nan=True), (name, np.argwhere(out != ref[0])[:8])
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
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(raw_series(q), raw_series(r)))
    # the table budget forcing one-tile chunks, per-instance F = N
    f_num = 1 + np.arange(N)

    def pi():
        return mk(m, N).set_measurement(start=S, f_den=441, f_num=f_num, harmonics=H).set_measurement_series(win, hop, W)
    a = pi()
    assert a.measurement_plan()["chunk"] == 4096
    a.measure(u, time_major=True)
    monkeypatch.setenv("ACME_MEAS_TABLE_BUDGET", "1")
    b = pi()
    assert b.measurement_plan()["chunk"] == 64
    b.measure(np.ascontiguousarray(u[:, :t1]), time_major=True)
    b.measure(np.ascontiguousarray(u[:, t1:]), time_major=True)
    monkeypatch.delenv("ACME_MEAS_TABLE_BUDGET")
    assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(raw_series(a), raw_series(b)))
    # reset restarts the series; re-arming removes it
    from acme_jl_amd.runner import AcmeError
    import pytest
    r = fresh()
    r.run(u, time_major=True)
    r.reset_measurement()
    q = mk(m, N)
    q.run(u, time_major=True)
    q.set_measurement(start=S, f0=(10, 441), harmonics=H).set_measurement_series(win, hop, W)
    u2 = np.ascontiguousarray(u[:, :S + 2 * hop + 30])
    r.measure(u2, time_major=True)
    q.measure(u2, time_major=True)
    (o1, c1), (o2, c2) = raw_series(r), raw_series(q)
    assert c1.tolist()[:4] == [win, win, 30, 0] and np.array_equal(c1, c2) and np.array_equal(o1, o2, equal_nan=True)
    with pytest.raises(AcmeError, match="measurement_series"):
        r.measurement()
    r.set_measurement(start=S, f0=(10, 441), harmonics=H)
    with pytest.raises(AcmeError, match="no measurement series"):
        r.measurement_series()
    assert r.measure(u2, time_major=True).measurement().count == 2 * hop + 30
