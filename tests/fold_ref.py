"""Shared by the emulator and GPU tests of the measurement fold (acme_batch_set_measurement_fold): the reference every fold
is held to -- numpy on the stored y of an identical run without a fold, slot by slot a sequential float64 chain from 0.0 --
and the checks, each taking ``mk(model, n)``, which makes a fresh runner on the library under test (the emulator's or the
GPU's).  The slots' sums (``measurement_fold(raw=True)``) and the reported means are compared with ``==``."""
import ctypes as C
import functools

import numpy as np
import pytest

import exact_ref as X
import measure_pi_ref as PI
import multitone_ref as MT
import source_ref as sr
from helpers import FS, HS, load
from test_measurement import clipper, clipper_u, raw, two_output_clipper

CAP = 65536
# the periods of the geometry, with start = 301 and T = 9000: one slot block and many; the chunk length (4096) and its
# neighbours; a period longer than a chunk
GEOMETRY = [1, 5, 63, 64, 65, 441, 4095, 4096, 4097, 5000]


def fold_sums(yw, P):
    """yw [count, ...], the window's samples along axis 0 -> (acc [P, ...], c [P]): slot s the sum of yw[s], yw[s + P], ...
    added in that order from 0.0, and the number of its samples"""
    acc = np.zeros((P,) + yw.shape[1:])
    for k in range(0, len(yw), P):
        seg = yw[k:k + P]
        acc[:len(seg)] += seg
    s = np.arange(P)
    return acc, np.where(len(yw) > s, (len(yw) - s - 1) // P + 1, 0)


def got_fold(r):
    """(sums, mean [N, nrows, Pmax], period [N], count) of the runner's fold"""
    a, b = r.measurement_fold(raw=True), r.measurement_fold()
    assert a.count == b.count and np.array_equal(a.period, b.period) and a.rows == b.rows
    return a.mean, b.mean, b.period, b.count


def assert_fold(got, yw, period):
    """``got`` (got_fold) against the reference on the window's samples yw [N, count, nrows]"""
    sums, mean, per, count = got
    period = np.broadcast_to(np.asarray(period, dtype=np.int64), (yw.shape[0],))
    assert count == yw.shape[1] and np.array_equal(per, period), (count, yw.shape, per[:4])
    assert sums.shape == mean.shape == (yw.shape[0], yw.shape[2], period.max())
    for P in np.unique(period):
        idx = np.flatnonzero(period == P)
        acc, c = fold_sums(np.ascontiguousarray(yw[idx].transpose(1, 0, 2)), int(P))
        acc = acc.transpose(1, 2, 0)                        # [instances, nrows, P]
        with np.errstate(invalid="ignore", divide="ignore"):
            want_sum, want_mean = np.where(c > 0, acc, np.nan), np.where(c > 0, acc / c, np.nan)
        assert np.array_equal(sums[idx][:, :, :P], want_sum, equal_nan=True), (P, np.argwhere(sums[idx][:, :, :P] != want_sum)[:6])
        assert np.array_equal(mean[idx][:, :, :P], want_mean, equal_nan=True), P
        assert np.isnan(mean[idx][:, :, P:]).all() and np.isnan(sums[idx][:, :, P:]).all(), P   # the slots beyond a pair's period
    return sums


def same_fold(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def window(y, start, length, rows=None):
    """the measured samples of the stored y [N, T, ny]: [N, count, nrows]"""
    end = y.shape[1] if not length else min(y.shape[1], start + length)
    return y[:, start:end][:, :, list(range(y.shape[2])) if rows is None else rows]


# ---- 1. period geometry, 3. rows --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plain_run(mk, two, N, T, start, length, H, rows):
    """the run without a fold every geometry case of a shape shares: (u, y, raw measurement); never modified"""
    m = two_output_clipper() if two else clipper()
    u = clipper_u(N, T)
    r = mk(m, N).set_measurement(start=start, length=length, f0=(10, 441) if H else None, harmonics=H, rows=None if rows is None else list(rows))
    y = r.run(u, time_major=True)
    return m, u, y, raw(r)


def check_geometry(mk, N, T, start, H, P, length=0, rows=None, two=False):
    m, u, y, plain = _plain_run(mk, two, N, T, start, length, H, None if rows is None else tuple(rows))
    r = mk(m, N).set_measurement(start=start, length=length, f0=(10, 441) if H else None, harmonics=H, rows=rows).set_measurement_fold(P)
    assert np.array_equal(r.run(u, time_major=True), y)
    with_fold = raw(r)
    assert with_fold[1] == plain[1] and np.array_equal(with_fold[0], plain[0])        # the measurement's own results
    got = got_fold(r)
    assert_fold(got, window(y, start, length, rows), P)
    return got, with_fold[1]


# ---- 2. per-instance periods --------------------------------------------------------------------------------------------------
def period_cases():
    return {"all equal": np.full(131, 441),
            "123-7-1": np.array([441] * 123 + [64] * 7 + [7]),
            "all distinct": 1 + np.arange(130),
            "Pmax of one": np.array([7] * 64 + [5000] + [7] * 65)}


def check_per_instance(mk, period, T, start=301, H=10, wire=False, shared=None):
    """one batch with a period per instance: the numpy reference, and each instance == the shared fold at its own period
    (``shared``: at most so many of the distinct periods, evenly spread -- the emulator's time)"""
    N = len(period)
    m, u = (X.wire_model(1, FS), X.scaled_rows(np.random.default_rng(N), N, T, 1)) if wire else (clipper(), clipper_u(N, T))
    arm = lambda: mk(m, N).set_measurement(start=start, f0=(10, 441), harmonics=H)
    r = arm().set_measurement_fold(period)
    y = r.run(u, time_major=True)
    got = got_fold(r)
    assert_fold(got, window(y, start, 0), period)
    distinct = np.unique(period)
    if shared is not None and len(distinct) > shared:
        distinct = distinct[np.linspace(0, len(distinct) - 1, shared).round().astype(int)]
    for P in distinct:
        q = arm().set_measurement_fold(int(P))
        q.measure(u, time_major=True)
        shared, idx = got_fold(q), np.flatnonzero(period == P)
        for k in (0, 1):
            assert np.array_equal(got[k][idx][:, :, :P], shared[k][idx], equal_nan=True), P
        assert shared[3] == got[3]


# ---- 5. all three forms carry a fold ----------------------------------------------------------------------------------------
def check_forms(mk, T, periods, start=3, H=10, wire=False, forms=("shared", "per instance", "bins")):
    """shared, per instance with mixed waves (F = N = 130) and bins (COEF6): the fold is the reference's, and the measurement's
    own results with the fold attached == those without it"""
    N, f_den = 130, 441
    m, u = (X.wire_model(1, FS), X.scaled_rows(np.random.default_rng(7), N, T, 1)) if wire else (clipper(), clipper_u(N, T))
    f_num = 1 + np.arange(N)
    tones = MT.tone_cases()["F=N"][0]
    arms = {"shared": lambda: mk(m, N).set_measurement(start=start, f0=(10, f_den), harmonics=H),
            "per instance": lambda: mk(m, N).set_measurement(start=start, f_den=f_den, f_num=f_num, harmonics=H),
            "bins": lambda: mk(m, N).set_measurement_bins(MT.COEF6, start=start, f_den=f_den, f_num=tones)}
    for name in forms:
        arm = arms[name]
        a = arm()
        if name == "per instance":
            assert PI.wave_kinds(a) == (0, 3)
        y = a.run(u, time_major=True)
        plain = raw(a)
        for P in periods:
            b = arm().set_measurement_fold(P)
            b.measure(u, time_major=True)
            with_fold = raw(b)
            assert with_fold[1] == plain[1] and np.array_equal(with_fold[0], plain[0]), (name, P)
            assert_fold(got_fold(b), window(y, start, 0), P)


# ---- 4. paths -----------------------------------------------------------------------------------------------------------------
PATH_START, PATH_PERIOD = 1203, 441


def check_paths(mk, dev, k, T, monkeypatch, N=70, P=PATH_PERIOD, S=PATH_START, wire=False):
    """one fold, H = 10, the diode clipper driven by what a per-instance sine source renders: the fold and the measurement read
    after every path == those after a host run with y stored.  ``dev``: the device-memory calls (put, run(r, u, keep, T)).
    ``wire``: the pass-through model on data of the test's choosing; the source, a sine of P samples' period, then has a
    reference run of its own on what it renders."""
    from fractions import Fraction
    from acme_jl_amd import examples
    from acme_jl_amd.model import DiscreteModel
    H = 10
    if wire:
        m = X.wire_model(1, k * FS)
        src = dict(kind="sine", f_den=3 * P, f_num=np.full(N, 3 if P > 1 else 0), amp=np.logspace(-2, 0.7, N),
                   phase=(1 + np.arange(N)) % (3 * P))          # (P = 1: the constant sin(phase))
    else:
        m = clipper() if k == 1 else DiscreteModel(examples.diodeclipper(), Fraction(1, k * FS), HS)
        src = dict(kind="sine", f_den=441, f_num=np.full(N, 10), amp=np.logspace(-2, 0.7, N))

    def fresh(sourced=False):
        r = mk(m, N).set_oversampling(k)
        if sourced and wire:            # (the measurement's fundamental stays 10 / 441: 3 / (3 P) is none below P = 3)
            r = sr.apply_sources(r, [src]).set_measurement(start=S, f0=(10, 441), harmonics=H)
            return r.set_measurement_fold(period_from_source=0)
        if sourced:
            r = sr.apply_sources(r, [src]).set_measurement(start=S, harmonics=H, f0_from_source=0)
            return r.set_measurement_fold(period_from_source=0)
        return r.set_measurement(start=S, f0=(10, 441), harmonics=H).set_measurement_fold(P)

    def read(r):
        return got_fold(r) + raw(r)
    us = sr.apply_sources(mk(m, N).set_oversampling(k), [src]).render_sources(T)
    u = X.scaled_rows(np.random.default_rng(P + k), N, T, 1) if wire else us
    r = fresh()
    y = r.run(u, time_major=True)
    ref = read(r)
    assert np.isfinite(y).all()
    assert_fold(ref[:4], window(y, S, 0), P)
    results = {"y NULL": read(fresh().measure(u, time_major=True))}
    # split calls: before the start, on a period's first sample, inside a period, on a chunk boundary
    cuts = sorted({c for c in (min(1000, S - 2), S + P, S + P + 40, S + P // 2 + 1, S + 4096) if 0 < c < T})
    assert len(cuts) >= 3
    r = fresh()
    for j, (a, b) in enumerate(zip([0] + cuts, cuts + [T])):
        part = np.ascontiguousarray(u[:, a:b])
        if j % 2:
            r.measure(part, time_major=True)
        else:
            assert np.array_equal(r.run(part, time_major=True), y[:, a:b])
    results["split"] = read(r)
    ud = dev.put(u)
    r = fresh()
    assert np.array_equal(dev.run(r, ud, True, T), y)
    results["device"] = read(r)
    r = fresh()
    dev.run(r, ud, False, T)
    results["device, y NULL"] = read(r)
    r = fresh()
    t1 = cuts[-1]
    dev.run(r, dev.put(u[:, :t1]), False, t1)
    dev.run(r, dev.put(u[:, t1:]), False, T - t1)
    results["device, y NULL, split"] = read(r)
    r = fresh()
    ya = np.zeros_like(y)
    r.run_async(u, ya)
    r.wait()
    assert np.array_equal(ya, y)
    results["async"] = read(r)
    r = fresh()
    r.run_async(u, None)
    r.wait()
    results["async, y NULL"] = read(r)
    r = fresh(sourced=True)
    if wire:                            # the source's own signal: run_sources == run on what it renders
        q = fresh()
        ys = q.run(us, time_major=True)
        assert np.array_equal(r.run_sources(T), ys) and np.array_equal(got_fold(r)[2], np.full(N, P))
        assert_fold(got_fold(r), window(ys, S, 0), P)
        for got in (read(r), read(fresh(sourced=True).measure(T=T))):
            assert same_fold(got[:4], read(q)[:4]) and np.array_equal(got[4], read(q)[4]) and got[5] == read(q)[5]
    else:
        assert np.array_equal(r.run_sources(T), y)
        results["sources"] = read(r)
        results["sources, y NULL"] = read(fresh(sourced=True).measure(T=T))
    monkeypatch.setenv("ACME_OS_SLICE", "150")
    results["slices of 150"] = read(fresh().measure(u, time_major=True))
    r = fresh()
    assert np.array_equal(r.run(u, time_major=True), y)
    results["slices of 150, y stored"] = read(r)
    monkeypatch.delenv("ACME_OS_SLICE")
    for name, got in results.items():
        assert got[3] == ref[3] and got[5] == ref[5], name
        assert same_fold(got[:3], ref[:3]) and np.array_equal(got[4], ref[4]), name
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
        assert same_fold(got_fold(q), got_fold(r))
    # chunks of one tile (the per-instance form under a table budget of one byte), the calls cut again
    f_num = 1 + np.arange(N)

    def pi():
        return mk(m, N).set_measurement(start=S, f_den=441, f_num=f_num, harmonics=H).set_measurement_fold(P)
    monkeypatch.setenv("ACME_MEAS_TABLE_BUDGET", "1")
    b = pi()
    assert b.measurement_plan()["chunk"] == 64
    b.measure(np.ascontiguousarray(u[:, :t1]), time_major=True)
    b.measure(np.ascontiguousarray(u[:, t1:]), time_major=True)
    monkeypatch.delenv("ACME_MEAS_TABLE_BUDGET")
    assert same_fold(got_fold(b), ref[:4])


# ---- 6. exact pins on the pass-through model ----------------------------------------------------------------------------------
def order_dependent_rows(rng, N, T):
    """data [N, T, 1] with magnitudes spread over 2^40 from sample to sample: a slot's sum depends on the order"""
    return rng.standard_normal((N, T, 1)) * 2.0 ** rng.integers(0, 41, (N, T, 1))


def check_exact(mk, N, P, T, lead=0, start=37):
    """the fold of data of the test's choosing through y = u: == the forward chain, which a reversed chain is not.  ``lead``
    samples of zeros are fed first, in calls of at most 2^18, and the window starts ``start`` samples into the data"""
    u = order_dependent_rows(np.random.default_rng(P + N), N, T)
    yw = u[:, start:]
    fwd = fold_sums(np.ascontiguousarray(yw.transpose(1, 0, 2)), P)[0]
    rev = np.zeros_like(fwd)
    for k in reversed(range(0, yw.shape[1], P)):                              # the same samples per slot, last first
        seg = yw[:, k:k + P].transpose(1, 0, 2)
        rev[:len(seg)] += seg
    assert (fwd != rev).any(), "the chosen data does not pin the order"
    r = mk(X.wire_model(1, FS), N).set_measurement(start=lead + start).set_measurement_fold(P)
    z = np.zeros((N, min(lead, 2 ** 18), 1))
    for a in range(0, lead, 2 ** 18):
        r.measure(z[:, :min(2 ** 18, lead - a)], time_major=True)
    assert np.array_equal(r.run(u, time_major=True), u)
    assert_fold(got_fold(r), yw, P)


# ---- 7. use level -------------------------------------------------------------------------------------------------------------
def check_bode(mk):
    """sallenkey, one instance per frequency k / 441, the fold of three periods behind BODE_START: line k of the folded period
    against the armed measurement's A_1.  Both are sums of the same count = n products y e^{-j th}: each lies within
    (n + 16) 2^-53 sum|y| of the exact correlation (exact_ref.harmonic_bound; the fold adds at most three samples and one
    division per slot before its DFT, which is evaluated in long double here), so the two amplitudes, scaled by 2 / count,
    differ by at most 2 (n + 16) 2^-53 sum|y| 2 / count.  Returns the worst |error| / bound."""
    m = load("sallenkey")
    P, f_num = 441, np.arange(1, 221)
    S, n = PI.BODE_START["sallenkey"], 3 * 441
    r = mk(m, len(f_num))
    r.set_source(0, "sine", f_den=P, f_num=f_num)
    r.set_measurement(start=S, length=n, harmonics=1, f0_from_source=0).set_measurement_fold(P)
    y = r.run_sources(S + n + 50)                               # (the samples behind the window are not measured)
    f, a1 = r.measurement_fold(), r.measurement().harmonics[:, 0, 0]
    assert f.count == n and (f.period == P).all() and f.mean.shape == (len(f_num), 1, P)
    l1 = np.abs(y[:, S:S + n, 0]).sum(axis=1)
    two_pi = 2 * np.arccos(np.longdouble(-1))
    worst = 0.0
    for i, k in enumerate(f_num):
        th = two_pi * ((int(k) * np.arange(P)) % P).astype(np.longdouble) / P
        x = f.mean[i, 0].astype(np.longdouble)
        line = complex((x * np.cos(th)).sum() * 2 / P, -(x * np.sin(th)).sum() * 2 / P)
        bound = 2 * X.harmonic_bound(n, l1[i]) * 2 / n
        worst = max(worst, abs(line - a1[i]) / bound)
        # spectrum() is numpy's double FFT of the same period: its own rounding, a few log2(P) ulps of sum|mean| 2 / P
        assert abs(f.spectrum(i)[k] - line) <= 64 * X.U * np.abs(f.mean[i, 0]).sum() * 2 / P, k
    assert np.array_equal(f.spectrum(0)[0], np.fft.rfft(f.mean[0, 0])[0] / P)       # the DC line is the mean
    return worst


# ---- 8. life cycle and errors -------------------------------------------------------------------------------------------------
def check_life_cycle(mk, N=5, T=700, P=64, start=9):
    from acme_jl_amd.runner import AcmeError
    m, u = clipper(), clipper_u(N, T)
    arm = lambda: mk(m, N).set_measurement(start=start, f0=(10, 441), harmonics=3)
    # reset zeroes the fold and keeps the periods
    per = np.array([P, 7, P, 100, 1][:N])
    r = arm().set_measurement_fold(per)
    r.measure(u, time_major=True)
    r.reset_measurement()
    zero = r.measurement_fold()
    assert zero.count == 0 and np.array_equal(zero.period, per) and np.isnan(zero.mean).all()
    q = mk(m, N)
    q.run(u, time_major=True)                               # (the same state as r's at its reset)
    q.set_measurement(start=start, f0=(10, 441), harmonics=3).set_measurement_fold(per)
    u2 = np.ascontiguousarray(u[:, :300])
    r.measure(u2, time_major=True)
    q.measure(u2, time_major=True)
    assert same_fold(got_fold(r), got_fold(q)) and got_fold(r)[3] == 300 - start
    # a fold set again replaces the earlier one (after a reset: nothing has been fed)
    r.reset_measurement().set_measurement_fold(5)
    assert r.measurement_fold().mean.shape == (N, 1, 5)
    # re-arming and clear remove it
    r.set_measurement(start=start, f0=(10, 441), harmonics=3)
    with pytest.raises(AcmeError, match="no measurement fold"):
        r.measurement_fold()
    L = r.lib.L
    assert L.acme_batch_get_measurement_fold(r.h, None, None, None) == -1 and "no measurement fold" in L.acme_last_error().decode()
    r.set_measurement_fold(P).clear_measurement()
    assert L.acme_batch_get_measurement_fold(r.h, None, None, None) == -1 and "no measurement fold" in L.acme_last_error().decode()
    with pytest.raises(AcmeError, match="no measurement is armed"):
        r.set_measurement_fold(P)


def check_set_matrices_carries_the_fold(mk):
    from helpers import sweep_inputs
    from test_emu_parity import superover_models_with_their_own_diodes
    models = superover_models_with_their_own_diodes(3, HS)
    u = np.ascontiguousarray(sweep_inputs("superover_var", 3, 60, seed=2).transpose(0, 2, 1))
    r = mk(models[0], 3, models=[models[0]] * 3).set_measurement(start=10, f0=(1, 30), harmonics=3).set_measurement_fold([7, 30, 11])
    ya = r.run(np.ascontiguousarray(u[:, :25]), time_major=True)
    r.set_models(1, [models[0]])
    r.set_models(2, [models[2]])                            # (the batch moves to the plain shape: a new batch takes the measurement over)
    yb = r.run(np.ascontiguousarray(u[:, 25:]), time_major=True)
    assert_fold(got_fold(r), window(np.concatenate([ya, yb], axis=1), 10, 0), [7, 30, 11])


def check_errors(mk):
    """every refusal with its code and the argument's name in the message"""
    from acme_jl_amd.runner import AcmeError
    m, u = clipper(), clipper_u(3, 10)
    lp = C.POINTER(C.c_longlong)

    def refused(r, code, what, period, period_i=None):
        a = None if period_i is None else np.asarray(period_i, dtype=np.int64)
        rc = r.lib.L.acme_batch_set_measurement_fold(r.h, period, None if a is None else a.ctypes.data_as(lp))
        msg = r.lib.L.acme_last_error().decode()
        assert rc == code and all(w in msg for w in what), (period, period_i, rc, msg)
    r = mk(m, 3)
    refused(r, -1, ["no measurement is armed"], 4)
    r.set_measurement(start=1)
    for bad in (0, -3, CAP + 1):
        refused(r, -1, ["period", str(CAP)], bad)
    refused(r, -1, ["period_i", "instance 1", str(CAP)], 4, [4, 0, 4])
    refused(r, -1, ["period_i", "instance 2", str(CAP)], 4, [4, CAP, CAP + 1])
    assert r.lib.L.acme_batch_get_measurement_fold(r.h, None, None, None) == -1      # (a refused fold leaves none behind)
    r.measure(u, time_major=True)
    refused(r, -1, ["samples have been fed"], 4)
    r.reset_measurement()
    r.set_measurement_fold(np.array([4, 1, CAP]))           # (`period` is ignored beside period_i; the cap itself is accepted)
    assert r.measurement_fold().mean.shape == (3, 1, CAP)
    # a series and a fold exclude each other, whichever is set first
    assert r.lib.L.acme_batch_set_measurement_series(r.h, 4, 4, 2) == -2 and "fold" in r.lib.L.acme_last_error().decode()
    with pytest.raises(AcmeError, match="fold"):
        r.set_measurement_series(4, 4, 2)
    r.set_measurement(start=1).set_measurement_series(4, 4, 2)
    refused(r, -2, ["series"], 4)
    # the Python layer's own refusals
    r.set_measurement(start=1)
    with pytest.raises(ValueError):
        r.set_measurement_fold()
    with pytest.raises(ValueError):
        r.set_measurement_fold(4, period_from_source=0)
    with pytest.raises(ValueError, match="no sine or multisine source"):
        r.set_measurement_fold(period_from_source=0)
    r.set_source(0, "sine", f_den=2 ** 31 - 1, f_num=[1, 2, 3])
    with pytest.raises(ValueError, match="exceeds 65536"):
        r.set_measurement_fold(period_from_source=0)
    r.set_source(0, "multisine", f_den=44100, f_num=np.array([[1000, 300, 0], [1500, 441, 0]]))
    r.set_measurement_fold(period_from_source=0)
    assert r.measurement_fold().period.tolist() == [441, 14700, 1]      # the least common multiple over the tones


def check_no_fold_invariance(mk, N, T):
    """a batch armed without a fold, and one armed after a fold has been set and removed: the results and the run kernel's
    launches of the existing forms"""
    m, u = clipper(), clipper_u(N, T)
    f_num = np.array([10, 20, 30])[np.arange(N) % 3]
    arms = {"shared": lambda r: r.set_measurement(start=5, f0=(10, 441), harmonics=10),
            "per instance": lambda r: r.set_measurement(start=5, f_den=441, f_num=f_num, harmonics=10),
            "bins": lambda r: r.set_measurement_bins(np.array([[1], [2], [3]]), start=5, f_den=441, f_num=f_num[None])}
    for name, arm in arms.items():
        a = arm(mk(m, N))
        y = a.run(u, time_major=True)
        b = arm(mk(m, N)).set_measurement_fold(441)
        arm(b)                                              # (arming removes the fold)
        assert np.array_equal(b.run(u, time_major=True), y)
        c = arm(mk(m, N)).set_measurement_fold(441).clear_measurement()
        arm(c)
        assert np.array_equal(c.run(u, time_major=True), y)
        d = arm(mk(m, N)).set_measurement_fold(441)         # ... and with the fold the run kernel's launches are the same
        assert np.array_equal(d.run(u, time_major=True), y)
        (oa, ca), (ob, cb), (oc, cc), (od, cd) = raw(a), raw(b), raw(c), raw(d)
        assert ca == cb == cc == cd == T - 5, name
        assert np.array_equal(oa, ob) and np.array_equal(oa, oc) and np.array_equal(oa, od), name
        assert a.kernel_time()[1] == b.kernel_time()[1] == c.kernel_time()[1] == d.kernel_time()[1] > 0, name
        for q in (b, c):
            assert q.lib.L.acme_batch_get_measurement_fold(q.h, None, None, None) == -1
