"""Shared by the emulator and GPU tests of the measurement target (acme_batch_set_measurement_target): the reference every
target is held to -- numpy on the stored y of an identical run without a target, every chain a sequential float64
accumulation (np.add.accumulate) with every product rounded on its own -- and the checks, each taking ``mk(model, n)``, which
makes a fresh runner on the library under test (the emulator's or the GPU's).  The seven chains
(``measurement_target(raw=True).sums``) are compared with ``==``."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest

import exact_ref as X
import source_ref as sr
from helpers import FS, HS
from test_measurement import clipper, raw, two_output_clipper

CAP = 16777216              # ACME_MAX_SOURCE_TABLE
MAX_TARGETS = 64
# the target lengths of the geometry, with start = 301 and T = 9000: below, at and above a tile (64) and a chunk (4096) -- a
# wrap inside a chunk and across one --, and one longer than the run
GEOMETRY = [1, 5, 63, 64, 65, 4095, 4096, 4099, 9001]
C_PATHS = 0.95              # a lost or stale e_prev / t_prev at any boundary shows


def _seq_sum(a):
    """[N, count, nrows] -> [N, nrows]: the sums along axis 1, added one after the other from 0.0"""
    if a.shape[1] == 0:
        return np.zeros((a.shape[0], a.shape[2]))
    return np.add.accumulate(a, axis=1)[:, -1]


def replay(yw, tgt, which=None, lag=None, c=0.0):
    """the contract on the window's samples yw [N, count, nrows] and the table tgt [K, nrows, P]: [N, nrows, 7] in the order
    See, Stt, Syt, St, emax, Pee, Ptt"""
    N, count, nrows = yw.shape
    K, nr, P = tgt.shape
    assert nr == nrows
    which = np.broadcast_to(np.asarray(0 if which is None else which, dtype=np.int64), (N,))
    lag = np.broadcast_to(np.asarray(0 if lag is None else lag, dtype=np.int64), (N,))
    s = (np.arange(count, dtype=np.int64)[None, :] + lag[:, None]) % P              # [N, count]
    t = tgt[which[:, None, None], np.arange(nrows)[None, None, :], s[:, :, None]]   # [N, count, nrows]
    e = yw - t
    ep, tp = np.zeros_like(e), np.zeros_like(t)
    ep[:, 1:], tp[:, 1:] = e[:, :-1], t[:, :-1]
    with np.errstate(invalid="ignore", over="ignore"):
        de, dt = e - c * ep, t - c * tp
        ae = np.abs(e)
        emax = np.where(np.isnan(ae).any(axis=1), np.nan, ae.max(axis=1, initial=0.0))
        out = [_seq_sum(e * e), _seq_sum(t * t), _seq_sum(yw * t), _seq_sum(t), emax, _seq_sum(de * de), _seq_sum(dt * dt)]
    return np.stack(out, axis=2)


def got_target(r):
    """(sums [N, nrows, 7], count) of the runner's target"""
    a = r.measurement_target(raw=True)
    return a.sums, a.count


def assert_target(got, yw, tgt, which=None, lag=None, c=0.0):
    sums, count = got
    assert count == yw.shape[1] and sums.shape == (yw.shape[0], yw.shape[2], 7), (count, sums.shape, yw.shape)
    want = replay(yw, tgt, which, lag, c)
    assert np.array_equal(sums, want, equal_nan=True), np.argwhere(~((sums == want) | (np.isnan(sums) & np.isnan(want))))[:6]
    return sums


def same(a, b):
    return a[1] == b[1] and np.array_equal(a[0], b[0], equal_nan=True)


def window(y, start, length, rows=None):
    """the measured samples of the stored y [N, T, ny]: [N, count, nrows]"""
    end = y.shape[1] if not length else min(y.shape[1], start + length)
    return y[:, start:end][:, :, list(range(y.shape[2])) if rows is None else rows]


def table(seed, K, nrows, P):
    return np.random.default_rng(seed).standard_normal((K, nrows, P)) * 3.0


def wire_data(N, T, seed=0):
    return X.wire_model(1, FS), X.scaled_rows(np.random.default_rng(1000 + seed + N), N, T, 1)


# ---- 1. exact pins: integers, every product and sum exact ---------------------------------------------------------------------
def check_exact_pins(mk, case, N=5, T=4000):
    """y = u small integers through the pass-through model, c = 0.5: the seven values from Python integers (fractions for the
    pre-emphasised pair, whose terms are multiples of 1/4), independent of any replay order"""
    rng = np.random.default_rng(11)
    ui = rng.integers(-1024, 1025, (N, T))
    ti = {"t = u": ui, "t = 0": np.zeros((N, 1), dtype=np.int64), "t = -u": -ui}[case]
    r = mk(X.wire_model(1, FS), N).set_measurement()
    r.set_measurement_target(ti.astype(np.float64)[:, None, :], which=np.arange(N), preemphasis=0.5)
    u = np.ascontiguousarray(ui.astype(np.float64)[:, :, None])
    assert np.array_equal(r.run(u, time_major=True), u)
    sums, count = got_target(r)
    assert count == T
    half = Fraction(1, 2)
    for i in range(N):
        y = [int(v) for v in ui[i]]
        t = [int(ti[i, m % ti.shape[1]]) for m in range(T)]
        e = [a - b for a, b in zip(y, t)]
        de = [e[m] - half * (e[m - 1] if m else 0) for m in range(T)]
        dt = [t[m] - half * (t[m - 1] if m else 0) for m in range(T)]
        want = [sum(v * v for v in e), sum(v * v for v in t), sum(a * b for a, b in zip(y, t)), sum(t), max(abs(v) for v in e),
                sum(v * v for v in de), sum(v * v for v in dt)]
        assert all(abs(w) < 2 ** 52 for w in want)
        assert sums[i, 0].tolist() == [float(w) for w in want], (case, i, sums[i, 0], want)
    if case == "t = u":
        assert not sums[:, 0, [0, 4, 5]].any()             # See, emax, Pee: 0.0 exactly


# ---- 2. geometry of P against the chunk and the tile, 4. rows -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plain_run(mk, two, N, T, start, length, rows):
    """the run without a target every geometry case of a shape shares: (model, u, y, raw measurement); never modified"""
    if two:
        from test_measurement import clipper_u
        m, u = two_output_clipper(), clipper_u(N, T)
    else:
        m, u = wire_data(N, T)
    r = mk(m, N).set_measurement(start=start, length=length, rows=None if rows is None else list(rows))
    y = r.run(u, time_major=True)
    return m, u, y, raw(r)


def check_geometry(mk, N, T, start, P, lags, length=0, rows=None, two=False):
    """``lags``: each entry one run -- an int, the shared lag, or "per instance": the lags 0, 1, P - 1 dealt out in turn"""
    m, u, y, plain = _plain_run(mk, two, N, T, start, length, None if rows is None else tuple(rows))
    yw = window(y, start, length, rows)
    tgt = table(P, 1, yw.shape[2], P)
    for lag in lags:
        la = np.array([0, 1 % P, P - 1])[np.arange(N) % 3] if isinstance(lag, str) else lag % P
        r = mk(m, N).set_measurement(start=start, length=length, rows=rows).set_measurement_target(tgt, lag=la, preemphasis=C_PATHS)
        r.measure(u, time_major=True)
        with_target = raw(r)
        assert with_target[1] == plain[1] and np.array_equal(with_target[0], plain[0])  # the measurement's own results
        assert_target(got_target(r), yw, tgt, None, la, C_PATHS)
    return yw.shape[1]


# ---- 3. per-instance which and lag ---------------------------------------------------------------------------------------------
def check_per_instance(mk, N, T, start=3, P=37, K=3, one_tuple=False, shared=None):
    """one batch with (which, lag) per instance -- the first 64 instances share a tuple (a uniform wave), the others do not --:
    the numpy reference, and each instance == the shared arming at its own tuple (``shared``: at most so many of the distinct
    tuples -- the emulator's time).  ``one_tuple``: every instance the same tuple, handed over per instance"""
    m, u = wire_data(N, T)
    tgt = table(N, K, 1, P)
    if one_tuple:
        which, lag = np.full(N, 2), np.full(N, 5)
    else:
        which, lag = np.arange(N) % K, np.array([0, 5, P - 1, 5])[np.arange(N) % 4]
        which[:64], lag[:64] = 1, 5
    arm = lambda: mk(m, N).set_measurement(start=start)
    r = arm().set_measurement_target(tgt, which=which, lag=lag, preemphasis=C_PATHS)
    y = r.run(u, time_major=True)
    got = got_target(r)
    assert_target(got, window(y, start, 0), tgt, which, lag, C_PATHS)
    tuples = sorted(set(zip(which.tolist(), lag.tolist())))
    if shared is not None and len(tuples) > shared:
        tuples = [tuples[k] for k in np.linspace(0, len(tuples) - 1, shared).round().astype(int)]
    for w, l in tuples:
        q = arm().set_measurement_target(tgt, which=w, lag=l, preemphasis=C_PATHS)
        q.measure(u, time_major=True)
        alone, idx = got_target(q), np.flatnonzero((which == w) & (lag == l))
        assert alone[1] == got[1] and np.array_equal(got[0][idx], alone[0][idx]), (w, l)


# ---- 5. paths -----------------------------------------------------------------------------------------------------------------
def check_paths(mk, dev, k, T, monkeypatch, N=70, P=97, S=3):
    """the pass-through model driven by what a per-instance sine source renders, oversampled by k: the target and the
    measurement read after every path == those after a host run with y stored.  ``dev``: the device-memory calls
    (put, run(r, u, keep, T))"""
    m = X.wire_model(1, k * FS)
    src = dict(kind="sine", f_den=441, f_num=1 + np.arange(N) % 40, amp=np.logspace(-2, 0.7, N), phase=np.arange(N) % 441)
    tgt = table(P + k, 2, 1, P)
    which, lag = np.arange(N) % 2, (7 * np.arange(N)) % P
    which[:64], lag[:64] = 1, 11 % P

    def fresh(sourced=False, pi=False):
        r = mk(m, N).set_oversampling(k)
        if sourced:
            r = sr.apply_sources(r, [src])
        if pi:      # (the per-instance form: its table's budget sets the chunk length)
            r.set_measurement(start=S, f_den=441, f_num=1 + np.arange(N), harmonics=2)
        else:
            r.set_measurement(start=S)
        return r.set_measurement_target(tgt, which=which, lag=lag, preemphasis=C_PATHS)

    def read(r):
        return got_target(r)
    u = sr.apply_sources(mk(m, N).set_oversampling(k), [src]).render_sources(T)
    r = fresh()
    y = r.run(u, time_major=True)
    ref = read(r)
    assert np.isfinite(y).all()
    assert_target(ref, window(y, S, 0), tgt, which, lag, C_PATHS)
    results = {"y NULL": read(fresh().measure(u, time_major=True))}
    # split calls: before the start, on a wrap of the target, inside a period, on a tile and on a chunk boundary
    for cut in sorted({c for c in (S - 1, S + P, S + P + 40, S + 64, S + 150, S + 4096) if 0 < c < T}):
        r = fresh()
        assert np.array_equal(r.run(np.ascontiguousarray(u[:, :cut]), time_major=True), y[:, :cut])
        r.measure(np.ascontiguousarray(u[:, cut:]), time_major=True)
        results[f"split at {cut}"] = read(r)
    t1 = min(S + P + 40, T - 1)
    ud = dev.put(u)
    r = fresh()
    assert np.array_equal(dev.run(r, ud, True, T), y)
    results["device"] = read(r)
    r = fresh()
    dev.run(r, ud, False, T)
    results["device, y NULL"] = read(r)
    r = fresh()
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
    assert np.array_equal(r.run_sources(T), y)
    results["sources"] = read(r)
    results["sources, y NULL"] = read(fresh(sourced=True).measure(T=T))
    monkeypatch.setenv("ACME_OS_SLICE", "150")
    results["slices of 150"] = read(fresh().measure(u, time_major=True))
    r = fresh()
    assert np.array_equal(r.run(u, time_major=True), y)
    results["slices of 150, y stored"] = read(r)
    # ... with chunks of one tile (the per-instance form under a table budget of one byte), the calls cut again
    monkeypatch.setenv("ACME_MEAS_TABLE_BUDGET", "1")
    b = fresh(pi=True)
    assert b.measurement_plan()["chunk"] == 64
    b.measure(np.ascontiguousarray(u[:, :t1]), time_major=True)
    b.measure(np.ascontiguousarray(u[:, t1:]), time_major=True)
    results["slices of 150, chunks of one tile, split"] = read(b)
    monkeypatch.delenv("ACME_MEAS_TABLE_BUDGET")
    monkeypatch.delenv("ACME_OS_SLICE")
    for name, got in results.items():
        assert same(got, ref), name
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
        assert same(read(q), read(r))


# ---- 6. c = 0, and a reset zeroes the carries ---------------------------------------------------------------------------------
def check_c_zero_and_reset(mk, N, T, P=50):
    m, u = wire_data(N, T)
    tgt = table(6, 1, 1, P)
    r = mk(m, N).set_measurement(start=2).set_measurement_target(tgt, lag=3, preemphasis=0.0)
    r.measure(u, time_major=True)
    s, _ = got_target(r)
    assert np.array_equal(s[:, :, 5], s[:, :, 0]) and np.array_equal(s[:, :, 6], s[:, :, 1]) and s[:, :, 0].all()
    r = mk(m, N).set_measurement(start=2).set_measurement_target(tgt, lag=3, preemphasis=C_PATHS)
    y = r.run(u, time_major=True)                          # (the pass-through model has no state: a rerun repeats y)
    first = assert_target(got_target(r), window(y, 2, 0), tgt, None, 3, C_PATHS)
    assert (first[:, :, 5] != first[:, :, 0]).all()
    r.reset_measurement()
    zero = got_target(r)
    assert zero[1] == 0 and not zero[0].any()               # a window nothing has reached: 0.0 sums, count 0
    r.measure(u, time_major=True)
    assert same(got_target(r), (first, T - 2))              # table, which, lag and c kept; chains and carries from 0.0


# ---- 7. coexistence ------------------------------------------------------------------------------------------------------------
def check_coexistence(mk, N, T, start=5):
    m, u = wire_data(N, T)
    tgt = table(9, 2, 1, 77)
    which, lag = np.arange(N) % 2, np.arange(N) % 77
    arm = lambda: mk(m, N).set_measurement(start=start, f0=(10, 441), harmonics=3)
    adds = {"fold": lambda r: r.set_measurement_fold(50), "spectrum": lambda r: r.set_measurement_spectrum(64, 32),
            "cross": lambda r: r.set_measurement_cross(0, 64, 32),
            "target": lambda r: r.set_measurement_target(tgt, which=which, lag=lag, preemphasis=C_PATHS)}
    reads = {"fold": lambda r: r.measurement_fold(raw=True).mean, "spectrum": lambda r: r.measurement_spectrum(raw=True).power,
             "cross": lambda r: np.stack([r.measurement_cross(raw=True).sxx, r.measurement_cross(raw=True).syy,
                                          r.measurement_cross(raw=True).sxy.real, r.measurement_cross(raw=True).sxy.imag]),
             "target": lambda r: got_target(r)[0]}
    base = arm()
    base.measure(u, time_major=True)
    every = arm()
    for add in adds.values():
        add(every)
    every.measure(u, time_major=True)
    assert raw(every)[1] == raw(base)[1] and np.array_equal(raw(every)[0], raw(base)[0])
    for name, add in adds.items():
        alone = add(arm())
        alone.measure(u, time_major=True)
        assert np.array_equal(reads[name](alone), reads[name](every), equal_nan=True), name
        assert np.array_equal(raw(alone)[0], raw(base)[0]), name


# ---- 8. use level --------------------------------------------------------------------------------------------------------------
def check_use_level(mk, N=16, T=2100, best=7, shift=37):
    """the diode clipper at N levels: the target is one instance's recorded output, rotated and taken back by the lag"""
    m = clipper()
    src = dict(kind="sine", f_den=441, f_num=np.full(N, 10), amp=np.logspace(-1, 0.7, N))
    y = sr.apply_sources(mk(m, N), [src]).run_sources(T)
    r = sr.apply_sources(mk(m, N), [src]).set_measurement()
    r.set_measurement_target(np.roll(y[best, :, 0], shift), lag=shift, preemphasis=C_PATHS)     # tgt[(m + shift) mod T] = y[m]
    r.measure(T=T)
    mt = r.measurement_target()
    assert mt.count == T and mt.see[best, 0] == 0.0 and mt.emax[best, 0] == 0.0 and mt.pee[best, 0] == 0.0
    others = np.arange(N) != best
    assert (mt.see[others, 0] > 0).all() and int(np.argmin(mt.esr[:, 0])) == best
    assert (np.diff(mt.gain[:, 0]) > 0).all() and mt.gain[best, 0] == 1.0
    assert mt.null_db[best, 0] == -np.inf and np.array_equal(mt.error_peak, mt.emax)
    assert_target((mt.sums, mt.count), y, np.roll(y[best, :, 0], shift)[None, None, :], None, shift, C_PATHS)
    # error_mean: the mean of y - t, within the rounding of two sums of T terms
    em = (y[:, :, 0] - y[best, :, 0][None]).mean(axis=1)
    assert np.allclose(mt.error_mean[:, 0], em, rtol=0, atol=4 * T * X.U * np.abs(y).max())
    assert np.allclose(mt.error_rms[:, 0], np.sqrt(mt.see[:, 0] / T), rtol=1e-15, atol=0)
    return mt


# ---- 9. life cycle and errors --------------------------------------------------------------------------------------------------
def check_life_cycle(mk, N=5, T=300, P=40, start=9):
    from acme_jl_amd.runner import AcmeError
    m, u = wire_data(N, T)
    tgt = table(3, 2, 1, P)
    which, lag = np.arange(N) % 2, np.arange(N) % P
    r = mk(m, N).set_measurement(start=start).set_measurement_target(tgt, which=which, lag=lag, preemphasis=0.5)
    y = r.run(u, time_major=True)
    assert_target(got_target(r), window(y, start, 0), tgt, which, lag, 0.5)
    # a target set again replaces the earlier one (after a reset: nothing has been fed)
    t2 = table(4, 1, 1, 7)
    r.reset_measurement().set_measurement_target(t2, preemphasis=0.25)
    r.measure(u, time_major=True)
    assert_target(got_target(r), window(y, start, 0), t2, None, None, 0.25)
    # re-arming and clear remove it
    L = r.lib.L
    r.set_measurement(start=start)
    with pytest.raises(AcmeError, match="no measurement target"):
        r.measurement_target()
    assert L.acme_batch_get_measurement_target(r.h, None, None) == -1 and "no measurement target" in L.acme_last_error().decode()
    r.set_measurement_target(t2).clear_measurement()
    assert L.acme_batch_get_measurement_target(r.h, None, None) == -1 and "no measurement target" in L.acme_last_error().decode()
    with pytest.raises(AcmeError, match="no measurement is armed"):
        r.set_measurement_target(t2)


def check_set_matrices_carries_the_target(mk):
    from helpers import sweep_inputs
    from test_emu_parity import superover_models_with_their_own_diodes
    models = superover_models_with_their_own_diodes(3, HS)
    u = np.ascontiguousarray(sweep_inputs("superover_var", 3, 60, seed=2).transpose(0, 2, 1))
    r = mk(models[0], 3, models=[models[0]] * 3).set_measurement(start=10)
    nrows = len(r._meas[1])
    tgt, which, lag = table(8, 2, nrows, 13), [0, 1, 1], [0, 12, 5]
    r.set_measurement_target(tgt, which=which, lag=lag, preemphasis=C_PATHS)
    ya = r.run(np.ascontiguousarray(u[:, :25]), time_major=True)
    r.set_models(1, [models[0]])
    r.set_models(2, [models[2]])                            # (the batch moves to the plain shape: a new batch takes the measurement over)
    yb = r.run(np.ascontiguousarray(u[:, 25:]), time_major=True)
    assert_target(got_target(r), window(np.concatenate([ya, yb], axis=1), 10, 0), tgt, which, lag, C_PATHS)


def check_errors(mk):
    """every refusal with its code and the argument's name in the message"""
    from acme_jl_amd.runner import AcmeError, _dp, _ip
    m, u = wire_data(3, 10)
    lp = C.POINTER(C.c_longlong)
    big = np.zeros(CAP)

    def refused(r, code, what, t, K, P, which=None, lag=None, c=0.0):
        wa = None if which is None else np.asarray(which, dtype=np.int32)
        la = None if lag is None else np.asarray(lag, dtype=np.int64)
        rc = r.lib.L.acme_batch_set_measurement_target(r.h, None if t is None else _dp(t), K, P, None if wa is None else _ip(wa),
                                                       None if la is None else la.ctypes.data_as(lp), c)
        msg = r.lib.L.acme_last_error().decode()
        assert rc == code and all(w in msg for w in what), (K, P, which, lag, c, rc, msg)
    t = np.arange(8.0)
    r = mk(m, 3)
    refused(r, -1, ["no measurement is armed"], t, 1, 8)
    r.set_measurement(start=1)
    refused(r, -1, ["t is null"], None, 1, 8)
    for K in (0, -1, MAX_TARGETS + 1):
        refused(r, -1, ["K", str(MAX_TARGETS)], big, K, 1)
    for P in (0, -5):
        refused(r, -1, ["P"], t, 1, P)
    refused(r, -1, ["K nrows P", str(CAP)], big, 1, CAP + 1)
    refused(r, -1, ["K nrows P", str(CAP)], big, 64, CAP // 64 + 1)
    for bad in (np.nan, np.inf, -np.inf):
        tb = t.copy()
        tb[5] = bad
        refused(r, -1, ["t[5]", "not finite"], tb, 2, 4)
    refused(r, -1, ["which", "instance 1"], t, 2, 4, which=[0, 2, 1])
    refused(r, -1, ["which", "instance 2"], t, 2, 4, which=[0, 1, -1])
    refused(r, -1, ["lag", "instance 0"], t, 2, 4, lag=[4, 0, 0])
    refused(r, -1, ["lag", "instance 2"], t, 2, 4, lag=[3, 0, -1])
    for c in (-0.1, 1.0, 1.5, np.nan, np.inf):
        refused(r, -1, ["preemph"], t, 2, 4, c=c)
    assert r.lib.L.acme_batch_get_measurement_target(r.h, None, None) == -1     # (a refused target leaves none behind)
    r.measure(u, time_major=True)
    refused(r, -1, ["samples have been fed"], t, 2, 4)
    r.reset_measurement()
    # the cap itself is accepted: K nrows P = ACME_MAX_SOURCE_TABLE
    r.set_measurement_target(big.reshape(64, 1, CAP // 64), which=[63, 0, 5], lag=[CAP // 64 - 1, 0, 1])
    r.measure(u, time_major=True)
    s, count = got_target(r)
    assert count == 9 and np.array_equal(s[:, 0, 0], (u[:, 1:, 0] ** 2).cumsum(axis=1)[:, -1]) and not s[:, 0, 1].any()
    r.reset_measurement()
    # a series and a target exclude each other, whichever is set first
    assert r.lib.L.acme_batch_set_measurement_series(r.h, 4, 4, 2) == -2 and "target" in r.lib.L.acme_last_error().decode()
    with pytest.raises(AcmeError, match="target"):
        r.set_measurement_series(4, 4, 2)
    r.set_measurement(start=1).set_measurement_series(4, 4, 2)
    refused(r, -2, ["series"], t, 2, 4)
    # the Python layer's own refusals
    from acme_jl_amd.runner import DimensionMismatch
    r.set_measurement(start=1)
    for bad in (np.zeros((2, 2, 4)), np.zeros((1, 1, 1, 4))):
        with pytest.raises(DimensionMismatch):
            r.set_measurement_target(bad)
    with pytest.raises(DimensionMismatch):
        r.set_measurement_target(t, which=[0, 0])
    with pytest.raises(DimensionMismatch):
        r.set_measurement_target(t, lag=[0, 0, 0, 0])
    with pytest.raises(DimensionMismatch):
        r.set_measurement_target(t, which=[0.5, 0, 0])


def check_no_target_invariance(mk, N, T):
    """a batch armed without a target, and one armed after a target has been set and removed: the results and the run kernel's
    launches of the existing forms"""
    from test_measurement import clipper_u
    m, u = clipper(), clipper_u(N, T)
    f_num = np.array([10, 20, 30])[np.arange(N) % 3]
    tgt = table(1, 1, 1, 441)
    arms = {"shared": lambda r: r.set_measurement(start=5, f0=(10, 441), harmonics=10),
            "per instance": lambda r: r.set_measurement(start=5, f_den=441, f_num=f_num, harmonics=10),
            "bins": lambda r: r.set_measurement_bins(np.array([[1], [2], [3]]), start=5, f_den=441, f_num=f_num[None])}
    for name, arm in arms.items():
        a = arm(mk(m, N))
        y = a.run(u, time_major=True)
        b = arm(mk(m, N)).set_measurement_target(tgt)
        arm(b)                                              # (arming removes the target)
        assert np.array_equal(b.run(u, time_major=True), y)
        c = arm(mk(m, N)).set_measurement_target(tgt).clear_measurement()
        arm(c)
        assert np.array_equal(c.run(u, time_major=True), y)
        d = arm(mk(m, N)).set_measurement_target(tgt)       # ... and with the target the run kernel's launches are the same
        assert np.array_equal(d.run(u, time_major=True), y)
        (oa, ca), (ob, cb), (oc, cc), (od, cd) = raw(a), raw(b), raw(c), raw(d)
        assert ca == cb == cc == cd == T - 5, name
        assert np.array_equal(oa, ob) and np.array_equal(oa, oc) and np.array_equal(oa, od), name
        assert a.kernel_time()[1] == b.kernel_time()[1] == c.kernel_time()[1] == d.kernel_time()[1] > 0, name
        for q in (b, c):
            assert q.lib.L.acme_batch_get_measurement_target(q.h, None, None) == -1


# ---- 10. a non-finite instance -------------------------------------------------------------------------------------------------
def check_nan_instance(mk, N=3, T=50):
    """the recipe of test_measurement: a NaN in one instance's input.  Its chains that see y read NaN, those of the target
    alone (Stt, St, Ptt) do not, and the other instances are unaffected"""
    from test_measurement import clipper_u
    m, u = clipper(), clipper_u(N, T)
    u[1, 20, 0] = np.nan
    tgt = table(2, 1, 1, 17)
    r = mk(m, N).set_measurement().set_measurement_target(tgt, lag=4, preemphasis=C_PATHS)
    y = r.run(u, time_major=True, check=False)
    assert r.report_arrays()["first_nonfinite"].tolist()[1] >= 0
    s = assert_target(got_target(r), y, tgt, None, 4, C_PATHS)
    assert np.isnan(s[1, 0, [0, 2, 4, 5]]).all() and np.isfinite(s[1, 0, [1, 3, 6]]).all() and np.isfinite(s[[0, 2]]).all()
