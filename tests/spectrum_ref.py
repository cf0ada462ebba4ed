"""Shared by the emulator and GPU tests of the measurement spectrum (acme_batch_set_measurement_spectrum, Welch-averaged
periodograms): the reference every spectrum is held to -- ``replay``, numpy on the stored y of an identical run without a
spectrum, following the header's contract literally in float64 (numpy has no fma) with the window and the table the kernel
itself uses (acme_batch_get_measurement_spectrum_table) -- and the checks, each taking ``mk(model, n)``, which makes a fresh
runner on the library under test (the emulator's or the GPU's).  The bins' sums (``measurement_spectrum(raw=True)``) and the
reported means are compared with ``==``."""
import ctypes as C
import functools

import numpy as np
import pytest

import exact_ref as X
import measure_pi_ref as PI
import multitone_ref as MT
import noise_ref as NR
import source_ref as sr
from fold_ref import got_fold, order_dependent_rows, same_fold, window
from helpers import FS, HS, load
from test_measurement import clipper, clipper_u, raw, two_output_clipper

U = X.U
MU_ABS = 1.5 * U            # the table's entries: |tw[k] - exact| (item 5; part of eta, not a measurement)
# (L, hop) with start = 301 and T = 9000 (count 8699): hop = L, L / 2, an odd hop; (4096, 4096): two segments, the second ends
# one chunk later; (4096, 1000): segments that start in one chunk and end two later
GEOMETRY = [(64, 64), (64, 32), (64, 37), (128, 96), (1024, 512), (4096, 2048), (4096, 4096), (4096, 1000)]


# ---- the reference ------------------------------------------------------------------------------------------------------------
def bit_reverse(L):
    bits = L.bit_length() - 1
    j = np.arange(L)
    r = np.zeros(L, dtype=np.int64)
    for k in range(bits):
        r |= ((j >> k) & 1) << (bits - 1 - k)
    return r


def transform(x, tw):
    """x [..., L] real -> (Xr, Xi) [..., L]: the radix-2 decimation-in-time transform of the contract, every operation a
    rounded float64 operation"""
    L = x.shape[-1]
    vr = np.ascontiguousarray(x[..., bit_reverse(L)])
    vi = np.zeros_like(vr)
    h = 1
    while h < L:
        i = np.arange(L)
        i = i[(i & h) == 0]
        k = (i & (h - 1)) * (L // (2 * h))
        wr, wi = tw[k, 0], tw[k, 1]
        ar, ai, br, bi = vr[..., i], vi[..., i], vr[..., i + h], vi[..., i + h]
        tr = wr * br - wi * bi
        ti = wr * bi + wi * br
        vr[..., i], vi[..., i], vr[..., i + h], vi[..., i + h] = ar + tr, ai + ti, ar - tr, ai - ti
        h *= 2
    return vr, vi


def segments_of(count, L, hop):
    return (count - L) // hop + 1 if count >= L else 0


def replay(yw, L, hop, w, tw, reverse=False, full=False):
    """yw [P, count], the window's samples per pair -> (acc [P, L / 2 + 1], segments): x = w y per segment, the transform,
    |X_k|^2 = Xr Xr + Xi Xi added per bin in segment order from 0.0 (``reverse``: last segment first -- the same terms in
    another order).  ``full``: also (Xr, Xi) [P, S, L / 2 + 1]"""
    S = segments_of(yw.shape[1], L, hop)
    acc = np.zeros((yw.shape[0], L // 2 + 1))
    Xr = Xi = np.zeros((yw.shape[0], 0, L // 2 + 1))
    if S:
        idx = hop * np.arange(S)[:, None] + np.arange(L)[None, :]
        Xr, Xi = transform(w * yw[:, idx], tw)
        Xr, Xi = Xr[..., :L // 2 + 1], Xi[..., :L // 2 + 1]
        pw = Xr * Xr + Xi * Xi
        for s in (reversed(range(S)) if reverse else range(S)):
            acc = acc + pw[:, s]
    return (acc, S, Xr, Xi) if full else (acc, S)


def got_spec(r):
    """(sums, mean [N, nrows, L / 2 + 1], segments, count) of the runner's spectrum"""
    a, b = r.measurement_spectrum(raw=True), r.measurement_spectrum()
    assert a.count == b.count and a.segments == b.segments and a.rows == b.rows and np.array_equal(a.window, b.window)
    return a.power, b.power, b.segments, b.count


def same_spec(a, b):
    return a[2:] == b[2:] and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[:2], b[:2]))


def assert_spec(r, got, yw):
    """``got`` (got_spec) against the replay on the window's samples yw [N, count, nrows], with the runner's own table"""
    sums, mean, S, count = got
    L, hop = r._spectrum
    w, tw = r.measurement_spectrum_table()
    N, cnt, nrows = yw.shape
    acc, want_S = replay(np.ascontiguousarray(yw.transpose(0, 2, 1)).reshape(N * nrows, cnt), L, hop, w, tw)
    acc = acc.reshape(N, nrows, L // 2 + 1)
    assert count == cnt and S == want_S, (count, cnt, S, want_S)
    assert sums.shape == mean.shape == acc.shape
    if S == 0:
        assert np.isnan(sums).all() and np.isnan(mean).all()
    else:
        assert np.array_equal(sums, acc), (L, hop, np.argwhere(sums != acc)[:6])
        assert np.array_equal(mean, acc / S), (L, hop)
    return sums


def windows(L):
    return {"rect": "rect", "hann": "hann", "random": np.random.default_rng(L).uniform(-1.0, 2.0, L)}


# ---- 1. segment geometry, windows, rows -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plain_run(mk, two, N, T, start, length, H, rows):
    """the run without a spectrum every geometry case of a shape shares: (model, u, y, raw measurement); never modified"""
    m = two_output_clipper() if two else clipper()
    u = clipper_u(N, T)
    r = mk(m, N).set_measurement(start=start, length=length, f0=(10, 441) if H else None, harmonics=H, rows=None if rows is None else list(rows))
    y = r.run(u, time_major=True)
    return m, u, y, raw(r)


def check_geometry(mk, N, T, start, H, L, hop, length=0, rows=None, two=False, win="hann"):
    m, u, y, plain = _plain_run(mk, two, N, T, start, length, H, None if rows is None else tuple(rows))
    r = mk(m, N).set_measurement(start=start, length=length, f0=(10, 441) if H else None, harmonics=H, rows=rows)
    r.set_measurement_spectrum(L, hop, windows(L)[win])
    assert np.array_equal(r.run(u, time_major=True), y)
    with_spec = raw(r)
    assert with_spec[1] == plain[1] and np.array_equal(with_spec[0], plain[0])        # the measurement's own results
    got = got_spec(r)
    assert_spec(r, got, window(y, start, length, rows))
    return got


def check_fold_and_spectrum(mk, N, T, start=301, H=10, L=128, hop=96, P=441):
    """a fold and a spectrum on one measurement: each == that of the run that carries it alone"""
    m, u, y, plain = _plain_run(mk, False, N, T, start, 0, H, None)
    arm = lambda: mk(m, N).set_measurement(start=start, f0=(10, 441), harmonics=H)
    both = arm().set_measurement_fold(P).set_measurement_spectrum(L, hop)
    other = arm().set_measurement_spectrum(L, hop).set_measurement_fold(P)      # (either way round)
    f, s = arm().set_measurement_fold(P), arm().set_measurement_spectrum(L, hop)
    for r in (both, other, f, s):
        r.measure(u, time_major=True)
        assert np.array_equal(raw(r)[0], plain[0])
    for r in (both, other):
        assert same_fold(got_fold(r), got_fold(f)) and same_spec(got_spec(r), got_spec(s))
    assert_spec(s, got_spec(s), window(y, start, 0))


def check_forms(mk, T, L, hop, start=3, H=10, wire=False):
    """shared, per instance (F = N = 130, mixed waves) and bins: the spectrum is the replay's, and the measurement's own
    results with the spectrum attached == those without it"""
    N, f_den = 130, 441
    m, u = (X.wire_model(1, FS), X.scaled_rows(np.random.default_rng(7), N, T, 1)) if wire else (clipper(), clipper_u(N, T))
    f_num = 1 + np.arange(N)
    tones = MT.tone_cases()["F=N"][0]
    arms = {"shared": lambda: mk(m, N).set_measurement(start=start, f0=(10, f_den), harmonics=H),
            "per instance": lambda: mk(m, N).set_measurement(start=start, f_den=f_den, f_num=f_num, harmonics=H),
            "bins": lambda: mk(m, N).set_measurement_bins(MT.COEF6, start=start, f_den=f_den, f_num=tones)}
    first = None
    for name, arm in arms.items():
        a = arm()
        y = a.run(u, time_major=True)
        plain = raw(a)
        b = arm().set_measurement_spectrum(L, hop)
        b.measure(u, time_major=True)
        with_spec = raw(b)
        assert with_spec[1] == plain[1] and np.array_equal(with_spec[0], plain[0]), name
        got = got_spec(b)
        assert_spec(b, got, window(y, start, 0))
        first = first or got
        assert same_spec(got, first), name


# ---- 2. paths -----------------------------------------------------------------------------------------------------------------
PATH_START = 1203


def check_paths(mk, dev, k, T, L, hop, monkeypatch, N=70, S=PATH_START, wire=False, tile_chunks=True):
    """one spectrum, H = 10, the model driven by what a per-instance sine source renders: the spectrum and the measurement read
    after every path == those after a host run with y stored.  ``dev``: the device-memory calls (put, run(r, u, keep, T)).
    ``wire``: the pass-through model in place of the diode clipper."""
    from fractions import Fraction
    from acme_jl_amd import examples
    from acme_jl_amd.model import DiscreteModel
    H = 10
    if wire:
        m = X.wire_model(1, k * FS)
    else:
        m = clipper() if k == 1 else DiscreteModel(examples.diodeclipper(), Fraction(1, k * FS), HS)
    src = dict(kind="sine", f_den=441, f_num=np.full(N, 10), amp=np.logspace(-2, 0.7, N))

    def fresh(sourced=False):
        r = mk(m, N).set_oversampling(k)
        if sourced:
            r = sr.apply_sources(r, [src]).set_measurement(start=S, harmonics=H, f0_from_source=0)
        else:
            r.set_measurement(start=S, f0=(10, 441), harmonics=H)
        return r.set_measurement_spectrum(L, hop)

    def read(r):
        return got_spec(r) + raw(r)
    u = sr.apply_sources(mk(m, N).set_oversampling(k), [src]).render_sources(T)
    r = fresh()
    y = r.run(u, time_major=True)
    ref = read(r)
    assert np.isfinite(y).all() and ref[2] >= 2
    assert_spec(r, ref[:4], window(y, S, 0))
    results = {"y NULL": read(fresh().measure(u, time_major=True))}
    # split calls: before the start, on a segment's first sample, inside a segment, on a chunk boundary
    cuts = sorted({c for c in (min(1000, S - 2), S + hop, S + hop + 40, S + L // 2 + 1, S + 4096) if 0 < c < T})
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
        assert same_spec(got[:4], ref[:4]), name
        assert got[5] == ref[5] and np.array_equal(got[4], ref[4]), name
    if k > 1:
        return
    # run_const on a constant row against run on the materialised input
    uc = np.logspace(-2, 0.7, N)[:, None]
    r = fresh()
    r.run(np.ascontiguousarray(np.broadcast_to(uc[:, None, :], (N, T, 1))), time_major=True)
    rc = fresh()
    rc.run_const(np.zeros((N, T, 0)), uc, [0])
    rn = fresh().measure_const(np.zeros((N, T, 0)), uc, [0])
    for q in (rc, rn):
        assert same_spec(got_spec(q), got_spec(r))
    if not tile_chunks:
        return
    # chunks of one tile (the per-instance form under a table budget of one byte), the calls cut again
    f_num = 1 + np.arange(N)
    monkeypatch.setenv("ACME_MEAS_TABLE_BUDGET", "1")
    b = mk(m, N).set_measurement(start=S, f_den=441, f_num=f_num, harmonics=H).set_measurement_spectrum(L, hop)
    assert b.measurement_plan()["chunk"] == 64
    b.measure(np.ascontiguousarray(u[:, :t1]), time_major=True)
    b.measure(np.ascontiguousarray(u[:, t1:]), time_major=True)
    monkeypatch.delenv("ACME_MEAS_TABLE_BUDGET")
    assert same_spec(got_spec(b), ref[:4])


def check_multi_device(mk, mk_md, L, hop, N=70, T=5200, wire=False):
    """``mk_md(model, n)``: a MultiDeviceRunner over two shards: its spectrum == the one runner's"""
    m = X.wire_model(1, FS) if wire else clipper()
    u = clipper_u(N, T)
    arm = lambda r: r.set_measurement(start=3, f0=(10, 441), harmonics=4).set_measurement_spectrum(L, hop)
    one = arm(mk(m, N))
    one.measure(u, time_major=True)
    md = arm(mk_md(m, N))
    md.measure(u)
    for sums in (False, True):
        a, b = one.measurement_spectrum(sums), md.measurement_spectrum(sums)
        assert a.count == b.count == T - 3 and a.segments == b.segments == segments_of(T - 3, L, hop) >= 2
        assert np.array_equal(a.power, b.power) and np.array_equal(a.window, b.window)


# ---- 3. life cycle and errors -------------------------------------------------------------------------------------------------
def check_life_cycle(mk, N=5, T=700, L=64, hop=48, start=9):
    from acme_jl_amd.runner import AcmeError
    m, u = clipper(), clipper_u(N, T)
    arm = lambda: mk(m, N).set_measurement(start=start, f0=(10, 441), harmonics=3)
    wrand = windows(L)["random"]
    # reset zeroes the sums and the carry, and keeps L, hop, the window and the table
    r = arm().set_measurement_spectrum(L, hop, wrand)
    table = r.measurement_spectrum_table()
    r.measure(np.ascontiguousarray(u[:, :start + hop + 30]), time_major=True)        # (stops inside segment 1)
    assert got_spec(r)[2:] == (1, hop + 30)
    r.reset_measurement()
    zero = r.measurement_spectrum()
    assert zero.count == 0 and zero.segments == 0 and np.isnan(zero.power).all() and np.array_equal(zero.window, wrand)
    assert all(np.array_equal(a, b) for a, b in zip(table, r.measurement_spectrum_table()))
    q = mk(m, N)
    q.run(np.ascontiguousarray(u[:, :start + hop + 30]), time_major=True)           # (the same state as r's at its reset)
    q.set_measurement(start=start, f0=(10, 441), harmonics=3).set_measurement_spectrum(L, hop, wrand)
    u2 = np.ascontiguousarray(u[:, :300])
    y2 = q.run(u2, time_major=True)
    cut = start + hop + 22              # inside segment 1: the chunk behind the cut reads segment 1's first samples from the ring
    for part in (u2[:, :cut], u2[:, cut:]):
        r.measure(np.ascontiguousarray(part), time_major=True)
    assert same_spec(got_spec(r), got_spec(q)) and got_spec(r)[3] == 300 - start
    assert_spec(q, got_spec(q), window(y2, start, 0))           # ... which the samples fed before the reset do not enter
    # a second pass after a reset == the first
    a = arm().set_measurement_spectrum(L, hop)
    b = mk(m, N)
    b.run(u2, time_major=True)
    b.set_measurement(start=start, f0=(10, 441), harmonics=3).set_measurement_spectrum(L, hop)
    a.measure(u2, time_major=True)
    a.reset_measurement()
    for part in (u2[:, :cut], u2[:, cut:]):
        a.measure(np.ascontiguousarray(part), time_major=True)
    b.measure(u2, time_major=True)
    assert same_spec(got_spec(a), got_spec(b))
    # a spectrum set again replaces the earlier one (after a reset: nothing has been fed)
    r.reset_measurement().set_measurement_spectrum(128, 128, "rect")
    assert r.measurement_spectrum().power.shape == (N, 1, 65) and (r.measurement_spectrum().window == 1.0).all()
    # re-arming and clear remove it
    r.set_measurement(start=start, f0=(10, 441), harmonics=3)
    with pytest.raises(AcmeError, match="no measurement spectrum"):
        r.measurement_spectrum()
    Lb = r.lib.L
    none = lambda: (Lb.acme_batch_get_measurement_spectrum(r.h, None, None, None) == -1 and "no measurement spectrum" in Lb.acme_last_error().decode()
                    and Lb.acme_batch_get_measurement_spectrum_table(r.h, None, None) == -1
                    and Lb.acme_batch_get_measurement_spectrum_sums(r.h, np.zeros(N * 65).ctypes.data_as(C.POINTER(C.c_double))) == -1)
    assert none()
    r.set_measurement_spectrum(L, hop).clear_measurement()
    assert none()
    with pytest.raises(AcmeError, match="no measurement is armed"):
        r.set_measurement_spectrum(L, hop)


def check_set_matrices_carries_the_spectrum(mk):
    from helpers import sweep_inputs
    from test_emu_parity import superover_models_with_their_own_diodes
    models = superover_models_with_their_own_diodes(3, HS)
    u = np.ascontiguousarray(sweep_inputs("superover_var", 3, 200, seed=2).transpose(0, 2, 1))
    r = mk(models[0], 3, models=[models[0]] * 3).set_measurement(start=10, f0=(1, 30), harmonics=3).set_measurement_spectrum(64, 20)
    ya = r.run(np.ascontiguousarray(u[:, :95]), time_major=True)
    r.set_models(1, [models[0]])
    r.set_models(2, [models[2]])                            # (the batch moves to the plain shape: a new batch takes the measurement over)
    yb = r.run(np.ascontiguousarray(u[:, 95:]), time_major=True)
    assert_spec(r, got_spec(r), window(np.concatenate([ya, yb], axis=1), 10, 0))


def check_errors(mk):
    """every refusal with its code and the argument's name in the message"""
    from acme_jl_amd.runner import AcmeError, DimensionMismatch
    m, u = clipper(), clipper_u(3, 10)
    dp = C.POINTER(C.c_double)

    def refused(r, code, what, L, hop, w=None):
        a = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        rc = r.lib.L.acme_batch_set_measurement_spectrum(r.h, L, hop, None if a is None else a.ctypes.data_as(dp))
        msg = r.lib.L.acme_last_error().decode()
        assert rc == code and all(x in msg for x in what), (L, hop, rc, msg)
    r = mk(m, 3)
    assert r.lib.L.acme_batch_set_measurement_spectrum(None, 64, 32, None) == -1
    refused(r, -1, ["no measurement is armed"], 64, 32)
    r.set_measurement(start=1)
    for bad in (0, -64, 32, 96, 100, 4095, 8192):
        refused(r, -1, ["L must be a power of two", "64", "4096"], bad, 1)
    for bad in (0, -1, 65):
        refused(r, -1, ["hop"], 64, bad)
    for bad in (np.nan, np.inf, -np.inf):
        w = np.ones(64)
        w[17] = bad
        refused(r, -1, ["w[17]", "not finite"], 64, 32, w)
    assert r.lib.L.acme_batch_get_measurement_spectrum(r.h, None, None, None) == -1      # (a refused spectrum leaves none behind)
    r.measure(u, time_major=True)
    refused(r, -1, ["samples have been fed"], 64, 32)
    r.reset_measurement().set_measurement_spectrum(4096, 4096)  # (the limits themselves are accepted)
    r.reset_measurement().set_measurement_spectrum(64, 1)
    assert r.lib.L.acme_batch_get_measurement_spectrum_sums(r.h, None) == -1 and "out" in r.lib.L.acme_last_error().decode()
    # a series and a spectrum exclude each other, whichever is set first
    assert r.lib.L.acme_batch_set_measurement_series(r.h, 4, 4, 2) == -2 and "spectrum" in r.lib.L.acme_last_error().decode()
    with pytest.raises(AcmeError, match="spectrum"):
        r.set_measurement_series(4, 4, 2)
    r.set_measurement(start=1).set_measurement_series(4, 4, 2)
    refused(r, -2, ["series"], 64, 32)
    # the Python layer's own refusals
    r.set_measurement(start=1)
    with pytest.raises(ValueError, match="window"):
        r.set_measurement_spectrum(64, window="hamming")
    with pytest.raises(DimensionMismatch):
        r.set_measurement_spectrum(64, window=np.ones(63))


def check_no_spectrum_invariance(mk, N, T):
    """a batch armed after a spectrum has been set and removed, and one with a spectrum: the results and the run kernel's
    launches of the existing forms"""
    m, u = clipper(), clipper_u(N, T)
    arm = lambda r: r.set_measurement(start=5, f0=(10, 441), harmonics=10)
    a = arm(mk(m, N))
    y = a.run(u, time_major=True)
    b = arm(arm(mk(m, N)).set_measurement_spectrum(64))
    c = arm(arm(mk(m, N)).set_measurement_spectrum(64).clear_measurement())
    d = arm(mk(m, N)).set_measurement_spectrum(64)
    for q in (b, c, d):
        assert np.array_equal(q.run(u, time_major=True), y)
        assert raw(q)[1] == raw(a)[1] and np.array_equal(raw(q)[0], raw(a)[0])
        assert q.kernel_time()[1] == a.kernel_time()[1] > 0
    for q in (b, c):
        assert q.lib.L.acme_batch_get_measurement_spectrum(q.h, None, None, None) == -1


# ---- 4. exact pins on the pass-through model ----------------------------------------------------------------------------------
def check_exact(mk, N, L, hop, T, lead=0, start=37):
    """the spectrum of data of the test's choosing through y = u, magnitudes spread over 2^40 from sample to sample: == the
    replay in segment order, which the replay in reverse order is not.  ``lead`` samples of zeros are fed first, in calls of
    at most 2^18, and the window starts ``start`` samples into the data"""
    u = order_dependent_rows(np.random.default_rng(L + hop + N), N, T)
    r = mk(X.wire_model(1, FS), N).set_measurement(start=lead + start).set_measurement_spectrum(L, hop)
    w, tw = r.measurement_spectrum_table()
    yw = np.ascontiguousarray(u[:, start:, 0])
    fwd, rev = replay(yw, L, hop, w, tw)[0], replay(yw, L, hop, w, tw, reverse=True)[0]
    assert (fwd != rev).any(), "the chosen data does not pin the order"
    z = np.zeros((N, min(lead, 2 ** 18), 1))
    for a in range(0, lead, 2 ** 18):
        r.measure(z[:, :min(2 ** 18, lead - a)], time_major=True)
    assert np.array_equal(r.run(u, time_major=True), u)
    sums = assert_spec(r, got_spec(r), u[:, start:])
    assert np.array_equal(sums[:, 0], fwd) and (sums[:, 0] != rev).any()


# ---- 5. the table -------------------------------------------------------------------------------------------------------------
def check_table(mk, sizes=(64, 128, 256, 512, 1024, 2048, 4096)):
    """exact at k = 0 and L / 4; every entry within MU_ABS of mpmath's (cos, -sin)(2 pi k / L).  Returns the worst error in
    units of 2^-53"""
    import mpmath
    r = mk(X.wire_model(1, FS), 1).set_measurement()
    worst = 0.0
    for L in sizes:
        r.reset_measurement().set_measurement_spectrum(L)
        w, tw = r.measurement_spectrum_table()
        assert tw.shape == (L // 2, 2) and tuple(tw[0]) == (1.0, 0.0) and tuple(tw[L // 4]) == (0.0, -1.0)
        assert np.array_equal(w, 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(L) / L))
        with mpmath.workprec(120):
            for k in range(L // 2):
                c, s = mpmath.cos_sin(2 * mpmath.pi * k / L)
                err = float(mpmath.sqrt((mpmath.mpf(float(tw[k, 0])) - c) ** 2 + (mpmath.mpf(float(tw[k, 1])) + s) ** 2))
                worst = max(worst, err / U)
                assert err <= MU_ABS, (L, k, err / U)
    return worst


# ---- 6. accuracy against exact arithmetic -------------------------------------------------------------------------------------
def eta():
    """Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2: the radix-2 transform with twiddles in error by
    mu_abs satisfies ||X^ - X||_2 <= sqrt(L) ||x||_2 q eta / (1 - q eta), q = log2 L, eta = mu + gamma_4 (sqrt 2 + mu) with
    gamma_4 = 4u / (1 - 4u); here mu enters twice (the table's error in both factors of the stated form)"""
    return 2 * MU_ABS + 4 * U * (np.sqrt(2.0) + 2 * MU_ABS) / (1 - 4 * U)


def ld_dft(x):
    """x [P, S, L] long double -> X [P, S, L / 2 + 1] (re, im) by the defining sum in long double, the roots of unity
    from long double cos / sin of the exact index (j k) mod L"""
    L = x.shape[-1]
    th = 2 * np.arccos(np.longdouble(-1)) * np.arange(L).astype(np.longdouble) / L
    c, s = np.cos(th), np.sin(th)
    j = np.arange(L)
    Xr, Xi = np.zeros(x.shape[:2] + (L // 2 + 1,), dtype=np.longdouble), np.zeros(x.shape[:2] + (L // 2 + 1,), dtype=np.longdouble)
    for k0 in range(0, L // 2 + 1, 128):
        k = np.arange(k0, min(k0 + 128, L // 2 + 1))
        jk = (j[:, None] * k[None, :]) % L
        Xr[..., k] = x @ c[jk]
        Xi[..., k] = -(x @ s[jk])
    return Xr, Xi


def check_accuracy(mk, L, hop=None, N=2, S=4, start=11):
    """random data through y = u, S segments: every transformed value of the replay (which the kernel's sums are pinned to,
    here too) within E_s of the long-double DFT of the exactly windowed segment, every accumulated bin of the KERNEL within
    the bound that follows.  Returns the worst ratios (transform, bins).

    E_s = sqrt(L) ||x_s||_2 (q eta / (1 - q eta) + u): the transform's error (Thm 24.2 bounds the 2-norm of the error vector,
    hence every component) plus the rounding of x_j = fl(w_j y_j), |dx_j| <= u |x_j|, which the exact transform carries to at
    most sqrt(L) ||dx||_2 <= sqrt(L) u ||x||_2 per component.  A bin: |X^|^2 evaluated as fl(fl(Xr Xr) + fl(Xi Xi)) is
    |X^|^2 (1 + d), |d| <= 2u + u^2, and | |X^|^2 - |X|^2 | <= 2 |X| E + E^2; the chain of S additions adds at most
    (S - 1) u of the running sum, itself at most sum (|X| + E)^2 (1 + ...): together below
    sum_s (2 |X_s| E_s + E_s^2) + (S + 3) u sum_s (|X_s| + E_s)^2.  The reference's own error (long double: 2^-64 per
    operation, L terms) is below 2^-10 of E_s at every L here and is not added."""
    hop = L // 2 if hop is None else hop
    T = start + L + (S - 1) * hop + 5
    q = L.bit_length() - 1
    u = X.scaled_rows(np.random.default_rng(L), N, T, 1)
    r = mk(X.wire_model(1, FS), N).set_measurement(start=start).set_measurement_spectrum(L, hop)
    w, tw = r.measurement_spectrum_table()
    assert np.array_equal(r.run(u, time_major=True), u)
    sums, _, segs, count = got_spec(r)
    yw = np.ascontiguousarray(u[:, start:, 0])
    acc, S_, Xr, Xi = replay(yw, L, hop, w, tw, full=True)
    assert segs == S_ == S and np.array_equal(sums[:, 0], acc)
    idx = hop * np.arange(S)[:, None] + np.arange(L)[None, :]
    x = w.astype(np.longdouble) * yw[:, idx].astype(np.longdouble)
    Er, Ei = ld_dft(x)
    qe = q * eta()
    E = np.sqrt(np.longdouble(L)) * np.sqrt((x * x).sum(axis=-1)) * (qe / (1 - qe) + U)      # [N, S]
    err = np.sqrt((Xr - Er) ** 2 + (Xi - Ei) ** 2)
    worst_x = float((err / E[..., None]).max())
    assert (err <= E[..., None]).all(), worst_x
    mag = np.sqrt(Er * Er + Ei * Ei)
    Eb = E[..., None]
    exact = (mag * mag).sum(axis=1)
    bound = (2 * mag * Eb + Eb * Eb).sum(axis=1) + (S + 3) * U * ((mag + Eb) ** 2).sum(axis=1)
    berr = np.abs(sums[:, 0].astype(np.longdouble) - exact)
    worst_b = float((berr / bound).max())
    assert (berr <= bound).all(), worst_b
    return worst_x, worst_b


# ---- 7. use level, deterministic ----------------------------------------------------------------------------------------------
def check_bode(mk):
    """sallenkey, one instance per frequency k / 64, one rectangular segment of 1024 samples behind BODE_START: amplitude() at
    bin 16 k against the armed measurement's |A_1| over the same 1024 samples.  Both estimate the same exact correlation
    X = sum_j y_j e^{-2 pi i k j / 64}, the spectrum as 2 sqrt(|X^|^2) / L, the measurement as (2 / n) |C - j S| with n = L.
    Spectrum side: |X^ - X| <= E (check_accuracy) and the power's three roundings, the square root's and none from the exact
    divisions by 1 and L / 2 -- at most 4u (|X| + E) --, so (2 / L)(E + 4u (|X| + E)), |X| <= sum |y|.  Measurement side: C and S
    each within exact_ref.harmonic_bound(n, sum |y|), so |A_1| within (2 / n) sqrt 2 of it.  Returns the worst |error| / bound."""
    m = load("sallenkey")
    L, f_num = 1024, np.arange(1, 32)
    S = PI.BODE_START["sallenkey"]
    r = mk(m, len(f_num))
    r.set_source(0, "sine", f_den=64, f_num=f_num)
    r.set_measurement(start=S, length=L, harmonics=1, f0_from_source=0).set_measurement_spectrum(L, L, "rect")
    y = r.run_sources(S + L + 50)
    sp, a1 = r.measurement_spectrum(), np.abs(r.measurement().harmonics[:, 0, 0])
    assert sp.segments == 1 and sp.count == L
    amp = sp.amplitude()
    yw = y[:, S:S + L, 0]
    l1, l2 = np.abs(yw).sum(axis=1), np.sqrt((yw * yw).sum(axis=1))
    qe = 10 * eta()
    E = np.sqrt(L) * l2 * (qe / (1 - qe) + U)
    worst = 0.0
    for i, k in enumerate(f_num):
        bound = (2.0 / L) * (E[i] + 4 * U * (l1[i] + E[i])) + (2.0 / L) * np.sqrt(2.0) * X.harmonic_bound(L, l1[i])
        worst = max(worst, abs(amp[i, 0, 16 * k] - a1[i]) / bound)
    return worst


# ---- 8. use level, noise --------------------------------------------------------------------------------------------------------
NOISE = dict(N=8, L=256, segments=400, amp=0.5, seed=1)


def noise_kind():
    c = NOISE
    return NR.noise(dist="gaussian", stream=[NR.seed_stream(c["seed"], i) for i in range(c["N"])], amp=np.full(c["N"], c["amp"]))


def noise_statistic(power, segments=None):
    """power [N, L / 2 + 1] means over the segments -> the bins' 0 < k < L / 2 deviations from amp^2 L in standard errors
    amp^2 L / sqrt(K), K = N x segments independent periodograms (each bin of white Gaussian noise is exponentially
    distributed: its standard deviation equals its mean)"""
    c = NOISE
    mean, K = c["amp"] ** 2 * c["L"], c["N"] * (segments or c["segments"])
    return (power[:, 1:c["L"] // 2].mean(axis=0) - mean) / (mean / np.sqrt(K))


def noise_reference_statistic(segments=None):
    """the same statistic from noise_ref's formulas and numpy's FFT alone (no library), over the first ``segments`` segments
    (None: all 400)"""
    c = NOISE
    S = segments or c["segments"]
    y = NR.gauss_row_float(noise_kind(), 0, c["N"], c["L"] * S, 0)
    pw = np.abs(np.fft.rfft(y.reshape(c["N"], S, c["L"]), axis=-1)) ** 2
    return noise_statistic(pw.mean(axis=1), S)


def check_noise(mk, segments=None):
    """a GAUSSIAN row through y = u: every bin's mean periodogram within 4.0 standard errors of amp^2 L, and the run through
    y = NULL == the run that stores y.  Returns the worst |deviation| in standard errors.  ``segments``: the first so many of
    the 400 (the emulator's time; the standard error is then that of N x segments periodograms)"""
    c = NOISE
    S = segments or c["segments"]
    T = c["L"] * S
    arm = lambda: NR.apply_sources(mk(X.wire_model(1, FS), c["N"]), [noise_kind()]).set_measurement().set_measurement_spectrum(c["L"], c["L"], "rect")
    r = arm()
    r.run_sources(T)
    q = arm().measure(T=T)
    assert same_spec(got_spec(r), got_spec(q))
    sp = r.measurement_spectrum()
    assert sp.segments == S and sp.count == T
    z = noise_statistic(sp.power[:, 0], S)
    assert len(z) == 127
    return float(np.abs(z).max())
