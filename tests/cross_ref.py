"""Shared by the emulator and GPU tests of the measurement cross-spectrum (acme_batch_set_measurement_cross): the reference
every cross-spectrum is held to -- ``replay``, numpy on the stored u and y of an identical run without a cross-spectrum,
following the header's contract literally in float64 (numpy has no fma) with the window and the table the kernel itself uses
(acme_batch_get_measurement_cross_table) -- and the checks, each taking ``mk(model, n)``, which makes a fresh runner on the
library under test (the emulator's or the GPU's).  The four planes' sums (``measurement_cross(raw=True)``) and the reported
means are compared with ``==``."""
import ctypes as C
import functools

import numpy as np
import pytest

import exact_ref as X
import measure_pi_ref as PI
import multitone_ref as MT
import noise_ref as NR
import source_ref as sr
import spectrum_ref as SR
from fold_ref import got_fold, order_dependent_rows, same_fold, window
from helpers import FS, HS, load
from spectrum_ref import bit_reverse, eta, got_spec, ld_dft, same_spec, segments_of, windows
from test_measurement import clipper, clipper_u, raw, two_output_clipper

U = X.U
# (L, hop) with start = 301 and T = 9000 (count 8699), as the issue lists them
GEOMETRY = [(64, 64), (64, 37), (128, 96), (1024, 512), (4096, 2048), (4096, 1000)]


# ---- the reference ------------------------------------------------------------------------------------------------------------
def transform(a, b, tw):
    """a, b [..., L] real -> (Zr, Zi) [..., L]: the contract's radix-2 decimation-in-time transform of the complex vector
    a + i b, every operation a rounded float64 operation (spectrum_ref.transform with the imaginary part loaded too)"""
    L = a.shape[-1]
    vr = np.ascontiguousarray(a[..., bit_reverse(L)])
    vi = np.ascontiguousarray(b[..., bit_reverse(L)])
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


def split(Zr, Zi):
    """Z [..., L] -> (Xr, Xi, Yr, Yi) [..., L / 2 + 1]: step 3 of the contract"""
    L = Zr.shape[-1]
    k = np.arange(L // 2 + 1)
    n = (L - k) % L
    return (0.5 * (Zr[..., k] + Zr[..., n]), 0.5 * (Zi[..., k] - Zi[..., n]),
            0.5 * (Zi[..., k] + Zi[..., n]), 0.5 * (Zr[..., n] - Zr[..., k]))


def replay(xw, yw, L, hop, w, tw, reverse=False, full=False):
    """xw, yw [P, count], the window's samples of x and y per pair -> (acc [P, 4, L / 2 + 1], segments): the planes xx, yy, re,
    im, each one chain per bin in segment order from 0.0 (``reverse``: last segment first -- the same terms in another
    order).  ``full``: also (Xr, Xi, Yr, Yi), each [P, S, L / 2 + 1]"""
    S = segments_of(yw.shape[1], L, hop)
    acc = np.zeros((yw.shape[0], 4, L // 2 + 1))
    parts = tuple(np.zeros((yw.shape[0], 0, L // 2 + 1)) for _ in range(4))
    if S:
        idx = hop * np.arange(S)[:, None] + np.arange(L)[None, :]
        parts = Xr, Xi, Yr, Yi = split(*transform(w * xw[:, idx], w * yw[:, idx], tw))
        terms = np.stack([Xr * Xr + Xi * Xi, Yr * Yr + Yi * Yi, Xr * Yr + Xi * Yi, Xr * Yi - Xi * Yr], axis=2)      # [P, S, 4, K]
        for s in (reversed(range(S)) if reverse else range(S)):
            acc = acc + terms[:, s]
    return (acc, S) + parts if full else (acc, S)


def planes(c):
    """a MeasurementCross -> [N, nrows, 4, L / 2 + 1]"""
    return np.stack([c.sxx, c.syy, c.sxy.real, c.sxy.imag], axis=2)


def got_cross(r):
    """(sums, mean [N, nrows, 4, L / 2 + 1], segments, count) of the runner's cross-spectrum"""
    a, b = r.measurement_cross(raw=True), r.measurement_cross()
    assert a.count == b.count and a.segments == b.segments and a.rows == b.rows and np.array_equal(a.window, b.window)
    assert a.in_row == b.in_row == r._cross[2] and a.hop == b.hop == r._cross[1] and a.nfft == r._cross[0]
    return planes(a), planes(b), b.segments, b.count


def same_cross(a, b):
    return a[2:] == b[2:] and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[:2], b[:2]))


def assert_cross(r, got, xw, yw):
    """``got`` (got_cross) against the replay on the window's samples xw [N, count] of the input row and yw [N, count, nrows]
    of the measured rows, with the runner's own table"""
    sums, mean, S, count = got
    L, hop, _ = r._cross
    w, tw = r.measurement_cross_table()
    N, cnt, nrows = yw.shape
    assert xw.shape == (N, cnt)
    xp = np.ascontiguousarray(np.broadcast_to(xw[:, None, :], (N, nrows, cnt))).reshape(N * nrows, cnt)
    acc, want_S = replay(xp, np.ascontiguousarray(yw.transpose(0, 2, 1)).reshape(N * nrows, cnt), L, hop, w, tw)
    acc = acc.reshape(N, nrows, 4, L // 2 + 1)
    assert count == cnt and S == want_S, (count, cnt, S, want_S)
    assert sums.shape == mean.shape == acc.shape
    if S == 0:
        assert np.isnan(sums).all() and np.isnan(mean).all()
    else:
        assert np.array_equal(sums, acc), (L, hop, np.argwhere(sums != acc)[:6])
        assert np.array_equal(mean, acc / S), (L, hop)
    return sums


# ---- 1. segment geometry, windows, rows, the input row ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plain_run(mk, two, N, T, start, length, H, rows):
    """the run without a cross-spectrum every geometry case of a shape shares: (model, u, y, raw measurement, run kernel
    launches); never modified"""
    m = two_output_clipper() if two else clipper()
    u = clipper_u(N, T)
    r = mk(m, N).set_measurement(start=start, length=length, f0=(10, 441) if H else None, harmonics=H, rows=None if rows is None else list(rows))
    y = r.run(u, time_major=True)
    return m, u, y, raw(r), r.kernel_time()[1]


def check_geometry(mk, N, T, start, H, L, hop, length=0, rows=None, two=False, win="hann"):
    m, u, y, plain, launches = _plain_run(mk, two, N, T, start, length, H, None if rows is None else tuple(rows))
    r = mk(m, N).set_measurement(start=start, length=length, f0=(10, 441) if H else None, harmonics=H, rows=rows)
    r.set_measurement_cross(0, L, hop, windows(L)[win])
    assert np.array_equal(r.run(u, time_major=True), y)                                 # the stored y
    with_cross = raw(r)
    assert with_cross[1] == plain[1] and np.array_equal(with_cross[0], plain[0])        # the measurement's own accumulators
    assert r.kernel_time()[1] == launches > 0                                           # the run kernel's launches
    got = got_cross(r)
    assert_cross(r, got, window(u, start, length)[:, :, 0], window(y, start, length, rows))
    return got


def check_in_row(mk, N, T, L, hop, start=11):
    """the pass-through model with two channels, row 0 constant through run_const: in_row = 1 (the varying row) and in_row = 0
    (the constant one) against both measured rows"""
    m = X.wire_model(2, FS)
    rng = np.random.default_rng(N + L)
    uv, uc = rng.standard_normal((N, T, 1)), rng.uniform(-2.0, 2.0, (N, 2))
    a = mk(m, N).set_measurement(start=start)
    y = a.run_const(uv, uc, [0])
    assert np.array_equal(y[:, :, 1:], uv) and np.array_equal(y[:, :, 0], np.broadcast_to(uc[:, :1], (N, T)))
    for in_row in (1, 0):
        r = mk(m, N).set_measurement(start=start).set_measurement_cross(in_row, L, hop)
        assert np.array_equal(r.run_const(uv, uc, [0]), y)
        assert raw(r)[1] == raw(a)[1] and np.array_equal(raw(r)[0], raw(a)[0]) and r.kernel_time()[1] == a.kernel_time()[1] > 0
        got = got_cross(r)
        assert got[2] >= 2
        assert_cross(r, got, y[:, start:, in_row], y[:, start:])
        q = mk(m, N).set_measurement(start=start).set_measurement_cross(in_row, L, hop).measure_const(uv, uc, [0])
        assert same_cross(got_cross(q), got)


def check_together(mk, N, T, start=301, H=10, L=128, hop=96, P=441):
    """a fold, a spectrum and a cross-spectrum on one measurement: each == that of the run that carries it alone"""
    m, u, y, plain, _ = _plain_run(mk, False, N, T, start, 0, H, None)
    arm = lambda: mk(m, N).set_measurement(start=start, f0=(10, 441), harmonics=H)
    all3 = arm().set_measurement_fold(P).set_measurement_spectrum(L, hop).set_measurement_cross(0, L, hop)
    other = arm().set_measurement_cross(0, 64, 37).set_measurement_spectrum(L, hop).set_measurement_fold(P)     # (another order, other segments)
    f, s = arm().set_measurement_fold(P), arm().set_measurement_spectrum(L, hop)
    c, c2 = arm().set_measurement_cross(0, L, hop), arm().set_measurement_cross(0, 64, 37)
    for r in (all3, other, f, s, c, c2):
        r.measure(u, time_major=True)
        assert np.array_equal(raw(r)[0], plain[0])
    for r, alone in ((all3, c), (other, c2)):
        assert same_fold(got_fold(r), got_fold(f)) and same_spec(got_spec(r), got_spec(s)) and same_cross(got_cross(r), got_cross(alone))
    assert_cross(c, got_cross(c), u[:, start:, 0], window(y, start, 0))


def check_forms(mk, T, L, hop, start=3, H=10, wire=False):
    """shared, per instance (F = N = 130, mixed waves) and bins: the cross-spectrum is the replay's, and the measurement's
    own results with it attached == those without it"""
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
        b = arm().set_measurement_cross(0, L, hop)
        b.measure(u, time_major=True)
        with_cross = raw(b)
        assert with_cross[1] == plain[1] and np.array_equal(with_cross[0], plain[0]), name
        got = got_cross(b)
        assert_cross(b, got, u[:, start:, 0], window(y, start, 0))
        first = first or got
        assert same_cross(got, first), name


# ---- 3. paths -----------------------------------------------------------------------------------------------------------------
PATH_START = SR.PATH_START


def check_paths(mk, dev, k, T, L, hop, monkeypatch, N=70, S=PATH_START, wire=False, tile_chunks=True):
    """spectrum_ref.check_paths' list for one cross-spectrum, H = 10, the model driven by what a per-instance sine source
    renders: the cross-spectrum and the measurement read after every path == those after a host run with y stored.  ``dev``:
    the device-memory calls (put, run(r, u, keep, T)).  ``wire``: the pass-through model in place of the diode clipper."""
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
        return r.set_measurement_cross(0, L, hop)

    def read(r):
        return got_cross(r) + raw(r)
    u = sr.apply_sources(mk(m, N).set_oversampling(k), [src]).render_sources(T)
    r = fresh()
    y = r.run(u, time_major=True)
    ref = read(r)
    assert np.isfinite(y).all() and ref[2] >= 2
    assert_cross(r, ref[:4], u[:, S:, 0], window(y, S, 0))      # (oversampled too: u before the interpolation, y after the decimation)
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
    r = fresh()
    assert np.array_equal(dev.run(r, ud, True, T), y)
    results["slices of 150, device"] = read(r)
    results["slices of 150, sources"] = read(fresh(sourced=True).measure(T=T))
    monkeypatch.delenv("ACME_OS_SLICE")
    for name, got in results.items():
        assert same_cross(got[:4], ref[:4]), name
        assert got[5] == ref[5] and np.array_equal(got[4], ref[4]), name
    if k > 1:
        return
    # run_const on a constant row (the input row itself) against run on the materialised input
    uc = np.logspace(-2, 0.7, N)[:, None]
    r = fresh()
    r.run(np.ascontiguousarray(np.broadcast_to(uc[:, None, :], (N, T, 1))), time_major=True)
    rc = fresh()
    rc.run_const(np.zeros((N, T, 0)), uc, [0])
    rn = fresh().measure_const(np.zeros((N, T, 0)), uc, [0])
    for q in (rc, rn):
        assert same_cross(got_cross(q), got_cross(r))
    if not tile_chunks:
        return
    # chunks of one tile (the per-instance form under a table budget of one byte), the calls cut again
    f_num = 1 + np.arange(N)
    monkeypatch.setenv("ACME_MEAS_TABLE_BUDGET", "1")
    b = mk(m, N).set_measurement(start=S, f_den=441, f_num=f_num, harmonics=H).set_measurement_cross(0, L, hop)
    assert b.measurement_plan()["chunk"] == 64
    b.measure(np.ascontiguousarray(u[:, :t1]), time_major=True)
    b.measure(np.ascontiguousarray(u[:, t1:]), time_major=True)
    monkeypatch.delenv("ACME_MEAS_TABLE_BUDGET")
    assert same_cross(got_cross(b), ref[:4])


def check_multi_device(mk, mk_md, L, hop, N=70, T=5200, wire=False):
    """``mk_md(model, n)``: a MultiDeviceRunner over two shards: its cross-spectrum == the one runner's"""
    m = X.wire_model(1, FS) if wire else clipper()
    u = clipper_u(N, T)
    arm = lambda r: r.set_measurement(start=3, f0=(10, 441), harmonics=4).set_measurement_cross(0, L, hop)
    one = arm(mk(m, N))
    one.measure(u, time_major=True)
    md = arm(mk_md(m, N))
    md.measure(u)
    for sums in (False, True):
        a, b = one.measurement_cross(sums), md.measurement_cross(sums)
        assert a.count == b.count == T - 3 and a.segments == b.segments == segments_of(T - 3, L, hop) >= 2
        assert np.array_equal(planes(a), planes(b)) and np.array_equal(a.window, b.window) and a.in_row == b.in_row == 0


# ---- 4. life cycle and errors -------------------------------------------------------------------------------------------------
def check_life_cycle(mk, N=5, T=700, L=64, hop=48, start=9):
    from acme_jl_amd.runner import AcmeError
    m, u = clipper(), clipper_u(N, T)
    arm = lambda: mk(m, N).set_measurement(start=start, f0=(10, 441), harmonics=3)
    wrand = windows(L)["random"]
    # reset zeroes the sums and the rings, and keeps L, hop, the window, the table and in_row
    r = arm().set_measurement_cross(0, L, hop, wrand)
    table = r.measurement_cross_table()
    r.measure(np.ascontiguousarray(u[:, :start + hop + 30]), time_major=True)        # (stops inside segment 1)
    assert got_cross(r)[2:] == (1, hop + 30)
    r.reset_measurement()
    zero = r.measurement_cross()
    assert zero.count == 0 and zero.segments == 0 and np.isnan(planes(zero)).all() and np.array_equal(zero.window, wrand) and zero.in_row == 0
    assert all(np.array_equal(a, b) for a, b in zip(table, r.measurement_cross_table()))
    q = mk(m, N)
    q.run(np.ascontiguousarray(u[:, :start + hop + 30]), time_major=True)           # (the same state as r's at its reset)
    q.set_measurement(start=start, f0=(10, 441), harmonics=3).set_measurement_cross(0, L, hop, wrand)
    u2 = np.ascontiguousarray(u[:, :300])
    y2 = q.run(u2, time_major=True)
    cut = start + hop + 22              # inside segment 1: the chunk behind the cut reads segment 1's first samples from the rings
    for part in (u2[:, :cut], u2[:, cut:]):
        r.measure(np.ascontiguousarray(part), time_major=True)
    assert same_cross(got_cross(r), got_cross(q)) and got_cross(r)[3] == 300 - start
    assert_cross(q, got_cross(q), u2[:, start:, 0], window(y2, start, 0))       # ... which the samples fed before the reset do not enter
    # a cross-spectrum set again replaces the earlier one (after a reset: nothing has been fed)
    r.reset_measurement().set_measurement_cross(0, 128, 128, "rect")
    assert planes(r.measurement_cross()).shape == (N, 1, 4, 65) and (r.measurement_cross().window == 1.0).all()
    # re-arming and clear remove it
    r.set_measurement(start=start, f0=(10, 441), harmonics=3)
    with pytest.raises(AcmeError, match="no measurement cross-spectrum"):
        r.measurement_cross()
    Lb = r.lib.L
    none = lambda: (Lb.acme_batch_get_measurement_cross(r.h, None, None, None) == -1 and "no measurement cross-spectrum" in Lb.acme_last_error().decode()
                    and Lb.acme_batch_get_measurement_cross_table(r.h, None, None) == -1
                    and Lb.acme_batch_get_measurement_cross_sums(r.h, np.zeros(N * 4 * 65).ctypes.data_as(C.POINTER(C.c_double))) == -1)
    assert none()
    r.set_measurement_cross(0, L, hop).clear_measurement()
    assert none()
    with pytest.raises(AcmeError, match="no measurement is armed"):
        r.set_measurement_cross(0, L, hop)


def check_set_matrices_carries_the_cross(mk):
    from helpers import sweep_inputs
    from test_emu_parity import superover_models_with_their_own_diodes
    models = superover_models_with_their_own_diodes(3, HS)
    u = np.ascontiguousarray(sweep_inputs("superover_var", 3, 200, seed=2).transpose(0, 2, 1))
    r = mk(models[0], 3, models=[models[0]] * 3).set_measurement(start=10, f0=(1, 30), harmonics=3).set_measurement_cross(0, 64, 20)
    ya = r.run(np.ascontiguousarray(u[:, :95]), time_major=True)
    r.set_models(1, [models[0]])
    r.set_models(2, [models[2]])                            # (the batch moves to the plain shape: a new batch takes the measurement over)
    yb = r.run(np.ascontiguousarray(u[:, 95:]), time_major=True)
    assert_cross(r, got_cross(r), u[:, 10:, 0], window(np.concatenate([ya, yb], axis=1), 10, 0))


def check_errors(mk):
    """every refusal with its code and the argument's name in the message"""
    from acme_jl_amd.model import DiscreteModel
    from acme_jl_amd.runner import AcmeError, DimensionMismatch
    m, u = clipper(), clipper_u(3, 10)
    dp = C.POINTER(C.c_double)

    def refused(r, code, what, in_row, L, hop, w=None):
        a = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        rc = r.lib.L.acme_batch_set_measurement_cross(r.h, in_row, L, hop, None if a is None else a.ctypes.data_as(dp))
        msg = r.lib.L.acme_last_error().decode()
        assert rc == code and all(x in msg for x in what), (in_row, L, hop, rc, msg)
    r = mk(m, 3)
    assert r.lib.L.acme_batch_set_measurement_cross(None, 0, 64, 32, None) == -1
    refused(r, -1, ["no measurement is armed"], 0, 64, 32)
    r.set_measurement(start=1)
    for bad in (-1, 1, 7):
        refused(r, -1, ["in_row"], bad, 64, 32)
    for bad in (0, -64, 32, 96, 100, 4095, 8192):
        refused(r, -1, ["L must be a power of two", "64", "4096"], 0, bad, 1)
    for bad in (0, -1, 65):
        refused(r, -1, ["hop"], 0, 64, bad)
    for bad in (np.nan, np.inf, -np.inf):
        w = np.ones(64)
        w[17] = bad
        refused(r, -1, ["w[17]", "not finite"], 0, 64, 32, w)
    assert r.lib.L.acme_batch_get_measurement_cross(r.h, None, None, None) == -1         # (a refused one leaves none behind)
    r.measure(u, time_major=True)
    refused(r, -1, ["samples have been fed"], 0, 64, 32)
    r.reset_measurement().set_measurement_cross(0, 4096, 4096)  # (the limits themselves are accepted)
    r.reset_measurement().set_measurement_cross(0, 64, 1)
    assert r.lib.L.acme_batch_get_measurement_cross_sums(r.h, None) == -1 and "out" in r.lib.L.acme_last_error().decode()
    # a series and a cross-spectrum exclude each other, whichever is set first
    assert r.lib.L.acme_batch_set_measurement_series(r.h, 4, 4, 2) == -2 and "cross-spectrum" in r.lib.L.acme_last_error().decode()
    with pytest.raises(AcmeError, match="cross-spectrum"):
        r.set_measurement_series(4, 4, 2)
    r.set_measurement(start=1).set_measurement_series(4, 4, 2)
    refused(r, -2, ["series"], 0, 64, 32)
    # a model without inputs
    from fractions import Fraction
    from acme_jl_amd.circuit import voltageprobe, voltagesource
    from acme_jl_amd.examples import build
    fixed = build([("src", voltagesource(1.0), {"-": "gnd"}), ("probe", voltageprobe(), {"+": ("src", "+"), "-": "gnd"})])
    z = mk(DiscreteModel(fixed, Fraction(1, FS), HS), 2).set_measurement()
    assert z.model.nu == 0
    refused(z, -1, ["nu"], 0, 64, 32)
    # the Python layer's own refusals
    r.set_measurement(start=1)
    with pytest.raises(ValueError, match="window"):
        r.set_measurement_cross(0, 64, window="hamming")
    with pytest.raises(DimensionMismatch):
        r.set_measurement_cross(0, 64, window=np.ones(63))


def check_no_cross_invariance(mk, N, T):
    """a batch armed after a cross-spectrum has been set and removed, and one with a cross-spectrum: the results and the run
    kernel's launches of the existing forms"""
    m, u = clipper(), clipper_u(N, T)
    arm = lambda r: r.set_measurement(start=5, f0=(10, 441), harmonics=10)
    a = arm(mk(m, N))
    y = a.run(u, time_major=True)
    b = arm(arm(mk(m, N)).set_measurement_cross(0, 64))
    c = arm(arm(mk(m, N)).set_measurement_cross(0, 64).clear_measurement())
    d = arm(mk(m, N)).set_measurement_cross(0, 64)
    for q in (b, c, d):
        assert np.array_equal(q.run(u, time_major=True), y)
        assert raw(q)[1] == raw(a)[1] and np.array_equal(raw(q)[0], raw(a)[0])
        assert q.kernel_time()[1] == a.kernel_time()[1] > 0
    for q in (b, c):
        assert q.lib.L.acme_batch_get_measurement_cross(q.h, None, None, None) == -1


# ---- 5. exact pins on the pass-through model ----------------------------------------------------------------------------------
def check_exact(mk, N, L, hop, T, lead=0, start=37):
    """two channels of data of the test's choosing through y = u, magnitudes spread over 2^40 from sample to sample, row 0 the
    input row and both rows measured: == the replay in segment order, which the replay in reverse order is not.  ``lead``
    samples of zeros are fed first, in calls of at most 2^18, and the window starts ``start`` samples into the data"""
    u = np.concatenate([order_dependent_rows(np.random.default_rng(L + hop + N), N, T),
                        order_dependent_rows(np.random.default_rng(L + hop + N + 1), N, T)], axis=2)
    r = mk(X.wire_model(2, FS), N).set_measurement(start=lead + start).set_measurement_cross(0, L, hop)
    w, tw = r.measurement_cross_table()
    xw = np.ascontiguousarray(u[:, start:, 0])
    fwd = np.stack([replay(xw, np.ascontiguousarray(u[:, start:, c]), L, hop, w, tw)[0] for c in (0, 1)], axis=1)
    rev = np.stack([replay(xw, np.ascontiguousarray(u[:, start:, c]), L, hop, w, tw, reverse=True)[0] for c in (0, 1)], axis=1)
    assert any((fwd[:, :, c] != rev[:, :, c]).any() for c in range(4)), "the chosen data does not pin the order"
    z = np.zeros((N, min(lead, 2 ** 18), 2))
    for a in range(0, lead, 2 ** 18):
        r.measure(z[:, :min(2 ** 18, lead - a)], time_major=True)
    assert np.array_equal(r.run(u, time_major=True), u)
    sums = assert_cross(r, got_cross(r), xw, u[:, start:])
    assert np.array_equal(sums, fwd) and any((sums[:, :, c] != rev[:, :, c]).any() for c in range(4))


# ---- 6. accuracy against exact arithmetic -------------------------------------------------------------------------------------
def sum_bounds(ax, ay, znorm, L):
    """The rounding bound of the four accumulated planes, from the exact bin magnitudes ax = |X_s,k|, ay = |Y_s,k| [P, S, K] and
    znorm = ||z_s||_2 [P, S], ||z_s||_2^2 = ||a||_2^2 + ||b||_2^2 with a = w x, b = w y exact: (Ex, Ey [P, S, K], Bxx, Byy, Bxy [P, K]).

    DESIGN 2.5j's derivation with the packed vector in place of the real one.  The transform: Higham Thm 24.2 bounds the
    2-norm of the error of the computed Z by sqrt(L) ||z||_2 q eta / (1 - q eta), hence every component's modulus; the
    roundings of a_j = fl(w_j x_j), b_j = fl(w_j y_j), |dz_j| <= u |z_j|, reach a component through the exact transform by at
    most sqrt(L) u ||z||_2: E_s = sqrt(L) ||z_s||_2 (q eta / (1 - q eta) + u).  The split: X = (Z_k + conj Z_n) / 2 exactly, so
    the error of Z carries over with at most (E_s + E_s) / 2 = E_s; the computed X has one rounded addition per component
    (the halving is exact), a relative u per component, at most sqrt 2 u |X^| <= sqrt 2 u (|X| + E_s) in modulus:
    Ex = E_s + sqrt 2 u (|X| + E_s), Ey likewise.  A product bin of one segment: conj(X^) Y^ - conj(X) Y is at most
    |X| Ey + |Y| Ex + Ex Ey in modulus, hence in either part; each part is evaluated as fl(fl(p) +- fl(q)) with
    |p| + |q| <= |X^| |Y^|, a relative 2u + u^2: together |X| Ey + |Y| Ex + Ex Ey + (2u + u^2)(|X| + Ex)(|Y| + Ey), and the same
    with Y = X for xx and X = Y for yy.  The chain of S additions adds at most (S - 1) u of the summed magnitudes, each computed
    term being at most (1 + 2u + u^2)(|X| + Ex)(|Y| + Ey) and a running sum at most (1 + u)^(S - 1) of their sum."""
    q = L.bit_length() - 1
    qe = q * eta()
    S = ax.shape[1]
    E = (np.sqrt(np.longdouble(L)) * znorm * (qe / (1 - qe) + U))[..., None]
    Ex = E + np.sqrt(2.0) * U * (ax + E)
    Ey = E + np.sqrt(2.0) * U * (ay + E)
    r2 = 2 * U + U * U

    def plane(a, ea, b, eb):
        mags = ((a + ea) * (b + eb)).sum(axis=1)
        return (a * eb + b * ea + ea * eb + r2 * (a + ea) * (b + eb)).sum(axis=1) + (S - 1) * U * (1 + r2) * (1 + U) ** (S - 1) * mags
    return Ex, Ey, plane(ax, Ex, ax, Ex), plane(ay, Ey, ay, Ey), plane(ax, Ex, ay, Ey)


def check_accuracy(mk, L, scale, hop=None, N=2, S=4, start=11):
    """random data through the two-channel pass-through model, y scaled by ``scale``, S segments: X and Y of the replay (which
    the kernel's sums are pinned to, here too) within Ex, Ey of the long-double DFT of the exactly windowed segments, every
    accumulated bin of the KERNEL within sum_bounds'.  Returns the worst ratios (X, Y, planes).  The reference's own error
    (long double: 2^-64 per operation, L terms) is below 2^-10 of E_s at every L here and is not added."""
    hop = L // 2 if hop is None else hop
    T = start + L + (S - 1) * hop + 5
    u = np.random.default_rng(L).standard_normal((N, T, 2))
    u[:, :, 1] *= scale
    r = mk(X.wire_model(2, FS), N).set_measurement(start=start, rows=[1]).set_measurement_cross(0, L, hop)
    w, tw = r.measurement_cross_table()
    assert np.array_equal(r.run(u, time_major=True), u)
    sums, _, segs, count = got_cross(r)
    xw, yw = np.ascontiguousarray(u[:, start:, 0]), np.ascontiguousarray(u[:, start:, 1])
    acc, S_, Xr, Xi, Yr, Yi = replay(xw, yw, L, hop, w, tw, full=True)
    assert segs == S_ == S and np.array_equal(sums[:, 0], acc)
    idx = hop * np.arange(S)[:, None] + np.arange(L)[None, :]
    wl = w.astype(np.longdouble)
    a, b = wl * xw[:, idx].astype(np.longdouble), wl * yw[:, idx].astype(np.longdouble)
    Er, Ei = ld_dft(np.concatenate([a, b]))
    (EXr, EYr), (EXi, EYi) = (Er[:N], Er[N:]), (Ei[:N], Ei[N:])
    ax, ay = np.sqrt(EXr * EXr + EXi * EXi), np.sqrt(EYr * EYr + EYi * EYi)
    Ex, Ey, Bxx, Byy, Bxy = sum_bounds(ax, ay, np.sqrt((a * a).sum(axis=-1) + (b * b).sum(axis=-1)), L)
    ex = np.sqrt((Xr - EXr) ** 2 + (Xi - EXi) ** 2)
    ey = np.sqrt((Yr - EYr) ** 2 + (Yi - EYi) ** 2)
    worst_x, worst_y = float((ex / Ex).max()), float((ey / Ey).max())
    assert (ex <= Ex).all() and (ey <= Ey).all(), (worst_x, worst_y)
    exact = [(ax * ax).sum(axis=1), (ay * ay).sum(axis=1), (EXr * EYr + EXi * EYi).sum(axis=1), (EXr * EYi - EXi * EYr).sum(axis=1)]
    worst_b = 0.0
    for c, bound in enumerate((Bxx, Byy, Bxy, Bxy)):
        berr = np.abs(sums[:, 0, c].astype(np.longdouble) - exact[c])
        worst_b = max(worst_b, float((berr / bound).max()))
        assert (berr <= bound).all(), (c, worst_b)
    return worst_x, worst_y, worst_b


def ratio_bounds(sxx, syy, sxy, Bxx, Byy, Bxy):
    """(bound on |H1 - H|, bound on |gamma^2 - gamma0^2|) for H1 = sxy / sxx and gamma^2 = |sxy|^2 / (sxx syy) evaluated in
    float64 from sums within Bxx, Byy of sxx, syy and Bxy of either part of sxy (the arguments: the exact or reference sums).
    H1: |d sxy| <= sqrt 2 Bxy and |d sxx| <= Bxx give (sqrt 2 Bxy + |H| Bxx) / (sxx - Bxx); numpy's complex division by a real
    adds at most 2u |H1|.  gamma^2: the relative errors 2 sqrt 2 Bxy / |sxy|, Bxx / sxx, Byy / syy of the three factors to first
    order, times (1 + their sum) for the rest, and 6u for the evaluation's six operations."""
    H, mag = np.abs(sxy) / sxx, np.abs(sxy)
    bh = (np.sqrt(2.0) * Bxy + H * Bxx) / (sxx - Bxx) + 4 * U * H
    rel = 2 * np.sqrt(2.0) * Bxy / mag + Bxx / (sxx - Bxx) + Byy / (syy - Byy)
    g = mag * mag / (sxx * syy)
    return bh, g * (rel * (1 + rel) + 6 * U)


def numpy_sums(xw, yw, L, S):
    """xw [N, S L], yw [N, S L] -> (sxx, syy, sxy, |X|, |Y| [N, S, K]): numpy's FFT on disjoint rectangular segments"""
    Xf = np.fft.rfft(xw.reshape(xw.shape[0], S, L), axis=-1)
    Yf = np.fft.rfft(yw.reshape(yw.shape[0], S, L), axis=-1)
    return (np.abs(Xf) ** 2).sum(axis=1), (np.abs(Yf) ** 2).sum(axis=1), (np.conj(Xf) * Yf).sum(axis=1), np.abs(Xf), np.abs(Yf)


def rect_bounds(xw, yw, L, S):
    """sum_bounds for disjoint rectangular segments of the stored xw, yw [N, S L], the magnitudes from numpy's FFT (their
    own relative error, some 1e-15, enters a BOUND and is immaterial).  The result is doubled: the numpy estimate the kernel
    is compared with is itself a float64 FFT, product and sum of the same length, held to the same bound."""
    sxx, syy, sxy, ax, ay = numpy_sums(xw, yw, L, S)
    zn = np.sqrt((xw * xw).reshape(xw.shape[0], S, L).sum(axis=-1) + (yw * yw).reshape(yw.shape[0], S, L).sum(axis=-1))
    _, _, Bxx, Byy, Bxy = sum_bounds(ax, ay, zn, L)
    return sxx, syy, sxy, 2 * Bxx, 2 * Byy, 2 * Bxy


# ---- 7. use level, deterministic ----------------------------------------------------------------------------------------------
SYSID_H_REF = 1.69e-12      # the reference alone (numpy's FFT on the emulator's stored u and y): worst |H1 - H_sine| / |H_sine|


def sine_gains(mk):
    """sallenkey, one instance per frequency k / 64, k = 1 ... 31, as spectrum_ref.check_bode runs them: the complex gain over
    the 1024 samples behind BODE_START -- the armed measurement's harmonics[:, 0, 0] over (2 / L) rfft(u)[16 k] of the
    rendered sine"""
    m = load("sallenkey")
    L, f_num = 1024, np.arange(1, 32)
    S = PI.BODE_START["sallenkey"]
    r = mk(m, len(f_num))
    r.set_source(0, "sine", f_den=64, f_num=f_num)
    u = r.render_sources(S + L)
    r.set_measurement(start=S, length=L, harmonics=1, f0_from_source=0)
    r.measure(T=S + L + 50)
    a_in = (2.0 / L) * np.fft.rfft(u[:, S:S + L, 0], axis=-1)[np.arange(31), 16 * f_num]
    return r.measurement().harmonics[:, 0, 0] / a_in


def check_sysid(mk):
    """sallenkey driven by a looped table of 1024 uniform values at three levels, 4 rectangular segments of 1024 behind
    BODE_START: no leakage (the excitation is periodic in L).  transfer() at bins 16 k against (a) the numpy estimate from the
    stored u and y, within the rounding bound of item 6, and (b), the numpy estimate, against the gain per-instance sine
    sources measure, within 4 x SYSID_H_REF.  Returns the worst (kernel against numpy / bound, numpy against sine, relative,
    |1 - coherence| over bins 1 ... 511)"""
    m = load("sallenkey")
    L, S, K = 1024, PI.BODE_START["sallenkey"], 4
    T = S + K * L
    arm = lambda: mk(m, 3).set_source(0, "table", table=np.random.default_rng(5).uniform(-1, 1, 1024), amp=np.array([0.1, 0.5, 1.0]))
    u = arm().render_sources(T)
    r = arm().set_measurement(start=S).set_measurement_cross(0, L, L, "rect")
    y = r.run_sources(T)
    c = r.measurement_cross()
    assert c.segments == K and c.count == K * L and c.in_row == 0 and c.rows == (0,)
    xw, yw = np.ascontiguousarray(u[:, S:, 0]), np.ascontiguousarray(y[:, S:, 0])
    sxx, syy, sxy, Bxx, Byy, Bxy = rect_bounds(xw, yw, L, K)
    H_np, H1 = sxy / sxx, c.transfer()[:, 0]
    bins = 16 * np.arange(1, 32)
    bh, _ = ratio_bounds(*(a[:, bins] for a in (sxx, syy, sxy, Bxx, Byy, Bxy)))
    worst_k = float((np.abs(H1 - H_np)[:, bins] / bh).max())
    assert worst_k <= 1.0, worst_k
    Hs = sine_gains(mk)
    worst_s = float((np.abs(H_np[:, bins] - Hs[None]) / np.abs(Hs[None])).max())
    with np.errstate(invalid="ignore"):      # (the filter's response is exactly 0 at Nyquist: 0 / 0 there)
        worst_g = float(np.abs(1.0 - c.coherence()[:, 0, 1:512]).max())
    print(f"sallenkey: kernel H1 against numpy's {worst_k:.3e} of its bound; numpy's against the sine gains {worst_s:.3e} "
          f"(|H| {np.abs(Hs).min():.2e} ... {np.abs(Hs).max():.2e}); worst |1 - coherence| {worst_g:.3e}")
    assert worst_s <= 4 * SYSID_H_REF, worst_s
    return worst_k, worst_s, worst_g


# ---- 8. use level, noise --------------------------------------------------------------------------------------------------------
NOISE = SR.NOISE


def coherence_limit(K, values=1016, p=1e-3):
    """c with values x P(gamma^2 > c) = p: gamma^2 of K disjoint segments of independent Gaussian signals is Beta(1, K - 1),
    P(gamma^2 > c) = (1 - c)^(K - 1)"""
    return 1.0 - (p / values) ** (1.0 / (K - 1))


def coherence_statistic(g, K):
    """g [N, 127] -> (worst value, the pooled mean's deviation from 1 / K in standard errors; one value's sd is
    sqrt((K - 1) / (K^2 (K + 1))))"""
    se = np.sqrt((K - 1) / (K * K * (K + 1.0))) / np.sqrt(g.size)
    return float(g.max()), float((g.mean() - 1.0 / K) / se)


def noise_reference_statistic(segments=None):
    """the statistic of two independent GAUSSIAN rows from noise_ref's formulas and numpy's FFT alone (no library)"""
    c = NOISE
    K = segments or c["segments"]
    x, y = (NR.gauss_row_float(SR.noise_kind(), row, c["N"], c["L"] * K, 0) for row in (0, 1))
    sxx, syy, sxy, _, _ = numpy_sums(x, y, c["L"], K)
    g = (np.abs(sxy) ** 2 / (sxx * syy))[:, 1:c["L"] // 2]
    assert g.shape == (8, 127)
    return coherence_statistic(g, K)


def check_noise(mk, segments=None):
    """two GAUSSIAN rows through the two-channel pass-through model, in_row = 0, both rows measured, disjoint rectangular
    segments.  Row 0 (y = x): |H1| = 1 and coherence 1 within item 6's bound; row 1 (independent): every coherence value below
    coherence_limit and the pooled mean within 4 standard errors of 1 / K; the run with y = NULL == the run that stores y.
    Returns (worst row-0 error / bound, worst coherence, pooled deviation in standard errors)."""
    c = NOISE
    K = segments or c["segments"]
    L, N, T = c["L"], c["N"], c["L"] * K
    arm = lambda: NR.apply_sources(mk(X.wire_model(2, FS), N), [SR.noise_kind(), SR.noise_kind()]).set_measurement().set_measurement_cross(0, L, L, "rect")
    r = arm()
    y = r.run_sources(T)
    q = arm().measure(T=T)
    assert same_cross(got_cross(r), got_cross(q))
    cr = r.measurement_cross()
    assert cr.segments == K and cr.count == T and cr.rows == (0, 1)
    x = np.ascontiguousarray(y[:, :, 0])
    sxx, syy, sxy, Bxx, Byy, Bxy = rect_bounds(x, x, L, K)
    bh, bg = ratio_bounds(sxx, syy, sxy, Bxx, Byy, Bxy)
    # (x = y: the exact H is 1 and the exact coherence 1; the numpy sums only size the bound)
    worst0 = max(float((np.abs(cr.transfer()[:, 0] - 1.0) / (bh / 2)).max()), float((np.abs(cr.coherence()[:, 0] - 1.0) / (bg / 2)).max()))
    assert worst0 <= 1.0, worst0
    g = cr.coherence()[:, 1, 1:L // 2]
    assert g.shape == (8, 127)
    worst, dev = coherence_statistic(g, K)
    assert worst < coherence_limit(K), (worst, coherence_limit(K))
    assert abs(dev) <= 4.0, dev
    return worst0, worst, dev
