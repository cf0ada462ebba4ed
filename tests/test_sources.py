"""Sources (acme_batch_set_source_*, csrc/acme_source.h) on the CPU wave emulator: rendered values against exact arithmetic
(CONST / TABLE bit for bit, SINE against mpmath at the phase reduced in unbounded integers), the defining property -- a source
run is acme_batch_run on the rendered u, bit for bit -- across memory kinds, stored and measured runs, oversampling, split and
asynchronous calls, the measurement end to end, argument errors and the interplay with the other entry points."""
import ctypes as C

import numpy as np
import pytest

import source_ref as sr
from exact_ref import U, harmonic_bound, ld_harmonics, unscale
from helpers import FS, HS, load

SLICE = 24          # ACME_OS_SLICE of these tests: every run of more samples crosses slices


def runner(model, n, lib, **kw):
    from acme_jl_amd.runner import ModelRunner
    return ModelRunner(model, n, lib=lib, **kw)


@pytest.fixture(autouse=True)
def small_slices(monkeypatch):
    monkeypatch.setenv("ACME_OS_SLICE", str(SLICE))


def awkward_kinds(N, rng, P):
    """a sine of prime f_den near 2^31 with f_num near f_den, a CONST row, a table of P entries, all with per-instance
    parameters"""
    return [dict(kind="sine", f_den=sr.PRIME_DEN, f_num=sr.PRIME_DEN - 1 - 3 * np.arange(N), phase=(np.arange(N) * 715827881) % sr.PRIME_DEN,
                 amp=rng.standard_normal(N) * 10.0 ** rng.integers(-3, 4, N), offset=rng.standard_normal(N)),
            dict(kind="const", offset=rng.standard_normal(N)),
            dict(kind="table", table=rng.standard_normal(P), amp=rng.standard_normal(N), offset=rng.standard_normal(N))]


# ---- 1. rendered values against exact arithmetic -----------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 7, 61])             # one entry, a prime, more than a slice
@pytest.mark.parametrize("clock", sr.CLOCKS)
def test_rendered_values_are_the_exact_ones(emu_lib, clock, P):
    N, T = 5, 2 * SLICE + 11                           # (the last slice ends mid-period of every row)
    rng = np.random.default_rng(P)
    kinds = awkward_kinds(N, rng, P)
    r = sr.apply_sources(runner(sr.wire_model(3, FS), N, emu_lib), kinds)
    r.source_clock = clock
    u = r.render_sources(T)
    want = sr.expected_rows(kinds, N, T, clock)
    assert np.array_equal(u[:, :, 1:], want[:, :, 1:])
    worst = sr.check_sine_row(u[:, :, 0], kinds[0], N, clock, [(i, t) for i in range(N) for t in range(T)])
    print(f"clock {clock}: worst sine error {worst:.3f} of its bound")
    # the same through a source run of the pass-through model: y = u
    y = r.run_sources(T)
    assert np.array_equal(y, u) and r.source_clock == clock + T


@pytest.mark.parametrize("nu,lds", [(1, "1"), (1, "0"), (2, "1"), (3, "0"), (5, "1"), (6, "1")])
def test_every_store_shape_and_both_table_paths(emu_lib, monkeypatch, nu, lds):
    """one and two elements per thread (odd and even row counts, a single row with an even and an odd number of samples),
    tables from LDS and from memory, defaults for every per-instance parameter, a caller's row among the sourced ones"""
    monkeypatch.setenv("ACME_SOURCE_LDS", lds)
    N = 6
    rng = np.random.default_rng(nu)
    tabs = [rng.standard_normal(P) for P in (1, 13, 4099, 29, 5, 2)]
    kinds = [dict(kind="table", table=tabs[c], amp=None if c % 2 else rng.standard_normal(N), offset=None if c % 3 else rng.standard_normal(N))
             for c in range(nu)]
    if nu >= 3:
        kinds[1] = None                                # (the caller's row)
        kinds[2] = dict(kind="sine", f_den=48, f_num=None, phase=np.arange(N) * 7)
    for T in (SLICE + 5, 2 * SLICE):
        r = sr.apply_sources(runner(sr.wire_model(nu, FS), N, emu_lib), kinds)
        r.source_clock = 4095
        uv = rng.standard_normal((N, T, 1)) if nu >= 3 else None
        u = r.render_sources(T, uv)
        want = sr.expected_rows(kinds, N, T, 4095)
        for c, k in enumerate(kinds):
            if k is None:
                assert np.array_equal(u[:, :, c], uv[:, :, 0])
            elif k["kind"] == "table":
                assert np.array_equal(u[:, :, c], want[:, :, c]), (c, T)
            else:
                sr.check_sine_row(u[:, :, c], k, N, 4095, [(i, t) for i in range(N) for t in range(T)])
        if uv is not None:                             # u_var = NULL renders zeros in the caller's rows
            assert np.array_equal(r.render_sources(T)[:, :, 1], np.zeros((N, T)))


def test_a_long_render_crosses_tiles_and_matches_short_ones(emu_lib, monkeypatch):
    """one launch of more than a tile of samples (ACME_OS_SLICE above 4096) against renders slice by slice: the same values,
    the table beyond what LDS holds included"""
    N, T = 3, 4096 + 300
    rng = np.random.default_rng(5)
    kinds = [dict(kind="sine", f_den=44100, f_num=1000 + np.arange(N), amp=rng.standard_normal(N)),
             dict(kind="table", table=rng.standard_normal(5000))]
    r = sr.apply_sources(runner(sr.wire_model(2, FS), N, emu_lib), kinds)
    r.source_clock = 2 ** 40
    short = r.render_sources(T)
    monkeypatch.setenv("ACME_OS_SLICE", "8192")
    assert np.array_equal(r.render_sources(T), short)
    assert np.array_equal(short[:, :, 1], sr.expected_rows(kinds, N, T, 2 ** 40)[:, :, 1])


# ---- 2. the defining property ---------------------------------------------------------------------------------------------------
def property_cases():
    """(name, model, N, kinds, u_var or None): the pass-through model, the diode clipper, superover with a sine on the signal
    row and CONST pots, a model with a caller's row next to sourced rows"""
    rng = np.random.default_rng(11)
    N = 3
    sine = dict(kind="sine", f_den=FS, f_num=1000 + 500 * np.arange(N), phase=np.arange(N) * 100, amp=np.logspace(-1, 0.5, N))
    pots = [dict(kind="const", offset=v) for v in ((np.arange(N) + 0.5) / N, np.full(N, 0.4), np.full(N, 0.7))]
    return [("wire", sr.wire_model(2, FS), N, [dict(sine, offset=rng.standard_normal(N)), dict(kind="table", table=rng.standard_normal(37))], None),
            ("diodeclipper", load("diodeclipper", HS), N, [sine], None),
            ("superover_var", load("superover_var", HS), N, [sine] + pots, None),
            ("birdie_var: caller's signal row, CONST pot", load("birdie_var", HS), N, [None, dict(kind="const", offset=(np.arange(N) + 1.0) / (N + 1))],
             0.3 * rng.standard_normal((N, 200, 1)))]


T_PROP = 2 * SLICE + 9
MODES = [dict(mem=0, keep=True), dict(mem=1, keep=True), dict(mem=0, keep=False), dict(mem=1, keep=False),
         dict(mem=0, keep=True, split=SLICE + 7), dict(mem=1, keep=True, split=SLICE + 7), dict(mem=0, keep=False, split=5),
         dict(mem=0, keep=True, use_async=True), dict(mem=1, keep=False, use_async=True),
         dict(mem=1, keep=True, measure=dict(f0=(1000, FS), harmonics=2))]


@pytest.mark.parametrize("mode", range(len(MODES)))
@pytest.mark.parametrize("case", range(4))
def test_a_source_run_is_a_run_on_the_rendered_input(emu_lib, case, mode):
    name, m, N, kinds, u_var = property_cases()[case]
    u = sr.check_defining_property(emu_lib, m, N, kinds, u_var, T_PROP, more=SLICE + 3, clock=2 ** 31 - 20, **MODES[mode])
    assert np.abs(u).max() > 1e-3 and np.isfinite(u).all()


@pytest.mark.parametrize("held", [False, True])
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("case", range(4))
def test_oversampled_source_runs(emu_lib, case, k, held):
    """the sourced row generated at the base rate, then interpolated or held as a caller's row is; CONST rows held"""
    name, m, N, kinds, u_var = property_cases()[case]
    rows = [r for r, kd in enumerate(kinds) if kd is not None and kd["kind"] != "const"][:1] if held else []
    for mode in (dict(mem=0, keep=True, split=SLICE + 7), dict(mem=1, keep=False)):
        sr.check_defining_property(emu_lib, m, N, kinds, u_var, T_PROP, k=k, held=rows, more=SLICE + 3, **mode)


def test_const_rows_are_held_on_an_oversampled_batch(emu_lib):
    """a CONST row goes through no filter: the twin that holds the row explicitly agrees, the one that interpolates it
    does not have to"""
    m, N, T = sr.wire_model(2, FS), 2, 40
    kinds = [dict(kind="sine", f_den=64, f_num=5), dict(kind="const", offset=np.array([0.25, -3.0]))]
    a = sr.apply_sources(runner(m, N, emu_lib), kinds).set_oversampling(4)
    u = a.render_sources(T)
    y = a.run_sources(T)
    b = runner(m, N, emu_lib).set_oversampling(4, held_rows=(1,))
    assert np.array_equal(y, b.run(u, time_major=True))


def test_balance_on_and_off(emu_lib, monkeypatch):
    monkeypatch.setenv("ACME_EMU_CUS", "1")
    name, m, N, kinds, _ = property_cases()[2]
    N = 40
    kinds = [dict(kind="sine", f_den=FS, f_num=1000, amp=np.logspace(-2, 0.5, N))] + [dict(kind="const", offset=v) for v in (0.2, 0.4, 0.7)]
    ys = []
    for mode in (0, 1):
        r = sr.apply_sources(runner(m, N, emu_lib), kinds)
        r.set_balance(mode)
        ys.append(r.run_sources(T_PROP))
        if mode == 0:
            u = r.render_sources(T_PROP)
    # (render after the run: the clock has advanced -- set it back)
    assert np.array_equal(ys[0], ys[1])
    twin = runner(m, N, emu_lib)
    r.source_clock = 0
    assert np.array_equal(twin.run(r.render_sources(T_PROP), time_major=True), ys[0])


# ---- 3. end to end with the measurement -----------------------------------------------------------------------------------------
def test_a_measured_sine_source_is_found_in_its_bin(emu_lib):
    from exact_ref import exact_moments, reported
    N, f_den, f_num, periods = 4, 96, 5, 3
    T = f_den * periods                                # whole periods of every f_num / f_den
    rng = np.random.default_rng(2)
    amp, off = np.logspace(-2, 1, N), rng.standard_normal(N)
    phase = np.array([0, 7, 48, 95])
    r = runner(sr.wire_model(1, FS), N, emu_lib)
    r.set_source(0, "sine", amp=amp, offset=off, f_den=f_den, f_num=f_num, phase=phase)
    H = 4
    r.set_measurement(f0=(f_num, f_den), harmonics=H)
    u = r.render_sources(T)
    r.measure(T=T)
    out, count = sr.raw_measurement(r)
    assert count == T
    # the accumulators against the extended-precision sums over the rendered signal, within exact_ref's bounds ...
    C_, S_, l1 = ld_harmonics(u, (f_num, f_den), H)
    Cg, Sg = unscale(out, count)
    bound = harmonic_bound(T, l1)[:, :, None]
    assert (np.abs(Cg - C_) <= bound).all() and (np.abs(Sg - S_) <= bound).all()
    # ... and the signal's own content: A_1 = amp exp(j (phase angle - pi / 2)) (a sine is a cosine a quarter turn late),
    # nothing in the harmonics, the mean the offset -- each within the same bound, scaled as the report scales (2 / count),
    # plus the rendered samples' own error (source_ref.sine_bound per sample, summed by the correlation)
    A = out[:, 0, 4::2] + 1j * out[:, 0, 5::2]
    th = 2 * np.pi * phase / f_den - np.pi / 2
    tol = 2.0 / T * (harmonic_bound(T, l1)[:, 0] + T * np.array([sr.sine_bound(a, o) for a, o in zip(amp, off)])) + 4 * U * amp
    assert (np.abs(A[:, 0] - amp * np.exp(1j * th)) <= np.sqrt(2) * tol).all(), np.abs(A[:, 0] - amp * np.exp(1j * th)) / tol
    assert (np.abs(A[:, 1:]) <= np.sqrt(2) * tol[:, None]).all()
    s, sq, mn, mx = exact_moments(u)
    mean, rms = reported((s, sq), count)
    assert np.array_equal(out[:, :, 0], mean)
    assert (np.abs(out[:, 0, 0] - off) <= (T + 2) * U * l1[:, 0] / T + np.array([sr.sine_bound(a, o) for a, o in zip(amp, off)])).all()


def test_a_frequency_sweep_is_one_batch(emu_lib):
    """per-instance frequencies: each instance's own bin is found when the measurement is armed at that frequency"""
    N, f_den = 4, 120
    f_num = np.array([3, 8, 15, 24])
    T = 2 * f_den
    r = runner(sr.wire_model(1, FS), N, emu_lib)
    r.set_source(0, "sine", f_den=f_den, f_num=f_num, amp=2.0)
    for i in range(N):
        r.source_clock = 0
        r.set_measurement(f0=(int(f_num[i]), f_den), harmonics=1)
        r.measure(T=T)
        a1 = np.abs(r.measurement().harmonics[:, 0, 0])
        assert abs(a1[i] - 2.0) < 1e-12
        assert (np.delete(a1, i) < 1e-12).all(), a1


# ---- 4. validation and interplay ------------------------------------------------------------------------------------------------
def rc(lib, code):
    return code, lib.L.acme_last_error().decode()


def test_argument_errors(emu_lib):
    L, N = emu_lib.L, 3
    r = runner(sr.wire_model(2, FS), N, emu_lib)
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_longlong)
    d = lambda *v: (C.c_double * len(v))(*v)           # noqa: E731
    ll = lambda *v: (C.c_longlong * len(v))(*v)        # noqa: E731
    INVALID, UNSUPPORTED = -1, -2
    assert L.acme_batch_run_sources(r.h, None, None, 8, 0, None) == INVALID         # nothing armed
    assert L.acme_batch_render_sources(r.h, None, d(*[0.0] * 48), 8, 0, None) == INVALID
    n = C.c_longlong(0)
    assert L.acme_batch_get_source_clock(r.h, C.byref(n)) == INVALID and L.acme_batch_set_source_clock(r.h, 5) == INVALID
    for row in (-1, 2, 64, 100):
        assert L.acme_batch_set_source_const(r.h, row, None) == INVALID, row
    for f_den in (0, -5, 2 ** 31, 2 ** 40):
        assert L.acme_batch_set_source_sine(r.h, 0, f_den, None, None, None, None) == INVALID, f_den
    assert L.acme_batch_set_source_sine(r.h, 0, 100, ll(0, 100, 1), None, None, None) == INVALID
    assert L.acme_batch_set_source_sine(r.h, 0, 100, ll(0, -1, 1), None, None, None) == INVALID
    assert L.acme_batch_set_source_sine(r.h, 0, 100, None, ll(0, 1, 100), None, None) == INVALID
    assert L.acme_batch_set_source_sine(r.h, 0, 100, None, ll(-1, 1, 1), None, None) == INVALID
    for P in (0, -1, 2 ** 24 + 1):
        assert L.acme_batch_set_source_table(r.h, 0, d(1.0), P, None, None) == INVALID, P
    assert L.acme_batch_set_source_table(r.h, 0, None, 4, None, None) == INVALID
    for bad in (np.nan, np.inf, -np.inf):
        assert L.acme_batch_set_source_const(r.h, 0, d(0.0, bad, 0.0)) == INVALID
        assert L.acme_batch_set_source_sine(r.h, 0, 100, None, None, d(1.0, 1.0, bad), None) == INVALID
        assert L.acme_batch_set_source_table(r.h, 0, d(1.0), 1, None, d(bad, 0.0, 0.0)) == INVALID
    assert L.acme_batch_get_source_clock(r.h, C.byref(n)) == INVALID                # (none of these armed anything)
    # armed: the clock, the u-taking entry points
    assert L.acme_batch_set_source_const(r.h, 1, d(1.0, 2.0, 3.0)) == 0
    assert L.acme_batch_set_source_clock(r.h, -1) == INVALID
    assert L.acme_batch_get_source_clock(r.h, None) == INVALID
    y, uv, u = np.zeros((N, 8, 2)), np.zeros((N, 8, 1)), np.zeros((N, 8, 2))
    assert L.acme_batch_run_sources(r.h, None, y.ctypes.data, 8, 0, None) == INVALID            # row 0 is the caller's
    assert L.acme_batch_run_sources(r.h, uv.ctypes.data, None, 8, 0, None) == INVALID           # y = NULL, nothing measured
    assert L.acme_batch_run_sources(r.h, uv.ctypes.data, y.ctypes.data, -1, 0, None) == INVALID
    assert L.acme_batch_run_sources(r.h, uv.ctypes.data, y.ctypes.data, 8, 7, None) == INVALID
    assert L.acme_batch_render_sources(r.h, None, None, 8, 0, None) == INVALID
    assert L.acme_batch_set_source_clock(r.h, 2 ** 63 - 4) == 0
    assert L.acme_batch_run_sources(r.h, uv.ctypes.data, y.ctypes.data, 8, 0, None) == INVALID  # the clock would overflow
    assert L.acme_batch_set_source_clock(r.h, 0) == 0
    for code, msg in (rc(emu_lib, L.acme_batch_run(r.h, u.ctypes.data, y.ctypes.data, 8, 0, None)),
                      rc(emu_lib, L.acme_batch_run_const(r.h, uv.ctypes.data, np.zeros((N, 2)).ctypes.data, 2, y.ctypes.data, 8, 0, None)),
                      rc(emu_lib, L.acme_batch_run_const(r.h, u.ctypes.data, np.zeros((N, 2)).ctypes.data, 0, y.ctypes.data, 8, 0, None)),
                      rc(emu_lib, L.acme_batch_run_async(r.h, u.ctypes.data, y.ctypes.data, 8, 0, None))):
        assert code == INVALID and "acme_batch_run_sources" in msg, (code, msg)
    assert L.acme_batch_wait(r.h) == 0
    assert L.acme_batch_run_sources(r.h, uv.ctypes.data, y.ctypes.data, 8, 0, None) == 0
    assert np.array_equal(y[:, :, 1], np.array([1.0, 2.0, 3.0])[:, None] * np.ones(8))


def test_not_together_with_isolation(emu_lib):
    L = emu_lib.L
    m = load("superover_var", HS)
    r = runner(m, 2, emu_lib)
    r.set_isolation(20.0)
    assert L.acme_batch_set_source_const(r.h, 1, None) == -2
    r.set_isolation(0.0)
    assert L.acme_batch_set_source_const(r.h, 1, None) == 0
    assert L.acme_batch_set_isolation(r.h, C.c_double(20.0)) == -2
    r.clear_source(1)
    assert L.acme_batch_set_isolation(r.h, C.c_double(20.0)) == 0


def test_clearing_restores_the_plain_batch(emu_lib):
    """acme_batch_run refused while armed, accepted after clear_source(-1); the run is then that of a batch that never had a
    source; the next first source starts the clock at 0"""
    from acme_jl_amd.runner import AcmeError
    m, N, T = load("diodeclipper", HS), 3, 60
    u = np.ascontiguousarray((np.logspace(-1, 0.5, N)[:, None] * np.sin(0.3 * np.arange(T))[None])[:, :, None])
    r = runner(m, N, emu_lib)
    r.set_source(0, "sine", f_den=100, f_num=3)
    r.source_clock = 77
    with pytest.raises(AcmeError, match="acme_batch_run_sources"):
        r.run(u, time_major=True)
    r.clear_source(-1)
    with pytest.raises(AcmeError, match="no input row has a source"):
        r.source_clock
    y = r.run(u, time_major=True)
    never = runner(m, N, emu_lib)
    assert np.array_equal(y, never.run(u, time_major=True))
    for a, b in zip(r.get_state(), never.get_state()):
        assert np.array_equal(a, b)
    r.set_source(0, "const", offset=1.0)
    assert r.source_clock == 0
    # replacing a row's source keeps the clock; clearing one of two rows too
    w = runner(sr.wire_model(2, FS), 2, emu_lib)
    w.set_source(0, "const", offset=1.0).set_source(1, "table", table=[1.0, 2.0, 3.0])
    assert np.array_equal(w.run_sources(4)[0, :, 1], [1.0, 2.0, 3.0, 1.0]) and w.source_clock == 4
    w.set_source(0, "sine", f_den=8, f_num=1)
    w.clear_source(1)
    assert w.source_clock == 4
    assert np.array_equal(w.render_sources(2, np.zeros((2, 2, 1)))[0, :, 0], w.render_sources(2)[0, :, 0])


def test_other_calls_leave_the_sources_and_the_clock_alone(emu_lib):
    m, N = load("diodeclipper", HS), 2
    kinds = [dict(kind="sine", f_den=FS, f_num=np.array([1000, 3000]), amp=np.array([0.5, 2.0]))]
    r = sr.apply_sources(runner(m, N, emu_lib, models=[m, m]), kinds)
    r.run_sources(30)
    before = r.render_sources(20)
    x, p, z = r.get_state()
    r.set_models(0, [m, m])
    r.set_state(x, p, z)
    r.reset_report()
    r.set_oversampling(2).set_oversampling(1)
    r.set_measurement(harmonics=0).reset_measurement().clear_measurement()
    assert r.source_clock == 30
    assert np.array_equal(r.render_sources(20), before)


def test_multi_device_runner_slices_the_parameters(emu_lib):
    from acme_jl_amd.runner import MultiDeviceRunner
    m, N, T = sr.wire_model(2, FS), 5, 30
    amp = np.arange(1.0, N + 1)
    table = np.arange(4.0)
    mr = MultiDeviceRunner(m, N, devices=[0, 0], lib=emu_lib)
    mr.set_source(0, "sine", f_den=50, f_num=np.arange(N), amp=amp).set_source(1, "table", table=table, offset=amp)
    one = runner(m, N, emu_lib).set_source(0, "sine", f_den=50, f_num=np.arange(N), amp=amp).set_source(1, "table", table=table, offset=amp)
    assert np.array_equal(mr.render_sources(T), one.render_sources(T))
    assert np.array_equal(mr.run_sources(T), one.run_sources(T))
    assert mr.source_clock == T
    mr.set_measurement(harmonics=0)
    mr.measure(T=T)
    assert mr.measurement().count == T and mr.source_clock == 2 * T
