"""PULSE and BURST rows (acme_batch_set_source_pulse / _burst, csrc/acme_source.h) on the CPU wave emulator: PULSE rows bit for bit
against pulse_ref's integer and fma replay at every clock, BURST rows == the SINE row where the envelope is 1, == the offset where
it is 0 and within source_ref.sine_bound of mpmath on the ramps, the render's independence of layout, slicing, call boundaries
and clock, every instantiation next to the other kinds, the defining property of the sources across memory kinds, stored and
measured runs, oversampling, split and asynchronous calls, the rows under an events measurement in closed form, argument errors,
clearing and the sharded runner.  The check_* functions take a runner factory: test_gpu_pulse_sources.py runs them on the MI355X."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import noise_ref as nr
import pulse_ref as pr
import source_ref as sr
from helpers import FS, HS, load
from test_sources import MODES, SLICE, T_PROP

INVALID, UNSUPPORTED = -1, -2
T_EXACT = 2 * 4096 + 1111                   # three slices of 4 096; the last ends mid-tile
EDGES = (0, 1, 255, 256, 511, 512, 4095, 4096, 4097, 8191, 8192, T_EXACT - 1)
PROP_CLOCK = 2 ** 31 + 1                    # (the step of the property cases starts 5 samples later)


def runner(model, n, lib, **kw):
    from acme_jl_amd.runner import ModelRunner
    return ModelRunner(model, n, lib=lib, **kw)


@pytest.fixture
def small_slices(monkeypatch):
    monkeypatch.setenv("ACME_OS_SLICE", str(SLICE))


@pytest.fixture
def tile_slices(monkeypatch):
    monkeypatch.setenv("ACME_OS_SLICE", "4096")


# ---- 1. PULSE, every element -------------------------------------------------------------------------------------------------------
def check_exact_pulse(make, clock):
    N, T = 9, T_EXACT
    k = pr.exact_pulses(clock, T)
    r = pr.apply_sources(make(sr.wire_model(1, FS), N), [k])
    r.source_clock = clock
    u = r.render_sources(T)
    want = pr.pulse_row(k, N, T, clock)
    assert np.array_equal(u[:, :, 0], want), np.argwhere(u[:, :, 0] != want)[:4]
    e, j = pr.envelope(k, N, T, clock)
    assert (e[0] == 0.0).all() and (e[1] == 1.0).all() and ((e[6] == 0.0) == (j[6] == 0)).all()      # always the offset; always high; low only at the ramp's foot
    assert (e[8, :T // 3] == 0.0).all() and e[8, T // 3 + 1000] == 1.0 and 0.0 < e[8, T // 3 + 1] < 1.0       # the step, its ramp
    y = r.run_sources(T)                                # the same through a source run of the pass-through model
    assert np.array_equal(y, u) and r.source_clock == clock + T


@pytest.mark.parametrize("clock", sr.CLOCKS)
def test_a_pulse_row_is_the_exact_one(emu_lib, tile_slices, clock):
    check_exact_pulse(lambda m, n: runner(m, n, emu_lib), clock)


def test_the_envelope_of_the_issue():
    """pulse_ref's own envelope at the points the issue states: 0 at j = 0, 1 at j = rise when on > 0 or fall > 0, never 1 with
    on = fall = 0; rise = fall = 0 high for exactly `on` samples"""
    e, j = pr.envelope(pr.pulse(period=[10, 10, 10, 10], on=[3, 0, 0, 4], rise=[4, 4, 4, 0], fall=[2, 2, 0, 0]), 4, 10, 0)
    assert np.array_equal(j[0], np.arange(10))
    assert e[0].tolist() == [0.0, 0.25, 0.5, 0.75, 1.0, 1.0, 1.0, 1.0, 0.5, 0.0]
    assert e[1].tolist() == [0.0, 0.25, 0.5, 0.75, 1.0, 0.5, 0.0, 0.0, 0.0, 0.0]
    assert e[2].tolist() == [0.0, 0.25, 0.5, 0.75] + [0.0] * 6
    assert e[3].tolist() == [1.0] * 4 + [0.0] * 6
    _, j = pr.envelope(pr.pulse(period=[7], on=[1], delay=[6]), 1, 3, 2 ** 62)
    assert j[0].tolist() == [(2 ** 62 - 6 + t) % 7 for t in range(3)]


# ---- 2. BURST ------------------------------------------------------------------------------------------------------------------------
def check_burst(make, clock, label):
    N, T = 7, T_EXACT
    k = pr.exact_bursts(N, clock, T)
    r = pr.apply_sources(make(sr.wire_model(2, FS), N), [k, pr.sine_of(k)])
    r.source_clock = clock
    u = r.render_sources(T)
    worst = pr.check_burst_row(u[:, :, 0], u[:, :, 1], k, N, T, clock, np.random.default_rng(8), edges=EDGES)
    print(f"{label}, clock {clock}: worst BURST ramp error {worst:.3f} of its bound")
    # the SINE row beside a BURST row (rendered as a burst of e = 1) is the SINE row of a launch without one, bit for bit
    s = pr.apply_sources(make(sr.wire_model(1, FS), N), [pr.sine_of(k)])
    s.source_clock = clock
    assert np.array_equal(s.render_sources(T)[:, :, 0], u[:, :, 1])
    sr.check_sine_row(u[:, :, 1], pr.sine_of(k), N, clock, [(i, t) for i in range(N) for t in (0, 511, 4096, T - 1)])
    return worst


@pytest.mark.parametrize("clock", [0, 2 ** 31 + 1, 2 ** 62])
def test_a_burst_row_is_the_sine_row_under_its_envelope(emu_lib, tile_slices, clock):
    check_burst(lambda m, n: runner(m, n, emu_lib), clock, "emulator")


# ---- 3. layout independence -----------------------------------------------------------------------------------------------------------
def six_rows(make, N, T, clock, uv):
    kinds = pr.layout_kinds(N)
    r = pr.apply_sources(make(sr.wire_model(6, FS), N), kinds)
    r.source_clock = clock
    return kinds, r.render_sources(T, uv)


def check_every_store_shape(make, monkeypatch, nu, lds):
    """one and two elements per thread (odd and even row counts, a single row with an even and an odd number of samples): a
    row's values are those of the six-row layout, the PULSE rows pulse_ref's, the TABLE row source_ref's"""
    N, clock = 6, 2 ** 40 + 1
    for T in (4096 + 5, 4096 + 600):
        uv = np.random.default_rng(T).standard_normal((N, T, 1))
        monkeypatch.setenv("ACME_SOURCE_LDS", "1")
        kinds, ref = six_rows(make, N, T, clock, uv)
        monkeypatch.setenv("ACME_SOURCE_LDS", lds)
        r = pr.apply_sources(make(sr.wire_model(nu, FS), N), kinds[:nu])
        r.source_clock = clock
        u = r.render_sources(T, uv if nu >= 3 else None)
        assert np.array_equal(u, ref[:, :, :nu]), (T, np.argwhere(u != ref[:, :, :nu])[:4])
        assert np.array_equal(u[:, :, 0], pr.pulse_row(kinds[0], N, T, clock))
        if nu >= 3:
            assert np.array_equal(u[:, :, 2], uv[:, :, 0])
        if nu >= 4:
            tab = sr.expected_rows([None] * 3 + [kinds[3]], N, 29, 0)[:, :, 3]
            assert np.array_equal(u[:, :, 3], tab[:, (clock + np.arange(T)) % 29])
        if nu >= 6:
            assert np.array_equal(u[:, :, 5], pr.pulse_row(kinds[5], N, T, clock))


@pytest.mark.parametrize("lds", ["1", "0"])
@pytest.mark.parametrize("nu", [1, 2, 3, 4, 5, 6])
def test_every_store_shape(emu_lib, monkeypatch, tile_slices, nu, lds):
    check_every_store_shape(lambda m, n: runner(m, n, emu_lib), monkeypatch, nu, lds)


def check_long_and_split_renders(make, monkeypatch):
    """one launch of more than a tile of samples against renders slice by slice; a render of T against renders of T1 + T2 with
    the cut inside a ramp of rows 0 and 1"""
    N, T, clock = 3, 4096 + 300, 2 ** 40 + 1
    uv = np.random.default_rng(0).standard_normal((N, T, 1))
    monkeypatch.setenv("ACME_OS_SLICE", "4096")
    kinds, short = six_rows(make, N, T, clock, uv)
    monkeypatch.setenv("ACME_OS_SLICE", "8192")
    kinds, long = six_rows(make, N, T, clock, uv)
    assert np.array_equal(long, short)
    assert np.array_equal(long[:, :, 0], pr.pulse_row(kinds[0], N, T, clock))
    monkeypatch.setenv("ACME_OS_SLICE", "4096")
    e0 = pr.envelope(kinds[0], N, T, clock)[0][0]
    e1 = pr.envelope(kinds[1], N, T, clock)[0][0]
    T1 = int(np.flatnonzero((e0 > 0) & (e0 < 1) & (e1 > 0) & (e1 < 1) & (np.arange(T) > 4096))[0])        # (inside ramps, past a slice)
    r = pr.apply_sources(make(sr.wire_model(6, FS), N), kinds)
    r.source_clock = clock
    a = r.render_sources(T1, uv[:, :T1])
    r.source_clock = clock + T1
    b = r.render_sources(T - T1, uv[:, T1:T])
    assert np.array_equal(np.concatenate([a, b], axis=1), short)


def test_a_long_launch_and_split_renders(emu_lib, monkeypatch):
    check_long_and_split_renders(lambda m, n: runner(m, n, emu_lib), monkeypatch)


def check_tail_renders(make):
    """a render from clock c is the tail of an earlier one: from 0 below 2^32, from shortly before c above it; the PULSE row
    pulse_ref's closed form at every clock"""
    N, T = 3, 4096 + 9
    kinds = [pr.pulse(period=[97, 513, 4099], on=[20, 100, 1000], delay=[96, 7, 0], rise=[3, 200, 1500], fall=[30, 1, 1599], amp=[1.0, -0.3, 7.0], offset=0.1),
             pr.burst(period=[97, 513, 4099], on=[20, 100, 1000], f_den=44100, f_num=[1000, 441, 7], delay=[96, 7, 0], rise=[3, 200, 1500], fall=[30, 1, 1599])]
    r = pr.apply_sources(make(sr.wire_model(2, FS), N), kinds)
    for c, back in ((4099 + 2 * 4096 + 1, None), (2 ** 32 + 3 * 4099 + 1, 4099 + 17), (2 ** 62 + 11, 50)):
        r.source_clock = c
        u = r.render_sources(T)
        start = 0 if back is None else c - back
        r.source_clock = start
        whole = r.render_sources(c - start + T)
        assert np.array_equal(whole[:, c - start:], u), c
        assert np.array_equal(u[:, :, 0], pr.pulse_row(kinds[0], N, T, c))


def test_a_render_from_a_clock_is_the_tail_of_an_earlier_one(emu_lib, tile_slices):
    check_tail_renders(lambda m, n: runner(m, n, emu_lib))


def check_next_to_the_other_kinds(make, N, T, clock):
    """PULSE and BURST rows next to a MULTISINE row, next to a NOISE row, next to both (the instantiation of every kind) and
    alone (the instantiation of the plain kinds and PULSE / BURST): each row is what every other launch renders for it, and what
    the launches without a PULSE row (the four older instantiations) render"""
    i = np.arange(N)
    multi = dict(kind="multisine", f_den=44100, f_num=np.array([[1000], [1900], [7]]), amp=np.array([[0.5], [0.25], [1.0]]), offset=np.linspace(-1, 1, N))
    kinds = [pr.pulse(period=513 + i, on=100 + i, delay=5 * i, rise=40, fall=3 * i, amp=np.linspace(1, 2, N), offset=np.linspace(0, 1, N)),
             multi, nr.noise("uniform", hold=5, amp=np.linspace(1, 2, N), offset=np.linspace(0, 1, N), seed=6),
             pr.burst(period=1000 + 7 * i, on=300, f_den=44100, f_num=1000 + i, delay=i, rise=100 + i, fall=50, amp=0.5)]
    renders = {}
    for sel in ((0, 1, 2, 3), (0, 1, 3), (0, 2, 3), (0, 3), (1, 2), (1,), (2,)):
        r = pr.apply_sources(make(sr.wire_model(4, FS), N), [k if c in sel else dict(kind="const", offset=1.0) for c, k in enumerate(kinds)])
        r.source_clock = clock
        renders[sel] = r.render_sources(T)
    every = renders[(0, 1, 2, 3)]
    for sel, u in renders.items():
        assert np.array_equal(u[:, :, list(sel)], every[:, :, list(sel)]), sel
    assert np.array_equal(every[:, :, 0], pr.pulse_row(kinds[0], N, T, clock))
    assert np.array_equal(every[:, :, 2], nr.uniform_row(kinds[2], 2, N, T, clock))
    assert np.abs(every[:, :, 1] - multi["offset"][:, None]).max() > 0.5 and np.abs(every[:, :, 3]).max() > 0.4


def test_next_to_the_other_kinds(emu_lib, tile_slices):
    check_next_to_the_other_kinds(lambda m, n: runner(m, n, emu_lib), 5, 4096 + 603, 2 ** 40 + 1)


# ---- 4. the defining property ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", range(len(MODES)))
@pytest.mark.parametrize("case", range(2))
def test_a_source_run_is_a_run_on_the_rendered_input(emu_lib, small_slices, case, mode):
    name, m, N, kinds = pr.property_cases(clock=PROP_CLOCK)[case]
    u = pr.check_defining_property(emu_lib, m, N, kinds, None, T_PROP, more=SLICE + 3, clock=PROP_CLOCK, **MODES[mode])
    assert np.abs(u[:, :, 0]).max() > 1e-2 and np.isfinite(u).all()
    if case == 1:       # the pot's ramp-and-hold: at its offset before the step, moving on the ramp
        assert (u[:, :5, 2] == 0.25).all() and (np.diff(u[:, 5:50, 2], axis=1) > 0).all()


@pytest.mark.parametrize("held", [False, True])
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("case", range(2))
def test_oversampled_source_runs(emu_lib, small_slices, case, k, held):
    """the rows generated at the base rate, then interpolated or held as a caller's row is"""
    name, m, N, kinds = pr.property_cases()[case]
    rows = [r for r, kd in enumerate(kinds) if kd["kind"] != "const"] if held else []
    for mode in (dict(mem=0, keep=True, split=SLICE + 7), dict(mem=1, keep=False)):
        pr.check_defining_property(emu_lib, m, N, kinds, None, T_PROP, k=k, held=rows, more=SLICE + 3, **mode)


# ---- 5. with the forms it serves ------------------------------------------------------------------------------------------------------
def check_pulse_under_events(make):
    """closed forms, no replay: ideal pulses (rise = fall = 0) under a comparator at mid-level -- rises and falls are the whole
    periods in the window, HIGH samples on x that, frequency 1 / P, duty on / P; per-instance P and on: a PWM sweep in one batch"""
    T = 9240                                            # = 2^3 3 5 7 11: every period below divides it
    P = np.array([8, 21, 105, 440, 1155, 3080, 4620])
    on = np.array([1, 19, 52, 110, 1000, 77, 2310])
    d = np.array([1, 1, 50, 300, 100, 3000, 2000])      # (the window starts low and every period's pulse ends inside it)
    N = len(P)
    r = make(sr.wire_model(1, FS), N)
    r.set_source(0, "pulse", period=P, on=on, delay=d, amp=2.0, offset=-0.5)
    r.set_measurement(harmonics=0).set_measurement_events(levels=0.5, slots=2)
    r.measure(T=T)
    ev = r.measurement_events()
    assert ev.count == T
    assert np.array_equal(ev.rises[:, 0, 0], T // P) and np.array_equal(ev.falls[:, 0, 0], T // P)
    assert np.array_equal(ev.high[:, 0, 0], on * (T // P)) and np.array_equal(ev.low[:, 0, 0], T - on * (T // P))
    assert np.array_equal(ev.frequency(1.0)[:, 0], 1.0 / P)
    assert np.array_equal(ev.duty()[:, 0], on / P)


def test_a_pulse_under_an_events_measurement(emu_lib, tile_slices):
    check_pulse_under_events(lambda m, n: runner(m, n, emu_lib))


def check_edge_time_sweep(make):
    """per-instance rise times in one batch, levels at 10 % and 90 %: transition_time is 0.8 r -- the linear interpolation of a
    linear ramp is exact but for rounding: within 4 x 2^-53 r"""
    rise = np.array([10, 50, 64, 100, 333, 1000, 4097, 7001])
    N, T = len(rise), T_EXACT
    r = make(sr.wire_model(1, FS), N)
    r.set_source(0, "step", at=2, rise=rise)
    r.set_measurement(harmonics=0).set_measurement_events(levels=[0.1, 0.9], slots=1)
    r.measure(T=T)
    tt = r.measurement_events().transition_time(0, 1)[:, 0]
    for i in range(N):
        err = abs(Fraction(float(tt[i])) - Fraction(4 * int(rise[i]), 5))
        print(f"rise {rise[i]}: transition_time {tt[i]!r}, error {float(err / rise[i]) * 2.0 ** 53:.3f} x 2^-53 r")
        assert err <= Fraction(4 * int(rise[i]), 2 ** 53), (i, tt[i])


def test_an_edge_time_sweep(emu_lib, tile_slices):
    check_edge_time_sweep(lambda m, n: runner(m, n, emu_lib))


def test_a_step_is_a_pulse_of_the_longest_period(emu_lib, small_slices):
    N, T = 3, 40
    a, b = runner(sr.wire_model(1, FS), N, emu_lib), runner(sr.wire_model(1, FS), N, emu_lib)
    a.set_source(0, "step", at=[3, 5, 0], rise=[0, 4, 2], amp=0.7, offset=0.1)
    at, rise = np.array([3, 5, 0]), np.array([0, 4, 2])
    b.set_source(0, "pulse", period=pr.PMAX, delay=at, rise=rise, on=pr.PMAX - at - rise, amp=0.7, offset=0.1)
    u = a.render_sources(T)
    assert np.array_equal(u, b.render_sources(T))
    assert u[0, :3, 0].tolist() == [0.1] * 3 and (u[0, 3:, 0] == 0.7 + 0.1).all() and u[1, 7, 0] == pr.fma_fast(0.7, 0.5, 0.1)
    a.source_clock = pr.PMAX - 2                        # it wraps at clock 2^31 - 1 + at: low again from 2^31 - 1 for `at` samples
    assert a.render_sources(6)[0, :, 0].tolist() == [0.7 + 0.1] * 2 + [0.1] * 3 + [0.7 + 0.1]


def test_a_burst_row_lends_its_frequency(emu_lib, small_slices):
    r = runner(sr.wire_model(1, FS), 2, emu_lib)
    r.set_source(0, "burst", period=100, on=50, f_den=100, f_num=[3, 5])
    r.set_measurement(f0_from_source=0, harmonics=2)
    r.set_source(0, "pulse", period=100, on=50)
    with pytest.raises(ValueError, match="no sine source"):
        r.set_measurement(f0_from_source=0, harmonics=2)


# ---- 6. arguments ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors(emu_lib, small_slices):
    L, N = emu_lib.L, 3
    r = runner(sr.wire_model(2, FS), N, emu_lib)
    d = lambda *v: (C.c_double * len(v))(*v)            # noqa: E731
    err = lambda: L.acme_last_error().decode()          # noqa: E731

    def shape(P=(10, 10, 10), delay=(0, 0, 0), rise=(1, 1, 1), on=(2, 2, 2), fall=(1, 1, 1)):
        return (C.c_longlong * 15)(*P, *delay, *rise, *on, *fall)
    ll = lambda *v: (C.c_longlong * len(v))(*v)         # noqa: E731
    pulse = lambda s, amp=None, off=None: L.acme_batch_set_source_pulse(r.h, 0, s, amp, off)       # noqa: E731
    burst = lambda s, den=100, fn=None, ph=None, amp=None, off=None: L.acme_batch_set_source_burst(r.h, 0, s, den, fn, ph, amp, off)      # noqa: E731
    r.set_source(0, "sine", f_den=100, f_num=3, amp=0.5)            # the row's previous source
    before = r.render_sources(30)
    for call, kind in ((pulse, "pulse"), (burst, "burst")):
        for row in (-1, 2, 64):
            fn = L.acme_batch_set_source_pulse if kind == "pulse" else L.acme_batch_set_source_burst
            args = (shape(), None, None) if kind == "pulse" else (shape(), 100, None, None, None, None)
            assert fn(r.h, row, *args) == INVALID and "row" in err(), row
        assert call(None) == INVALID and "null shape" in err() and kind in err()
        for bad, word, inst in ((dict(P=(10, 0, 10)), "period", 1), (dict(P=(10, 10, 2 ** 31)), "period", 2), (dict(P=(-5, 10, 10)), "period", 0),
                                (dict(delay=(0, 10, 0)), "delay", 1), (dict(delay=(0, 0, -1)), "delay", 2),
                                (dict(rise=(-1, 1, 1)), "negative", 0), (dict(on=(2, -2, 2)), "negative", 1), (dict(fall=(1, 1, -7)), "negative", 2),
                                (dict(rise=(1, 8, 1)), "rise + on + fall", 1), (dict(on=(2, 2, 2 ** 62)), "rise + on + fall", 2)):
            assert call(shape(**bad)) == INVALID and word in err() and f"instance {inst})" in err(), (bad, err())
        for v in (np.nan, np.inf, -np.inf):
            assert call(shape(), amp=d(1.0, v, 1.0)) == INVALID and "non-finite" in err() and "instance 1" in err()
            assert call(shape(), off=d(v, 0.0, 0.0)) == INVALID and "non-finite" in err() and "instance 0" in err()
    for den in (0, -1, 2 ** 31):
        assert burst(shape(), den=den) == INVALID and "f_den" in err()
    assert burst(shape(), fn=ll(0, 100, 0)) == INVALID and "instance 1" in err()
    assert burst(shape(), ph=ll(0, 0, -1)) == INVALID and "instance 2" in err()
    assert np.array_equal(r.render_sources(30), before)             # every refused call left the row as it was
    # the limits themselves are accepted
    assert pulse(shape(P=(1, 2 ** 31 - 1, 10), delay=(0, 2 ** 31 - 2, 9), rise=(0, 0, 10), on=(1, 2 ** 31 - 1, 0), fall=(0, 0, 0))) == 0
    assert burst(shape(P=(1, 2 ** 31 - 1, 10), delay=(0, 0, 9), rise=(0, 2 ** 31 - 1, 0), on=(0, 0, 0), fall=(0, 0, 10)), den=2 ** 31 - 1) == 0
    u = np.full((N, 6, 2), np.nan)
    assert L.acme_batch_render_sources(r.h, None, u.ctypes.data, 6, 0, None) == 0 and np.isfinite(u[:, :, 0]).all()
    y = np.zeros((N, 6, 2))
    for fn in (L.acme_batch_run, L.acme_batch_run_async):           # refused while a row is armed
        assert fn(r.h, u.ctypes.data, y.ctypes.data, 6, 0, None) == INVALID and "acme_batch_run_sources" in err()
    assert L.acme_batch_wait(r.h) == 0
    # Python: the keywords' own refusals
    with pytest.raises(ValueError, match="period and on"):
        r.set_source(0, "pulse", period=10)
    with pytest.raises(ValueError, match="f_den"):
        r.set_source(0, "burst", period=10, on=1)
    with pytest.raises(ValueError, match="step source"):
        r.set_source(0, "step", at=1, period=10)
    with pytest.raises(ValueError, match="belong to a pulse"):
        r.set_source(0, "sine", f_den=100, period=10)
    with pytest.raises(Exception, match="integers"):
        r.set_source(0, "pulse", period=10.5, on=1)


def test_not_together_with_isolation(emu_lib):
    L = emu_lib.L
    r = runner(load("superover_var", HS), 2, emu_lib)
    s = (C.c_longlong * 10)(10, 10, 0, 0, 1, 1, 2, 2, 1, 1)
    r.set_isolation(20.0)
    assert L.acme_batch_set_source_pulse(r.h, 0, s, None, None) == UNSUPPORTED and "isolation" in L.acme_last_error().decode()
    assert L.acme_batch_set_source_burst(r.h, 0, s, 100, None, None, None, None) == UNSUPPORTED
    r.set_isolation(0.0)
    assert L.acme_batch_set_source_pulse(r.h, 0, s, None, None) == 0
    assert L.acme_batch_set_isolation(r.h, C.c_double(20.0)) == UNSUPPORTED


def test_replacing_and_clearing(emu_lib, small_slices):
    """a pulse row replaced by a burst and back renders what it rendered; clear_source followed by a plain run is a batch that
    never had a source"""
    from acme_jl_amd.runner import AcmeError
    m, N, T = load("diodeclipper", HS), 3, SLICE + 6
    r = runner(m, N, emu_lib)
    spec = dict(period=[7, 11, 13], on=[2, 3, 4], rise=[1, 2, 3], fall=[1, 0, 6], amp=0.8)
    r.set_source(0, "pulse", **spec)
    first = r.render_sources(T)
    assert np.array_equal(first[:, :, 0], pr.pulse_row(pr.pulse(offset=None, delay=0, **spec), N, T, 0))
    r.set_source(0, "burst", f_den=100, f_num=3, **spec)
    assert not np.array_equal(r.render_sources(T), first)
    r.set_source(0, "pulse", **spec)
    assert np.array_equal(r.render_sources(T), first)
    with pytest.raises(AcmeError, match="acme_batch_run_sources"):
        r.run(first, time_major=True)
    r.clear_source(0)
    y = r.run(first, time_major=True)
    never = runner(m, N, emu_lib)
    assert np.array_equal(y, never.run(first, time_major=True))
    for a, b in zip(r.get_state(), never.get_state()):
        assert np.array_equal(a, b)


def test_multi_device_runner_slices_the_five_columns(emu_lib, small_slices):
    from acme_jl_amd.runner import MultiDeviceRunner
    m, N, T = sr.wire_model(3, FS), 5, SLICE + 16
    i = np.arange(N)

    def arm(r):
        r.set_source(0, "pulse", period=7 + i, on=2 + i % 2, delay=i, rise=1 + i % 3, fall=i % 2, amp=1.0 + i, offset=0.1 * i)
        r.set_source(1, "burst", period=20, on=5 + i, f_den=100, f_num=3 + i, phase=i, rise=2, fall=i)
        return r.set_source(2, "step", at=3 + i, rise=i, amp=0.5)
    mr, one = arm(MultiDeviceRunner(m, N, devices=[0, 0], lib=emu_lib)), arm(runner(m, N, emu_lib))
    u = one.render_sources(T)
    assert np.array_equal(mr.render_sources(T), u)
    assert np.array_equal(u[:, :, 0], pr.pulse_row(pr.pulse(period=7 + i, on=2 + i % 2, delay=i, rise=1 + i % 3, fall=i % 2, amp=1.0 + i, offset=0.1 * i), N, T, 0))
    assert np.array_equal(mr.run_sources(T), one.run_sources(T)) and mr.source_clock == T
