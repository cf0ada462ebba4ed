"""NOISE rows (acme_batch_set_source_noise, csrc/acme_source.h) on the CPU wave emulator: the published Philox known answers,
UNIFORM rows bit for bit and GAUSSIAN rows within noise_ref.gauss_bound against arithmetic that shares no code with the
library, the render's independence of layout, slicing, call boundaries and clock, the separation of rows and streams, the
defining property of the sources across memory kinds, stored and measured runs, oversampling, split and asynchronous calls,
the moments through the measurement, the draws' statistics, argument errors and the sharded runner."""
import ctypes as C

import numpy as np
import pytest

import noise_ref as nr
import source_ref as sr
from helpers import FS, HS, load
from test_sources import MODES, SLICE, T_PROP

INVALID, UNSUPPORTED = -1, -2


def runner(model, n, lib, **kw):
    from acme_jl_amd.runner import ModelRunner
    return ModelRunner(model, n, lib=lib, **kw)


@pytest.fixture(autouse=True)
def small_slices(monkeypatch):
    monkeypatch.setenv("ACME_OS_SLICE", str(SLICE))


# ---- 1. known answers -------------------------------------------------------------------------------------------------------------
def test_known_answers(emu_lib):
    for counter, key, out in nr.KNOWN_ANSWERS:
        assert nr.philox(counter, key) == out
        q, s = counter[0] + (counter[1] << 32), key[0] + (key[1] << 32)
        if counter[3] == 0:         # (the vectorised form has the sources' counter layout: the fourth word is 0)
            assert tuple(int(w[0]) for w in nr.words(s, counter[2], [q])) == out
    assert tuple(int(w[0]) for w in nr.words(-1, 7, [2 ** 40 + 3])) == nr.philox((3, 256, 7, 0), (0xFFFFFFFF, 0xFFFFFFFF))
    # the library: counter and key all zero -- row 0, stream 0, clock 0 -- gives the first published vector's words
    r = runner(sr.wire_model(1, FS), 1, emu_lib)
    r.set_source(0, "noise", dist="uniform", stream=[0])
    x = 0x6627e8d5 + 2 ** 32 * (0xe169c58d % 2 ** 21)
    want = (2 * x + 1 - 2 ** 53) / 2.0 ** 53            # (an odd integer below 2^53 over a power of two: exact)
    assert r.render_sources(3)[0, 0, 0] == want


# ---- 2. exact rows ----------------------------------------------------------------------------------------------------------------
def exact_kinds(N, rng):
    stream = ([-1, 2 ** 63 - 1, -2 ** 63, 7, (12345 << 32) + 6] + list(range(100, 100 + N)))[:N]
    return [nr.noise("uniform", stream=stream, amp=rng.standard_normal(N) * 10.0 ** rng.integers(-3, 4, N), offset=rng.standard_normal(N)),
            nr.noise("gaussian"),
            nr.noise("uniform", hold=7)]


@pytest.mark.parametrize("clock", sr.CLOCKS)
def test_rendered_rows_are_the_exact_ones(emu_lib, clock):
    N, T = 5, 2 * SLICE + 11
    kinds = exact_kinds(N, np.random.default_rng(1))
    r = nr.apply_sources(runner(sr.wire_model(3, FS), N, emu_lib), kinds)
    r.source_clock = clock
    u = r.render_sources(T)
    for row in (0, 2):
        want = nr.uniform_row(kinds[row], row, N, T, clock)
        assert np.array_equal(u[:, :, row], want), (row, np.argwhere(u[:, :, row] != want)[:4])
    worst = nr.check_gauss_row(u[:, :, 1], kinds[1], 1, N, clock, [(i, t) for i in range(N) for t in range(T)])
    print(f"clock {clock}: worst Gaussian error {worst:.3f} of its bound")
    # the held row: constant over the blocks of 7 samples aligned to the clock, changing from block to block
    q = (clock + np.arange(T)) // 7
    for i in range(N):
        for b in np.unique(q):
            assert len(set(u[i, q == b, 2])) == 1
        firsts = [u[i, q == b, 2][0] for b in np.unique(q)]
        assert all(a != b for a, b in zip(firsts, firsts[1:]))
    y = r.run_sources(T)                                # the same through a source run of the pass-through model
    assert np.array_equal(y, u) and r.source_clock == clock + T


# ---- 3. layout independence -------------------------------------------------------------------------------------------------------
def layout_reference(lib, N, T, clock, uv):
    kinds = nr.layout_kinds(N)
    r = nr.apply_sources(runner(sr.wire_model(6, FS), N, lib), kinds)
    r.source_clock = clock
    return kinds, r.render_sources(T, uv)


@pytest.mark.parametrize("lds", ["1", "0"])
@pytest.mark.parametrize("nu", [1, 2, 3, 4, 5, 6])
def test_every_store_shape(emu_lib, monkeypatch, nu, lds):
    """one and two elements per thread (odd and even row counts, a single row with an even and an odd number of samples): a
    row's values are those of the six-row layout -- they depend on (stream, row, clock) alone -- and the UNIFORM rows
    noise_ref's"""
    N, clock = 6, 4095
    for T in (SLICE + 5, 2 * SLICE):
        uv = np.random.default_rng(T).standard_normal((N, T, 1))
        monkeypatch.setenv("ACME_SOURCE_LDS", "1")
        kinds, ref = layout_reference(emu_lib, N, T, clock, uv)
        monkeypatch.setenv("ACME_SOURCE_LDS", lds)
        r = nr.apply_sources(runner(sr.wire_model(nu, FS), N, emu_lib), kinds[:nu])
        r.source_clock = clock
        u = r.render_sources(T, uv if nu >= 3 else None)
        assert np.array_equal(u, ref[:, :, :nu]), (T, np.argwhere(u != ref[:, :, :nu])[:4])
        if nu >= 3:
            assert np.array_equal(u[:, :, 2], uv[:, :, 0])
        for row in (1, 5):
            if row < nu:
                assert np.array_equal(u[:, :, row], nr.uniform_row(kinds[row], row, N, T, clock))
        if nu >= 4:
            assert np.array_equal(u[:, :, 3], sr.expected_rows([None] * 3 + [kinds[3]], N, T, clock)[:, :, 3])


def test_a_long_launch_and_split_renders(emu_lib, monkeypatch):
    """one launch of more than a tile of samples against renders slice by slice; a render of T against renders of T1 + T2 with
    the cut inside a slice"""
    N, T, clock = 3, 4096 + 300, 2 ** 40 + 1
    uv = np.random.default_rng(0).standard_normal((N, T, 1))
    kinds, short = layout_reference(emu_lib, N, T, clock, uv)
    monkeypatch.setenv("ACME_OS_SLICE", "8192")
    kinds, long = layout_reference(emu_lib, N, T, clock, uv)
    assert np.array_equal(long, short)
    assert np.array_equal(long[:, :, 5], nr.uniform_row(kinds[5], 5, N, T, clock))
    monkeypatch.setenv("ACME_OS_SLICE", str(SLICE))
    T, T1 = 3 * SLICE + 5, SLICE + 7
    r = nr.apply_sources(runner(sr.wire_model(6, FS), N, emu_lib), kinds)
    r.source_clock = clock
    a = r.render_sources(T1, uv[:, :T1])
    r.source_clock = clock + T1
    b = r.render_sources(T - T1, uv[:, T1:T])
    assert np.array_equal(np.concatenate([a, b], axis=1), short[:, :T])


@pytest.mark.parametrize("hold", [1, 3, 4096 + 5])
def test_a_render_from_a_clock_is_the_tail_of_an_earlier_one(emu_lib, hold):
    """below 2^32 literally the tail of a render from 0; above 2^32, where nobody renders from 0, the tail of a render that
    starts mid-block before it; at every clock the closed form from 0: noise_ref's uniform row with ==, the Gaussian row against
    mpmath"""
    N, T = 3, SLICE + 9
    kinds = [nr.noise("uniform", hold=hold, seed=2), nr.noise("gaussian", hold=hold, seed=2)]
    r = nr.apply_sources(runner(sr.wire_model(2, FS), N, emu_lib), kinds)
    for c, back in ((4096 + 5 + 2 * SLICE + 1, None), (2 ** 32 + 3 * (4096 + 5) + 1, 4096 + 5 + 17), (2 ** 62 + 11, 50)):
        r.source_clock = c
        u = r.render_sources(T)
        start = 0 if back is None else c - back
        r.source_clock = start
        whole = r.render_sources(c - start + T)
        assert np.array_equal(whole[:, c - start:], u), (c, hold)
        assert np.array_equal(u[:, :, 0], nr.uniform_row(kinds[0], 0, N, T, c))
        nr.check_gauss_row(u[:, :, 1], kinds[1], 1, N, c, [(i, t) for i in range(N) for t in range(T)])


def check_noise_next_to_a_multisine(make, N, T, clock):
    """a launch that holds NOISE and MULTISINE rows (the fourth instantiation): each row is what the launches with one of the
    two kinds render"""
    multi = dict(kind="multisine", f_den=44100, f_num=np.array([[1000], [1900], [7]]), amp=np.array([[0.5], [0.25], [1.0]]), offset=np.linspace(-1, 1, N))
    kinds = [nr.noise("uniform", hold=5, amp=np.linspace(1, 2, N), offset=np.linspace(0, 1, N), seed=6), multi, nr.noise("gaussian", seed=6)]
    renders = []
    for sel in ((0, 1, 2), (0, 2), (1,)):
        r = nr.apply_sources(make(sr.wire_model(3, FS), N), [k if c in sel else dict(kind="const", offset=1.0) for c, k in enumerate(kinds)])
        r.source_clock = clock
        renders.append(r.render_sources(T))
    both, noise_only, multi_only = renders
    assert np.array_equal(both[:, :, [0, 2]], noise_only[:, :, [0, 2]]) and np.array_equal(both[:, :, 1], multi_only[:, :, 1])
    assert np.array_equal(both[:, :, 0], nr.uniform_row(kinds[0], 0, N, T, clock))
    assert np.abs(both[:, :, 1] - kinds[1]["offset"][:, None]).max() > 0.5


def test_noise_next_to_a_multisine(emu_lib):
    check_noise_next_to_a_multisine(lambda m, n: runner(m, n, emu_lib), 5, 2 * SLICE + 3, 2 ** 40 + 1)


# ---- 4. rows and streams ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", ["uniform", "gaussian"])
def test_rows_and_streams_are_separate(emu_lib, dist):
    N, T = 4, SLICE + 5
    stream = [5, 77, 5, -3]
    r = runner(sr.wire_model(2, FS), N, emu_lib)
    r.set_source(0, "noise", dist=dist, stream=stream).set_source(1, "noise", dist=dist, stream=stream)
    u = r.render_sources(T)
    assert not (u[:, :, 0] == u[:, :, 1]).any()                 # the same stream on two rows: different sequences
    assert np.array_equal(u[0], u[2]) and not (u[0] == u[1]).any()      # the same stream on one row: the same sequence
    swapped = [77, 5, 5, -3]
    r.set_source(0, "noise", dist=dist, stream=swapped).set_source(1, "noise", dist=dist, stream=swapped)
    v = r.render_sources(T)
    assert np.array_equal(v[0], u[1]) and np.array_equal(v[1], u[0]) and np.array_equal(v[2:], u[2:])


# ---- 5. the defining property -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", range(len(MODES)))
@pytest.mark.parametrize("case", range(2))
def test_a_noise_source_run_is_a_run_on_the_rendered_input(emu_lib, case, mode):
    name, m, N, kinds = nr.property_cases()[case]
    u = nr.check_defining_property(emu_lib, m, N, kinds, None, T_PROP, more=SLICE + 3, clock=2 ** 31 - 20, **MODES[mode])
    assert np.abs(u[:, :, 0]).max() > 1e-2 and np.isfinite(u).all()


@pytest.mark.parametrize("held", [False, True])
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("case", range(2))
def test_oversampled_noise_source_runs(emu_lib, case, k, held):
    """the noise row generated at the base rate, then interpolated or held as a caller's row is"""
    name, m, N, kinds = nr.property_cases()[case]
    for mode in (dict(mem=0, keep=True, split=SLICE + 7), dict(mem=1, keep=False)):
        nr.check_defining_property(emu_lib, m, N, kinds, None, T_PROP, k=k, held=[0] if held else [], more=SLICE + 3, **mode)


# ---- 6. moments through the measurement ---------------------------------------------------------------------------------------------
def test_moments_of_a_measured_uniform_row(emu_lib):
    from exact_ref import exact_moments, reported
    N, T = 4, 3 * SLICE + 5
    rng = np.random.default_rng(4)
    k = nr.noise("uniform", amp=np.logspace(-2, 1, N), offset=rng.standard_normal(N), seed=1)
    r = nr.apply_sources(runner(sr.wire_model(1, FS), N, emu_lib), [k])
    r.source_clock = 2 ** 40
    r.set_measurement(harmonics=0)
    u = r.render_sources(T)
    assert np.array_equal(u[:, :, 0], nr.uniform_row(k, 0, N, T, 2 ** 40))
    r.measure(T=T)
    out, count = sr.raw_measurement(r)
    assert count == T
    s, sq, mn, mx = exact_moments(u)
    mean, rms = reported((s, sq), count)
    for name, got, want in (("mean", out[:, :, 0], mean), ("rms", out[:, :, 1], rms), ("min", out[:, :, 2], mn), ("max", out[:, :, 3], mx)):
        assert np.array_equal(got, want), name


# ---- 7. statistics ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist,var", [("uniform", 1.0 / 3.0), ("gaussian", 1.0)])
@pytest.mark.parametrize("clock", [0, 2 ** 31 - 20, 2 ** 62])
def test_statistics_of_the_draws(emu_lib, monkeypatch, clock, dist, var):
    """deterministic (the streams are fixed): every standardised statistic of noise_ref.standardised_statistics within 4.0
    standard errors (the reference formulas' largest at these inputs: 2.98, the uniform mean at clock 2^31 - 20, pooled over
    the row; per instance 2.78 for the mean and 2.29 for the variance)"""
    monkeypatch.setenv("ACME_OS_SLICE", "4096")
    N, T = 8, 3 * 4096 + 1111
    r = runner(sr.wire_model(2, FS), N, emu_lib)
    r.set_source(0, "noise", dist=dist, stream=np.arange(N)).set_source(1, "noise", dist=dist, stream=np.arange(N))
    r.source_clock = clock
    u = r.render_sources(T)
    stats = nr.standardised_statistics(u[:, :, 0], u[:, :, 1], var)
    print(clock, dist, {k: round(v, 2) for k, v in stats.items()})
    for name, v in stats.items():
        assert v <= 4.0, (name, v)
    assert np.abs(u).max() < (1.0 if dist == "uniform" else 9.0)


# ---- 8. arguments -------------------------------------------------------------------------------------------------------------------
def test_argument_errors(emu_lib):
    L, N = emu_lib.L, 3
    r = runner(sr.wire_model(2, FS), N, emu_lib)
    d = lambda *v: (C.c_double * len(v))(*v)           # noqa: E731
    err = lambda: L.acme_last_error().decode()         # noqa: E731
    n = C.c_longlong(0)
    for row in (-1, 2, 64):
        assert L.acme_batch_set_source_noise(r.h, row, 0, 1, None, None, None) == INVALID and "row" in err(), row
    for dist in (-1, 2, 5):
        assert L.acme_batch_set_source_noise(r.h, 0, dist, 1, None, None, None) == INVALID and "dist" in err(), dist
    for hold in (0, -1, 2 ** 31, 2 ** 40):
        assert L.acme_batch_set_source_noise(r.h, 0, 1, hold, None, None, None) == INVALID and "hold" in err(), hold
    for bad in (np.nan, np.inf, -np.inf):
        assert L.acme_batch_set_source_noise(r.h, 0, 0, 1, None, d(1.0, bad, 1.0), None) == INVALID and "non-finite" in err()
        assert L.acme_batch_set_source_noise(r.h, 0, 0, 1, None, None, d(bad, 0.0, 0.0)) == INVALID and "non-finite" in err()
    assert L.acme_batch_get_source_clock(r.h, C.byref(n)) == INVALID                # (none of these armed anything)
    assert L.acme_batch_set_source_noise(r.h, 0, 1, 2 ** 31 - 1, None, None, None) == 0             # the largest hold; NULL streams: i
    assert L.acme_batch_set_source_noise(r.h, 1, 0, 1, None, None, None) == 0
    u = np.full((N, 6, 2), np.nan)
    assert L.acme_batch_render_sources(r.h, None, u.ctypes.data, 6, 0, None) == 0
    k = nr.noise("uniform", stream=[0, 1, 2])
    assert np.array_equal(u[:, :, 1], nr.uniform_row(k, 1, N, 6, 0))
    assert (u[:, :, 0] == u[:, :1, 0]).all()                                        # (held over the whole render)
    y = np.zeros((N, 6, 2))
    for fn in (L.acme_batch_run, L.acme_batch_run_async):                           # refused while a noise row is armed
        assert fn(r.h, u.ctypes.data, y.ctypes.data, 6, 0, None) == INVALID and "acme_batch_run_sources" in err()
    assert L.acme_batch_wait(r.h) == 0
    # Python: the keywords' own refusals
    with pytest.raises(ValueError, match="noise"):
        r.set_source(0, "nois")
    with pytest.raises(ValueError, match="distribution"):
        r.set_source(0, "noise", dist="cauchy")
    with pytest.raises(ValueError, match="seed"):
        r.set_source(0, "noise", seed=2 ** 31)
    with pytest.raises(Exception, match="streams"):
        r.set_source(0, "noise", stream=[1, 2])


def test_not_together_with_isolation(emu_lib):
    L = emu_lib.L
    r = runner(load("superover_var", HS), 2, emu_lib)
    r.set_isolation(20.0)
    assert L.acme_batch_set_source_noise(r.h, 0, 1, 1, None, None, None) == UNSUPPORTED
    assert "isolation" in L.acme_last_error().decode()
    r.set_isolation(0.0)
    assert L.acme_batch_set_source_noise(r.h, 0, 1, 1, None, None, None) == 0
    assert L.acme_batch_set_isolation(r.h, C.c_double(20.0)) == UNSUPPORTED


def test_replacing_and_clearing(emu_lib):
    """a noise row replaced by a sine and back renders what it rendered; clear_source restores the plain batch"""
    from acme_jl_amd.runner import AcmeError
    m, N, T = load("diodeclipper", HS), 3, SLICE + 6
    r = runner(m, N, emu_lib)
    r.set_source(0, "noise", amp=0.3, seed=4)
    first = r.render_sources(T)
    r.set_source(0, "sine", f_den=100, f_num=3)
    sine = r.render_sources(T)
    assert not np.array_equal(sine, first)
    sr.check_sine_row(sine[:, :, 0], dict(f_den=100, f_num=3), N, 0, [(i, t) for i in range(N) for t in range(T)])
    r.set_source(0, "noise", amp=0.3, seed=4)
    assert np.array_equal(r.render_sources(T), first)
    with pytest.raises(AcmeError, match="acme_batch_run_sources"):
        r.run(first, time_major=True)
    r.clear_source(0)
    y = r.run(first, time_major=True)
    never = runner(m, N, emu_lib)
    assert np.array_equal(y, never.run(first, time_major=True))
    for a, b in zip(r.get_state(), never.get_state()):
        assert np.array_equal(a, b)


def test_a_noise_row_lends_no_frequency(emu_lib):
    r = runner(sr.wire_model(1, FS), 2, emu_lib)
    r.set_source(0, "sine", f_den=100, f_num=3).set_source(0, "noise")
    with pytest.raises(ValueError, match="no sine source"):
        r.set_measurement(f0_from_source=0, harmonics=2)
    with pytest.raises(ValueError, match="no multisine or sine source"):
        r.set_measurement_bins([[1]], tones_from_source=0)
    r.set_measurement(harmonics=0)
    with pytest.raises(ValueError, match="no sine or multisine source"):
        r.set_measurement_fold(period_from_source=0)


# ---- 9. the sharded runner ----------------------------------------------------------------------------------------------------------
def test_multi_device_runner_forms_the_streams_over_the_global_index(emu_lib):
    from acme_jl_amd.runner import MultiDeviceRunner
    m, N, T = sr.wire_model(2, FS), 5, SLICE + 6
    amp = np.arange(1.0, N + 1)

    def arm(r):
        return r.set_source(0, "noise", amp=amp, seed=3).set_source(1, "noise", offset=amp, dist="uniform", hold=4, stream=np.arange(N) - 2)
    mr, one = arm(MultiDeviceRunner(m, N, devices=[0, 0], lib=emu_lib)), arm(runner(m, N, emu_lib))
    u = one.render_sources(T)
    assert np.array_equal(mr.render_sources(T), u)
    assert np.array_equal(u[:, :, 1], nr.uniform_row(nr.noise("uniform", hold=4, stream=np.arange(N) - 2, offset=amp), 1, N, T, 0))
    nr.check_gauss_row(u[:, :, 0], nr.noise("gaussian", amp=amp, seed=3), 0, N, 0, [(i, t) for i in range(N) for t in range(0, T, 5)])
    assert np.array_equal(mr.run_sources(T), one.run_sources(T)) and mr.source_clock == T
