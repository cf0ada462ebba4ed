"""The multisine source (acme_batch_set_source_multisine) and measurement bins (acme_batch_set_measurement_bins) on the CPU
wave emulator.

Source: one tone == the SINE row; 2, 3 and 4 tones against mpmath at phases reduced in unbounded integers; the defining
property (a source run is acme_batch_run on the rendered input, bit for bit) in every mode; argument errors; clear_source.
Bins: bin b of instance i == harmonic 1 of the shared measurement at k[b][i]; one tone with coefficients 1 ... B == the
per-instance form; the plan; invariance across slices, calls, memory, entry points, y stored or not, the table budget; reset,
re-arming, acme_batch_set_matrices; exact pins on the pass-through model; superposition on the linear fixtures."""
import ctypes as C

import numpy as np
import pytest

import exact_ref as X
import measure_pi_ref as PI
import multitone_ref as MT
import source_ref as sr
from helpers import FS, HS, load
from test_measurement import clipper, clipper_u, raw, two_output_clipper

SLICE = 24          # ACME_OS_SLICE of these tests: every run of more samples crosses slices
M31 = 2 ** 31 - 1


def runner(model, n, lib, **kw):
    from acme_jl_amd.runner import ModelRunner
    return ModelRunner(model, n, lib=lib, **kw)


@pytest.fixture(autouse=True)
def small_slices(monkeypatch):
    monkeypatch.setenv("ACME_OS_SLICE", str(SLICE))


# ---- source 1: one tone is the SINE row ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("clock", sr.CLOCKS)
def test_one_tone_is_the_sine_row(emu_lib, clock):
    """f_den = 2^31 - 1 with f_num near it, every store shape (nu = 1 ... 6: one and two elements per thread), odd lengths"""
    N = 5
    rng = np.random.default_rng(1)
    one = MT.awkward_tones(1, N, rng)
    sine = dict(one, kind="sine", f_num=one["f_num"][0], phase=one["phase"][0], amp=one["amp"][0])
    for nu in range(1, 7):
        row = (nu - 1) // 2                                # (the tone row's place: first and second element of a pair)
        for T in (SLICE + 5, 2 * SLICE):
            us = []
            for k in (one, sine):
                kinds = [dict(kind="const", offset=rng.standard_normal(N)) if c % 2 else None for c in range(nu)]
                kinds[row] = k
                r = sr.apply_sources(runner(sr.wire_model(nu, FS), N, emu_lib), kinds)
                r.source_clock = clock
                us.append(r.render_sources(T)[:, :, row])
            assert np.array_equal(us[0], us[1]), (nu, T)
            assert np.abs(us[0]).max() > 1e-3


# ---- source 2: the chain against mpmath ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("tones", [2, 3, 4])
@pytest.mark.parametrize("clock", sr.CLOCKS)
def test_tones_against_mpmath(emu_lib, clock, tones):
    N, T = 4, 2 * SLICE + 11
    rng = np.random.default_rng(tones)
    k = MT.awkward_tones(tones, N, rng)
    r = sr.apply_sources(runner(sr.wire_model(2, FS), N, emu_lib), [dict(kind="const", offset=1.0), k])
    r.source_clock = clock
    u = r.render_sources(T)
    worst = MT.check_multisine_row(u[:, :, 1], k, N, clock, [(i, t) for i in range(N) for t in range(T)])
    print(f"clock {clock}, {tones} tones: worst error {worst:.3f} of its bound")
    y = r.run_sources(T)
    assert np.array_equal(y, u) and r.source_clock == clock + T


def test_defaults_and_per_tone_scalars(emu_lib):
    """phase and amp NULL are 0 and 1; (tones,) values hold for every instance"""
    N, T = 3, SLICE + 3
    r = runner(sr.wire_model(1, FS), N, emu_lib)
    r.set_source(0, "multisine", f_den=96, f_num=[5, 7, 11])
    k = dict(f_den=96, f_num=np.array([5, 7, 11]))
    MT.check_multisine_row(r.render_sources(T)[:, :, 0], k, N, 0, [(i, t) for i in range(N) for t in range(T)])
    q = runner(sr.wire_model(1, FS), N, emu_lib)
    q.set_source(0, "multisine", f_den=96, f_num=np.array([[5] * N, [7] * N, [11] * N]), phase=[0, 0, 0], amp=np.ones((3, N)), offset=0.0)
    assert np.array_equal(q.render_sources(T), r.render_sources(T))


# ---- source 3: the defining property ------------------------------------------------------------------------------------------
def property_cases():
    N = 3
    tt = MT.two_tone(N, FS)
    pots = [dict(kind="const", offset=v) for v in ((np.arange(N) + 0.5) / N, np.full(N, 0.4), np.full(N, 0.7))]
    return [("diodeclipper", load("diodeclipper", HS), N, [tt]),
            ("superover_var", load("superover_var", HS), N, [dict(tt, offset=np.array([0.0, 0.01, -0.02]))] + pots)]


T_PROP = 2 * SLICE + 9
MODES = [dict(mem=0, keep=True), dict(mem=1, keep=True), dict(mem=0, keep=False), dict(mem=1, keep=False),
         dict(mem=0, keep=True, split=SLICE + 7), dict(mem=1, keep=False, split=SLICE + 7),
         dict(mem=0, keep=True, use_async=True), dict(mem=1, keep=False, use_async=True)]


@pytest.mark.parametrize("mode", range(len(MODES)))
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("case", range(2))
def test_a_multisine_run_is_a_run_on_the_rendered_input(emu_lib, case, k, mode):
    name, m, N, kinds = property_cases()[case]
    u = sr.check_defining_property(emu_lib, m, N, kinds, None, T_PROP, k=k, more=SLICE + 3, clock=2 ** 31 - 20, **MODES[mode])
    assert np.abs(u).max() > 1e-3 and np.isfinite(u).all()


# ---- source 4: validation and interplay ---------------------------------------------------------------------------------------
def test_source_argument_errors(emu_lib):
    L, N = emu_lib.L, 3
    r = runner(sr.wire_model(2, FS), N, emu_lib)
    d = lambda *v: (C.c_double * len(v))(*v)           # noqa: E731
    ll = lambda *v: (C.c_longlong * len(v))(*v)        # noqa: E731
    err = lambda: L.acme_last_error().decode()         # noqa: E731
    ok = ll(1, 2, 3, 4, 5, 6)
    for tones in (0, -1, 5):
        assert L.acme_batch_set_source_multisine(r.h, 0, 100, tones, ok, None, None, None) == -1 and "tones" in err()
    assert L.acme_batch_set_source_multisine(r.h, 0, 100, 2, None, None, None, None) == -1 and "f_num" in err()
    for f_den in (0, -5, 2 ** 31):
        assert L.acme_batch_set_source_multisine(r.h, 0, f_den, 2, ok, None, None, None) == -1
    assert L.acme_batch_set_source_multisine(r.h, 0, 100, 2, ll(1, 2, 3, 4, 100, 6), None, None, None) == -1
    assert "tone 1" in err() and "instance 1" in err()
    assert L.acme_batch_set_source_multisine(r.h, 0, 100, 2, ll(1, 2, -1, 4, 5, 6), None, None, None) == -1
    assert "tone 0" in err() and "instance 2" in err()
    assert L.acme_batch_set_source_multisine(r.h, 0, 100, 2, ok, ll(0, 0, 0, 100, 0, 0), None, None) == -1
    assert "tone 1" in err() and "instance 0" in err()
    for bad in (np.nan, np.inf, -np.inf):
        assert L.acme_batch_set_source_multisine(r.h, 0, 100, 2, ok, None, d(1, 1, 1, 1, 1, bad), None) == -1
        assert L.acme_batch_set_source_multisine(r.h, 0, 100, 2, ok, None, None, d(0, bad, 0)) == -1
    for row in (-1, 2, 64):
        assert L.acme_batch_set_source_multisine(r.h, row, 100, 2, ok, None, None, None) == -1
    n = C.c_longlong(0)
    assert L.acme_batch_get_source_clock(r.h, C.byref(n)) == -1           # (none of these armed anything)
    assert L.acme_batch_set_source_multisine(r.h, 0, 100, 2, ok, None, None, None) == 0
    with pytest.raises(ValueError):
        r.set_source(0, "multisine", f_den=100, f_num=[1, 2, 3, 4, 5])
    with pytest.raises(ValueError):
        r.set_source(0, "multisine", f_den=100)


def test_isolation_and_clear_source(emu_lib):
    L = emu_lib.L
    m = load("diodeclipper", HS)
    N, T = 3, 60
    r = runner(m, N, emu_lib)
    r.set_isolation(20.0)
    f = (C.c_longlong * 6)(1, 2, 3, 4, 5, 6)
    assert L.acme_batch_set_source_multisine(r.h, 0, 100, 2, f, None, None, None) == -2
    r.set_isolation(0.0)
    r.set_source(0, "multisine", **{k: v for k, v in MT.two_tone(N, FS).items() if k != "kind"})
    assert L.acme_batch_set_isolation(r.h, C.c_double(20.0)) == -2
    r.run_sources(30)
    before = r.render_sources(20)
    x, p, z = r.get_state()                                # the other calls leave the row and the clock alone
    r.set_state(x, p, z)
    r.reset_report()
    r.set_oversampling(2).set_oversampling(1)
    r.set_measurement(harmonics=0).reset_measurement().clear_measurement()
    assert r.source_clock == 30 and np.array_equal(r.render_sources(20), before)
    # clear_source: the row is the caller's again, the batch a plain one
    u = clipper_u(N, T)
    r.clear_source(0)
    r.set_state(*runner(m, N, emu_lib).get_state())
    assert np.array_equal(r.run(u, time_major=True), runner(m, N, emu_lib).run(u, time_major=True))
    assert L.acme_batch_set_isolation(r.h, C.c_double(20.0)) == 0


def test_multi_device_runner_slices_the_tones(emu_lib):
    from acme_jl_amd.runner import MultiDeviceRunner
    m, N, T = sr.wire_model(1, FS), 5, 40
    k = MT.awkward_tones(3, N, np.random.default_rng(0), f_den=441)
    coef = [[1, 0, 0], [0, 1, -1], [1, 1, 1]]
    mr = MultiDeviceRunner(m, N, devices=[0, 0], lib=emu_lib)
    one = runner(m, N, emu_lib)
    for r in (mr, one):
        r.set_source(0, "multisine", f_den=441, f_num=k["f_num"], phase=k["phase"], amp=k["amp"], offset=k["offset"])
        r.set_measurement_bins(coef, tones_from_source=0)
    assert np.array_equal(mr.render_sources(T), one.render_sources(T))
    mr.measure(T=T)
    one.measure(T=T)
    assert np.array_equal(mr.measurement().bins, one.measurement().bins)
    mr.set_measurement_bins(coef, f_den=441, f_num=k["f_num"])
    mr.measure(T=T)
    assert mr.measurement().bins.shape == (N, 1, 3)


# ---- bins 1: bin by bin against the shared measurement -----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MT.tone_cases()))
def test_each_bin_is_the_shared_measurement_at_its_frequency(emu_lib, name):
    f_num, kinds = MT.tone_cases()[name]
    # F = N: only bins of f2 - f1 (7 for every instance), so that 130 groups make four distinct bin frequencies
    coef = np.array([[-1, 1], [1, -1], [2, -2], [0, 0]]) if name == "F=N" else MT.COEF6
    got, kb = MT.check_bins_against_shared(lambda m, n: runner(m, n, emu_lib), clipper(), f_num, kinds, 441, 100,
                                           dict(start=3, length=90), coef)
    assert (kb > 441 // 2).any()                           # (a combination that wrapped below zero)
    assert np.abs(got[0][:, 0, 4:6]).max() > 1e-3


# ---- bins 2: one tone, coefficients 1 ... B, is the per-instance form ---------------------------------------------------------
@pytest.mark.parametrize("B", [0, 1, 10, 17, 32])
def test_one_tone_with_harmonic_coefficients_is_the_per_instance_form(emu_lib, B):
    # P = N nrows = 67, 70, 35 -- never a multiple of 64; a row mask
    for m, N, rows in ((clipper(), 67, None), (two_output_clipper(), 35, None), (two_output_clipper(), 35, [1])):
        u = clipper_u(N, 90)
        f_num = np.array([10, 20, 30])[np.arange(N) % 3]
        spec = dict(start=5, length=80, rows=rows)
        rp = runner(m, N, emu_lib).set_measurement(f_den=441, f_num=f_num, harmonics=B, **spec)
        y = rp.run(u, time_major=True)
        rb = runner(m, N, emu_lib).set_measurement_bins(1 + np.arange(B), f_den=441, f_num=f_num[None], **spec)
        assert np.array_equal(rb.run(u, time_major=True), y)
        (a, ca), (b, cb) = raw(rp), raw(rb)
        assert ca == cb == 80 and a.shape == b.shape == (N, len(rows) if rows else m.ny, 4 + 2 * B)
        assert np.array_equal(a, b), (B, N, rows, np.argwhere(a != b)[:8])
        pa, pb = rp.measurement_plan(), rb.measurement_plan()
        assert pa["groups"] == pb["groups"] == 3 and pa["chunk"] == pb["chunk"]
        assert np.array_equal(pa["perm"], pb["perm"]) and np.array_equal(pa["wave_group"], pb["wave_group"])


# ---- bins 3: invariance -------------------------------------------------------------------------------------------------------
def test_bins_are_bit_identical_across_every_path(emu_lib, monkeypatch):
    from acme_jl_amd.runner import ModelRunner
    m = clipper()
    N, T = 5, 150
    tt = MT.two_tone(N, 441, 19, 20)
    f_num = np.stack([[19, 19, 21, 19, 21], [20, 20, 20, 20, 20]])
    tt["f_num"] = f_num
    spec = dict(start=4, f_den=441, f_num=f_num)

    def fresh(sourced=False):
        r = runner(m, N, emu_lib)
        if sourced:
            sr.apply_sources(r, [tt])
        return r.set_measurement_bins(MT.COEF6, **spec)
    r = fresh(True)
    assert r.measurement_plan()["chunk"] == 4096 and r.measurement_plan()["groups"] == 2
    u = r.render_sources(T)
    y = r.run_sources(T)
    ref = raw(r)
    assert ref[1] == T - 4 and np.isfinite(ref[0]).all()
    results = {"sourced, y NULL": raw(fresh(True).measure(T=T))}
    for sl in ("7", "4096"):                               # ACME_OS_SLICE small against large (7 does not divide T)
        monkeypatch.setenv("ACME_OS_SLICE", sl)
        rs = fresh()
        assert np.array_equal(rs.run(u, time_major=True), y)
        results[f"slice {sl}"] = raw(rs)
        results[f"slice {sl}, y NULL"] = raw(fresh().measure(u, time_major=True))
    monkeypatch.setenv("ACME_OS_SLICE", str(SLICE))
    monkeypatch.setenv("ACME_MEAS_TABLE_BUDGET", "1")      # the table budget forced small: chunks of one tile
    rb = fresh()
    assert rb.measurement_plan()["chunk"] == 64
    results["one-tile chunks"] = raw(rb.measure(u, time_major=True))
    rb = fresh(True)                                       # ... and split source calls with the cut inside a chunk and a slice
    rb.run_sources(77)
    rb.measure(T=T - 77)
    results["one-tile chunks, split, sourced"] = raw(rb)
    monkeypatch.delenv("ACME_MEAS_TABLE_BUDGET")
    r2 = fresh()
    r2.run(np.ascontiguousarray(u[:, :77]), time_major=True)
    r2.measure(np.ascontiguousarray(u[:, 77:]), time_major=True)
    results["split"] = raw(r2)
    rd = fresh()                                           # "device" memory (the emulator's device is host memory)
    yd = np.zeros_like(y)
    ModelRunner.run_device(rd, u.ctypes.data, yd.ctypes.data, T)
    assert np.array_equal(yd, y)
    results["device"] = raw(rd)
    rdn = fresh()
    ModelRunner.run_device(rdn, u.ctypes.data, 0, T)
    results["device, y NULL"] = raw(rdn)
    ra = fresh()
    ya = np.zeros_like(y)
    ra.run_async(u, ya)
    ra.wait()
    assert np.array_equal(ya, y)
    results["async"] = raw(ra)
    rn = fresh(True)
    rn.run_sources_async(T)
    rn.wait()
    results["sources async, y NULL"] = raw(rn)
    for k, (out, count) in results.items():
        assert count == ref[1], k
        assert np.array_equal(out, ref[0]), k


# ---- bins 4: reset, re-arming, set_matrices -----------------------------------------------------------------------------------
def test_reset_rearming_and_set_matrices(emu_lib):
    from helpers import sweep_inputs
    from test_emu_parity import superover_models_with_their_own_diodes
    m = clipper()
    uc = clipper_u(3, 90, f=2000.0)
    f_num = np.array([[1, 2, 3], [5, 5, 4]])
    coef = np.array([[1, 0], [0, 1], [1, -1]])
    kb = MT.bin_frequencies(coef, f_num, 44)
    # reset: the clock restarts, the bins stay
    r = runner(m, 3, emu_lib).set_measurement_bins(coef, start=3, length=30, f_den=44, f_num=f_num)
    r.measure(np.ascontiguousarray(uc[:, :40]), time_major=True)
    r.reset_measurement()
    r.measure(np.ascontiguousarray(uc[:, 40:]), time_major=True)

    def shared():
        q = runner(m, 3, emu_lib)
        q.run(np.ascontiguousarray(uc[:, :40]), time_major=True)
        return q
    ref = MT.shared_by_bin(shared, lambda q: q.measure(np.ascontiguousarray(uc[:, 40:]), time_major=True), 44, kb, dict(start=3, length=30))
    assert raw(r)[1] == 30
    MT.assert_bin_by_bin(raw(r), kb, ref)
    # arming another form replaces the bins, and the bins replace it
    r.set_measurement(f0=(2, 44), harmonics=2)
    assert r.lib.L.acme_batch_get_measurement_plan(r.h, None, None, None, None) == -1
    r.set_measurement_bins(coef, f_den=44, f_num=f_num)
    assert r.measurement_plan()["groups"] == 3
    r.set_measurement(f_den=44, f_num=[1, 1, 2], harmonics=2)
    assert r.measurement_plan()["groups"] == 2 and raw(r)[0].shape == (3, 1, 8)
    r.set_state(*runner(m, 3, emu_lib).get_state())
    r.measure(uc, time_major=True)
    q = runner(m, 3, emu_lib).set_measurement(f_den=44, f_num=[1, 1, 2], harmonics=2)
    q.measure(uc, time_major=True)
    assert np.array_equal(raw(r)[0], raw(q)[0])
    # set_matrices rebuilds the batch: accumulators, clock, plan and bins go with it
    models = superover_models_with_their_own_diodes(3, HS)
    u = np.ascontiguousarray(sweep_inputs("superover_var", 3, 60, seed=2).transpose(0, 2, 1))
    kb = MT.bin_frequencies(coef, f_num, 30)

    def feed(r):
        r.run(np.ascontiguousarray(u[:, :25]), time_major=True)
        r.set_models(1, [models[0]])
        r.set_models(2, [models[2]])
        r.run(np.ascontiguousarray(u[:, 25:]), time_major=True)

    def batch():
        return runner(models[0], 3, emu_lib, models=[models[0]] * 3)
    r = batch().set_measurement_bins(coef, start=10, f_den=30, f_num=f_num)
    feed(r)
    assert raw(r)[1] == 50 and r.measurement_plan()["groups"] == 3
    MT.assert_bin_by_bin(raw(r), kb, MT.shared_by_bin(batch, feed, 30, kb, dict(start=10)))


def test_bins_argument_errors(emu_lib):
    from acme_jl_amd.runner import AcmeError
    r = runner(clipper(), 4, emu_lib)
    L = emu_lib.L
    err = lambda: L.acme_last_error().decode()         # noqa: E731

    def arm(f_num=(1, 2, 3, 4, 5, 6, 7, 8), f_den=10, tones=2, bins=2, coef=(1, 0, 0, 1), start=0, length=0, rows=0):
        p = None if f_num is None else (C.c_longlong * len(f_num))(*f_num)
        c = None if coef is None else (C.c_int * len(coef))(*coef)
        return L.acme_batch_set_measurement_bins(r.h, start, length, f_den, tones, p, bins, c, rows)
    assert arm(tones=0) == -1 and arm(tones=5) == -1 and "tones" in err()
    assert arm(bins=-1) == -1 and arm(bins=33) == -1 and "bins" in err()
    assert arm(f_num=None) == -1 and "f_num" in err()
    assert arm(coef=None) == -1 and "coef" in err()
    assert arm(f_num=(1, 2, 3, 4, 5, 6, 10, 8)) == -1 and "tone 1" in err() and "instance 2" in err()
    assert arm(f_num=(1, -2, 3, 4, 5, 6, 7, 8)) == -1 and "tone 0" in err() and "instance 1" in err()
    assert arm(coef=(1, 0, 0, 32768)) == -1 and "bin 1" in err()
    assert arm(f_den=0) == -1 and arm(f_den=1 << 31) == -1 and arm(rows=0b10) == -1 and arm(start=-1) == -1 and arm(length=-1) == -1
    assert L.acme_batch_get_measurement_plan(r.h, None, None, None, None) == -1     # (nothing was armed by any of these)
    r.set_isolation(2.0)
    assert arm() == -2
    r.set_isolation(0.0)
    assert arm(bins=0, coef=None) == 0 and arm() == 0
    with pytest.raises(AcmeError, match="measurement"):
        r.set_isolation(2.0)
    with pytest.raises(ValueError, match="source"):
        r.set_measurement_bins([[1]], tones_from_source=0)
    r.set_source(0, "sine", f_den=10, f_num=[1, 2, 3, 4])
    r.set_measurement_bins([[1], [2]], tones_from_source=0)         # (a SINE row: one tone)
    assert r.measurement_plan()["groups"] == 4


# ---- bins 5: exact pins on the pass-through model ----------------------------------------------------------------------------
def test_exact_moments_and_bins_on_the_pass_through_model(emu_lib, monkeypatch):
    """f_den = 2^31 - 1 with tones next to it and at 0; one-tile chunks: 165 = 2 x 64 + 37 samples are three chunks with a
    ragged last tile; row 3 of a 5-output model"""
    N, T = 6, 480
    f_num = np.array([[M31 - 1, 0, 1234567, M31 - 2, 5, 1], [M31 - 2, 0, 7654321, M31 - 1, 5, M31 - 1]])
    coef = np.array([[1, 0], [0, 1], [1, -1], [-3, 2], [32767, -32767], [1, 1]])
    kb = MT.bin_frequencies(coef, f_num, M31)
    assert (kb == 0).any()
    u = X.scaled_rows(np.random.default_rng(11), N, T, 5)
    m = X.wire_model(5, FS)
    monkeypatch.setenv("ACME_MEAS_TABLE_BUDGET", "1")
    for rows in ([3], None):
        r = runner(m, N, emu_lib).set_measurement_bins(coef, start=301, length=165, f_den=M31, f_num=f_num, rows=rows)
        assert r.measurement_plan()["chunk"] == 64
        assert np.array_equal(r.run(u, time_major=True), u)
        out, count = raw(r)
        seg = u[:, 301:466][:, :, rows if rows else list(range(5))]
        worst = MT.check_exact_bins(out, count, seg, M31, kb)
        print(f"bins on the pass-through model: worst |error| / bound {worst:.2e}")


# ---- bins 6: superposition on the linear fixtures ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rc_ladder", "sallenkey"])
def test_superposition_on_a_linear_model(emu_lib, name, monkeypatch):
    monkeypatch.setenv("ACME_OS_SLICE", "4096")
    m = load(name)
    assert m.nn() == 0 and (m.nu, m.ny) == (1, 1)
    pairs = np.array([[19000, 60, 440, 1000, 9000, 50], [20000, 7000, 550, 3001, 9100, 15000]])
    amps = np.array([[1.0, 0.8, 0.5, 2.0, 1.0, 0.1], [1.0, 0.2, 1.5, 0.25, 1.0, 3.0]])
    worst = MT.check_superposition(lambda mm, n: runner(mm, n, emu_lib), m, name, FS, pairs, amps)
    print(f"{name}: worst error {worst:.3e} of BODE_ATOL x the tones' amplitudes")
