"""Per-instance measurement fundamentals (acme_batch_set_measurement_per_instance) on the CPU wave emulator.

A. every f_num[i] = f reduces to acme_batch_set_measurement(f, f_den), bit for bit.
B. mixed f_num: instance i == the shared measurement at f_num[i] on an identical run; the plan read back through
   acme_batch_get_measurement_plan says which waves are uniform (one group: the broadcast loop) and which mixed (per-lane
   loads) -- the emulator walks the same plan slot by slot, the GPU file runs the two loops themselves:
     F = 1 (N = 130)                        3 uniform waves, none mixed
     F = 3, groups of 200 / 7 / 1           3 uniform waves (192 of the 200) and 1 mixed (8 + 7 + 1)
     F = N = 130                            3 mixed waves, none uniform
     frequency fastest / slowest (N = 200)  3 uniform waves and 1 mixed of the remainders (3 + 3 + 2), either way
C. invariance: slices, split calls, host / device memory, every entry point, y stored or not, oversampling, table budget.
D. exact pins on the pass-through model (exact_ref).   E. argument errors.   F. a Bode plot in one batch."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import exact_ref as X
import measure_pi_ref as PI
from helpers import FS, HS, load
from test_measurement import birdie_u, clipper, clipper_u, raw, two_output_clipper

M31 = 2 ** 31 - 1


def runner(model, n, lib, **kw):
    from acme_jl_amd.runner import ModelRunner
    return ModelRunner(model, n, lib=lib, **kw)


# ---- A. reduces to the shared measurement --------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [0, 1, 10, 17, 32])
def test_equal_frequencies_reduce_to_the_shared_measurement(emu_lib, H):
    # (model, N, rows): P = N nrows = 67, 70, 35 -- never a multiple of 64
    for m, N, rows in ((clipper(), 67, None), (two_output_clipper(), 35, None), (two_output_clipper(), 35, [1])):
        u = clipper_u(N, 90)
        spec = dict(start=5, length=80, harmonics=H, rows=rows)
        rs = runner(m, N, emu_lib).set_measurement(f0=(10, 441) if H else None, **spec)
        y = rs.run(u, time_major=True)
        rp = runner(m, N, emu_lib).set_measurement(f_den=441, f_num=10, **spec)
        assert np.array_equal(rp.run(u, time_major=True), y)
        (a, ca), (b, cb) = raw(rs), raw(rp)
        assert ca == cb == 80 and a.shape == b.shape
        assert np.array_equal(a, b), (H, N, rows, np.argwhere(a != b)[:8])
        assert PI.wave_kinds(rp)[1] == 0                   # (one group: every wave uniform)
        rn = runner(m, N, emu_lib).set_measurement(f_den=441, f_num=np.full(N, 10), **spec)
        rn.measure(u, time_major=True)
        assert np.array_equal(raw(rn)[0], a)


# ---- B. instance by instance ------------------------------------------------------------------------------------------------
def _freq_cases():
    rng = np.random.default_rng(3)
    three = np.array([5] * 200 + [7] * 7 + [11])[rng.permutation(208)]
    return {"F1": (np.full(130, 9), (3, 0)),
            "F3-200-7-1": (three, (3, 1)),
            "F=N": (1 + np.arange(130), (0, 3)),
            "fastest": (np.array([3, 14, 25])[np.arange(200) % 3], (3, 1)),
            "slowest": (np.array([3, 14, 25])[np.arange(200) * 3 // 200], (3, 1))}


@pytest.mark.parametrize("name", list(_freq_cases()))
def test_each_instance_is_the_shared_measurement_at_its_frequency(emu_lib, name):
    f_num, kinds = _freq_cases()[name]
    N, T, f_den = len(f_num), 150, 441
    u = X.scaled_rows(np.random.default_rng(N), N, T, 1)
    m = X.wire_model(1, FS)
    spec = dict(start=3, length=140, harmonics=3)
    one = runner(m, N, emu_lib)                                # (the wire model has no state: one batch, re-armed, reruns identically)
    assert np.array_equal(one.run(u, time_major=True), u)
    r = runner(m, N, emu_lib).set_measurement(f_den=f_den, f_num=f_num, **spec)
    assert PI.wave_kinds(r) == kinds, (name, PI.wave_kinds(r))
    assert r.measurement_plan()["groups"] == len(set(f_num.tolist()))
    r.measure(u, time_major=True)
    got = raw(r)
    if name == "F=N":
        # 130 shared runs of the whole batch take minutes on the emulator: the wire model is y = u (asserted above), so a
        # batch of instance i alone on u[i] is an identical run of it (the GPU file runs the whole batch per frequency)
        for i in range(N):
            q = runner(m, 1, emu_lib).set_measurement(f0=(int(f_num[i]), f_den), **spec)
            q.measure(np.ascontiguousarray(u[i:i + 1]), time_major=True)
            o, c = raw(q)
            assert c == got[1] and np.array_equal(o[0], got[0][i]), i
        return
    ref = PI.shared_by_frequency(lambda: one, lambda q: q.measure(u, time_major=True), f_den, f_num, spec)
    PI.assert_instance_by_instance(got, f_num, ref)


def test_each_instance_on_a_nonlinear_two_output_model(emu_lib):
    m = two_output_clipper()
    N, T, f_den = 70, 100, 441                                 # P = 140: groups of 2 x 33, 2 x 30, 2 x 7 pairs
    f_num = np.array([10] * 33 + [20] * 30 + [30] * 7)[np.random.default_rng(4).permutation(N)]
    u = clipper_u(N, T)
    spec = dict(start=7, harmonics=4)
    r = runner(m, N, emu_lib).set_measurement(f_den=f_den, f_num=f_num, **spec)
    # 66 pairs -> one whole wave of group 0; the remainders 2 + 60 + 14 = 76: a mixed wave (2 + 60 + 2) and 12 of group 2 alone
    assert PI.wave_kinds(r) == (2, 1)
    r.measure(u, time_major=True)
    ref = PI.shared_by_frequency(lambda: runner(m, N, emu_lib), lambda q: q.measure(u, time_major=True), f_den, f_num, spec)
    PI.assert_instance_by_instance(raw(r), f_num, ref)


# ---- C. invariance ----------------------------------------------------------------------------------------------------------
def test_slices_calls_memory_entry_points_budget_and_y_null_are_bit_identical(emu_lib, monkeypatch):
    from acme_jl_amd.runner import ModelRunner
    m = load("birdie_var", HS)
    N, T = 3, 150
    u = birdie_u(N, T)
    f_den, f_num = 441, np.array([10, 20, 10])
    spec = dict(start=4, f_den=f_den, f_num=f_num, harmonics=4)

    def fresh():
        return runner(m, N, emu_lib).set_measurement(**spec)
    r = fresh()
    assert r.measurement_plan()["chunk"] == 4096
    y = r.run(u, time_major=True)
    ref = raw(r)
    shared = PI.shared_by_frequency(lambda: runner(m, N, emu_lib), lambda q: q.measure(u, time_major=True), f_den, f_num,
                                    dict(start=4, harmonics=4))
    PI.assert_instance_by_instance(ref, f_num, shared)
    results = {}
    for sl in ("7", "4096"):                               # ACME_OS_SLICE small against large (7 does not divide T)
        monkeypatch.setenv("ACME_OS_SLICE", sl)
        rs = fresh()
        assert np.array_equal(rs.run(u, time_major=True), y)
        results[f"slice {sl}"] = raw(rs)
        results[f"slice {sl}, y NULL"] = raw(fresh().measure(u, time_major=True))
    monkeypatch.delenv("ACME_OS_SLICE")
    monkeypatch.setenv("ACME_MEAS_TABLE_BUDGET", "1")      # the table budget forced small: chunks of one tile
    rb = fresh()
    assert rb.measurement_plan()["chunk"] == 64
    results["one-tile chunks"] = raw(rb.measure(u, time_major=True))
    rb = fresh()                                           # ... and split calls with the cut inside a chunk
    rb.run(np.ascontiguousarray(u[:, :77]), time_major=True)
    rb.measure(np.ascontiguousarray(u[:, 77:]), time_major=True)
    results["one-tile chunks, split"] = raw(rb)
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
    uv, uc = np.ascontiguousarray(u[:, :, :1]), np.ascontiguousarray(u[:, 0, :])
    rc = fresh()
    assert np.array_equal(rc.run_const(uv, uc, [1]), y)
    results["run_const"] = raw(rc)
    results["run_const, y NULL"] = raw(fresh().measure_const(uv, uc, [1]))
    ra = fresh()
    ya = np.zeros_like(y)
    ra.run_async(u, ya)
    ra.wait()
    assert np.array_equal(ya, y)
    results["async"] = raw(ra)
    rn = fresh()
    rn.run_async(u, None)
    rn.wait()
    results["async, y NULL"] = raw(rn)
    for k, (out, count) in results.items():
        assert count == ref[1], k
        assert np.array_equal(out, ref[0]), k


def test_run_sources_and_f0_from_source(emu_lib, monkeypatch):
    m = load("birdie_var", HS)
    N, T, f_den = 3, 100, 441
    f_num = np.array([10, 20, 30])

    def fresh():
        r = runner(m, N, emu_lib)
        r.set_source(0, "sine", amp=np.array([0.1, 0.5, 1.0]), f_den=f_den, f_num=f_num)
        r.set_source(1, "const", offset=np.array([0.3, 0.6, 0.9]))
        return r.set_measurement(start=6, harmonics=3, f0_from_source=0)
    r = fresh()
    u = r.render_sources(T)
    y = r.run_sources(T)
    ref = raw(r)
    monkeypatch.setenv("ACME_OS_SLICE", "9")
    assert np.array_equal(raw(fresh().measure(T=T))[0], ref[0])
    monkeypatch.delenv("ACME_OS_SLICE")
    rr = runner(m, N, emu_lib).set_measurement(start=6, harmonics=3, f_den=f_den, f_num=f_num)
    assert np.array_equal(rr.run(u, time_major=True), y)
    assert np.array_equal(raw(rr)[0], ref[0])
    # the fundamental of a driven instance carries its drive: A_1 is far above the harmonics' floor
    assert (np.abs(r.measurement().harmonics[:, 0, 0]) > 1e-3).all()


@pytest.mark.parametrize("k", [1, 3])
def test_oversampled_batches_are_invariant_too(emu_lib, monkeypatch, k):
    from acme_jl_amd import examples
    from acme_jl_amd.model import DiscreteModel
    m = DiscreteModel(examples.diodeclipper(), Fraction(1, k * FS), HS)
    N, T = 5, 150
    u = clipper_u(N, T, f=3000.0)
    f_num = np.array([3, 1, 3, 2, 1])
    spec = dict(start=6, f_den=14, f_num=f_num, harmonics=5)

    def fresh():
        return runner(m, N, emu_lib).set_oversampling(k).set_measurement(**spec)
    r = fresh()
    y = r.run(u, time_major=True)
    ref = raw(r)
    shared = PI.shared_by_frequency(lambda: runner(m, N, emu_lib).set_oversampling(k), lambda q: q.measure(u, time_major=True),
                                    14, f_num, dict(start=6, harmonics=5))
    PI.assert_instance_by_instance(ref, f_num, shared)
    monkeypatch.setenv("ACME_OS_SLICE", "9")
    monkeypatch.setenv("ACME_MEAS_TABLE_BUDGET", "1")
    rn = fresh()
    assert np.array_equal(rn.run(np.ascontiguousarray(u[:, :70]), time_major=True), y[:, :70])
    rn.measure(np.ascontiguousarray(u[:, 70:]), time_major=True)
    assert raw(rn)[1] == ref[1] and np.array_equal(raw(rn)[0], ref[0])


def test_reset_keeps_the_frequencies_and_set_matrices_keeps_everything(emu_lib):
    from test_emu_parity import superover_models_with_their_own_diodes
    from helpers import sweep_inputs
    models = superover_models_with_their_own_diodes(3, HS)
    u = np.ascontiguousarray(sweep_inputs("superover_var", 3, 60, seed=2).transpose(0, 2, 1))
    f_num = np.array([1, 2, 3])
    spec = dict(start=10, harmonics=3)

    def feed(r):
        """the run below: 25 samples, two rebuilds of the batch (the second leaves the condensed shape), 35 samples"""
        r.run(np.ascontiguousarray(u[:, :25]), time_major=True)
        r.set_models(1, [models[0]])
        r.set_models(2, [models[2]])
        assert r.batch_kernel_variant() == (0, "tuned")
        r.run(np.ascontiguousarray(u[:, 25:]), time_major=True)

    def fresh():
        return runner(models[0], 3, emu_lib, models=[models[0]] * 3)
    r = fresh().set_measurement(f_den=30, f_num=f_num, **spec)
    assert r.batch_kernel_variant()[0] > 0
    feed(r)
    got = raw(r)
    assert got[1] == 50
    PI.assert_instance_by_instance(got, f_num, PI.shared_by_frequency(fresh, feed, 30, f_num, spec))
    assert r.measurement_plan()["groups"] == 3             # (the plan went with the accumulators)
    # reset: the clock restarts, the frequencies stay
    m = clipper()
    uc = clipper_u(3, 90, f=2000.0)
    r = runner(m, 3, emu_lib).set_measurement(start=3, length=30, f_den=44, f_num=f_num, harmonics=3)
    r.measure(np.ascontiguousarray(uc[:, :40]), time_major=True)
    r.reset_measurement()
    r.measure(np.ascontiguousarray(uc[:, 40:]), time_major=True)

    def shared():
        q = runner(m, 3, emu_lib)
        q.run(np.ascontiguousarray(uc[:, :40]), time_major=True)
        return q
    ref = PI.shared_by_frequency(shared, lambda q: q.measure(np.ascontiguousarray(uc[:, 40:]), time_major=True), 44, f_num,
                                 dict(start=3, length=30, harmonics=3))
    assert raw(r)[1] == 30
    PI.assert_instance_by_instance(raw(r), f_num, ref)


def test_arming_either_form_replaces_the_other(emu_lib):
    m = clipper()
    u = clipper_u(3, 50)
    r = runner(m, 3, emu_lib).set_measurement(f_den=44, f_num=[1, 2, 3], harmonics=2)
    r.set_measurement(f0=(2, 44), harmonics=2)
    assert r.lib.L.acme_batch_get_measurement_plan(r.h, None, None, None, None) == -1
    r.measure(u, time_major=True)
    q = runner(m, 3, emu_lib).set_measurement(f0=(2, 44), harmonics=2)
    q.measure(u, time_major=True)
    assert np.array_equal(raw(r)[0], raw(q)[0])
    q.set_measurement(f_den=44, f_num=2, harmonics=2)          # ... and back: a fresh clock, fresh accumulators
    q.set_state(*runner(m, 3, emu_lib).get_state())
    q.measure(u, time_major=True)
    assert np.array_equal(raw(r)[0], raw(q)[0])


# ---- D. exact pins on the pass-through model ---------------------------------------------------------------------------------
def test_exact_moments_and_harmonics_per_instance(emu_lib, monkeypatch):
    """f_den = 2^31 - 1 with f_num next to it and 0; one-tile chunks: the window of 165 = 2 x 64 + 37 samples is three chunks
    with a ragged last tile; row 3 of a 5-output model (a strided row).  (A window beyond 2^20 samples: the GPU file.)"""
    N, T, H = 6, 480, 3
    f_num = np.array([M31 - 1, 0, 1234567, M31 - 2, 0, 1])
    u = X.scaled_rows(np.random.default_rng(11), N, T, 5)
    m = X.wire_model(5, FS)
    monkeypatch.setenv("ACME_MEAS_TABLE_BUDGET", "1")
    for rows in ([3], None):
        r = runner(m, N, emu_lib).set_measurement(start=301, length=165, f_den=M31, f_num=f_num, harmonics=H, rows=rows)
        assert r.measurement_plan()["chunk"] == 64
        assert np.array_equal(r.run(u, time_major=True), u)
        out, count = raw(r)
        seg = u[:, 301:466][:, :, rows if rows else list(range(5))]
        PI.check_exact_per_instance(out, count, seg, M31, np.repeat(f_num, 1), H)


# ---- E. argument errors -------------------------------------------------------------------------------------------------------
def test_argument_errors(emu_lib):
    from acme_jl_amd.runner import AcmeError
    m = clipper()
    r = runner(m, 4, emu_lib)
    L = emu_lib.L

    def arm(f_num=(1, 2, 3, 4), f_den=10, start=0, length=0, harmonics=2, rows=0):
        p = None if f_num is None else (C.c_longlong * 4)(*f_num)
        return L.acme_batch_set_measurement_per_instance(r.h, start, length, f_den, p, harmonics, rows)
    assert arm(f_num=(1, 2, 10, 11)) == -1 and "instance 2" in L.acme_last_error().decode()
    assert arm(f_num=(1, -1, 3, 4)) == -1 and "instance 1" in L.acme_last_error().decode()
    assert arm(f_num=None) == -1 and "f_num" in L.acme_last_error().decode()
    assert arm(f_den=0) == -1 and arm(f_den=-3) == -1 and arm(f_den=1 << 31) == -1
    assert arm(harmonics=33) == -1 and arm(rows=0b10) == -1 and arm(start=-1) == -1 and arm(length=-1) == -1
    assert L.acme_batch_get_measurement_plan(r.h, None, None, None, None) == -1     # (nothing was armed by any of these)
    r.set_isolation(2.0)                                    # isolation either way round
    assert arm() == -2
    r.set_isolation(0.0)
    assert arm() == 0
    with pytest.raises(AcmeError, match="measurement"):
        r.set_isolation(2.0)
    with pytest.raises(ValueError, match="exclude"):
        r.set_measurement(f0=(1, 10), f_den=10, f_num=[1, 2, 3, 4], harmonics=1)
    with pytest.raises(ValueError):
        r.set_measurement(f_num=[1, 2, 3, 4], harmonics=1)      # (no f_den)
    with pytest.raises(AcmeError, match="instance 3"):
        r.set_measurement(f_den=10, f_num=[1, 2, 3, 10], harmonics=1)
    with pytest.raises(ValueError, match="sine source"):
        r.set_measurement(harmonics=1, f0_from_source=0)        # (no source on row 0)
    r.set_source(0, "const", offset=0.5)
    with pytest.raises(ValueError, match="sine source"):
        r.set_measurement(harmonics=1, f0_from_source=0)        # (a source, but no sine)


def test_multi_device_runner_slices_the_frequencies(emu_lib):
    from acme_jl_amd.runner import MultiDeviceRunner
    m = clipper()
    N, T = 7, 60
    u = clipper_u(N, T)
    f_num = np.array([1, 2, 3, 1, 2, 3, 5])
    md = MultiDeviceRunner(m, N, devices=[0, 0, 0], lib=emu_lib).set_measurement(f_den=44, f_num=f_num, harmonics=2)
    md.measure(u)
    one = runner(m, N, emu_lib).set_measurement(f_den=44, f_num=f_num, harmonics=2)
    one.measure(u, time_major=True)
    assert np.array_equal(md.measurement().harmonics, one.measurement().harmonics)


# ---- F. a Bode plot in one batch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rc_ladder", "sallenkey"])
def test_bode_plot_in_one_batch_against_the_transfer_function(emu_lib, name):
    """24 frequencies 20 Hz ... 20 kHz, one instance each; |A_1 - expected| <= 1e-12 absolute (unit amplitude).  A plain numpy
    float64 simulation of the same recurrence deviates by 8.2e-15 (rc_ladder, 20 Hz) and <= 2.3e-16 (sallenkey)."""
    m = load(name)
    assert m.nn() == 0 and (m.nu, m.ny) == (1, 1)
    f_den, S = FS, PI.BODE_START[name]
    f_num = np.unique(np.round(np.logspace(np.log10(20), np.log10(20000), 24)).astype(np.int64))
    assert len(f_num) == 24
    a1 = PI.bode_measured(runner(m, 24, emu_lib), f_den, f_num, S)
    err = np.abs(a1 - PI.bode_expected(m, f_den, f_num, S))
    print(f"{name}: max |A_1 - expected| {err.max():.2e} at {f_num[err.argmax()]} Hz")
    assert err.max() <= PI.BODE_ATOL, (err.max(), f_num[err.argmax()])
