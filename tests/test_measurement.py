"""Output measurements (acme_batch_set_measurement) on the CPU wave emulator: the accumulators against numpy applied to the
stored outputs in every kernel family and on decomposed models, their bit-identity across slices, split calls, host and
device memory, run / run_const / run_async and y stored or not, windows, oversampled batches, acme_batch_set_matrices,
argument errors and non-finite instances."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from helpers import FS, HS, load, sine
from measure_ref import assert_measured, np_measure


def runner(model, n, lib, **kw):
    from acme_jl_amd.runner import ModelRunner
    return ModelRunner(model, n, lib=lib, **kw)


def raw(r):
    """(out [N, nrows, 4 + 2H], count) straight from acme_batch_get_measurement"""
    from acme_jl_amd.runner import _dp
    H, rows = r._meas
    out = np.empty((r.n, len(rows), 4 + 2 * H))
    count = C.c_longlong(0)
    r.lib.check(r.lib.L.acme_batch_get_measurement(r.h, _dp(out), C.byref(count)))
    return out, count.value


def clipper():
    from acme_jl_amd import examples
    from acme_jl_amd.model import DiscreteModel
    return DiscreteModel(examples.diodeclipper(), Fraction(1, FS), HS)


def clipper_u(N, T, f=1000.0):
    return np.ascontiguousarray((np.logspace(-2, 0.7, N)[:, None] * sine(T, f=f)[None])[:, :, None])


def birdie_u(N, T):
    from helpers import sweep_inputs
    return np.ascontiguousarray(sweep_inputs("birdie_var", N, T).transpose(0, 2, 1))      # [N][T][2], vol in row 1


def cases():
    """(name, model, u [N, T, nu]): one model per kernel family, decomposed models among them"""
    import circuits
    from acme_jl_amd.model import DiscreteModel
    from test_oversampling import plumbing_cases
    out = [(name, m, u) for name, m, u, _ in plumbing_cases()]
    two = DiscreteModel(circuits.two_stage_clipper(), Fraction(1, FS), HS)
    out.append(("two-stage clipper (2 sub-problems)", two, clipper_u(3, 40)))
    return out


# ---- 1. numpy on the stored outputs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(5))
def test_measurement_matches_numpy_on_the_stored_outputs(emu_lib, case):
    name, m, u = cases()[case]
    N, T = u.shape[0], u.shape[1]
    f0, H = (3, 20), 5
    r = runner(m, N, emu_lib).set_measurement(f0=f0, harmonics=H)
    y = r.run(u, time_major=True)
    out, count = raw(r)
    assert count == T
    assert np.abs(y).max() > 1e-3, name
    assert_measured(out, np_measure(y, f0=f0, H=H)[0])
    # the Measurement object says the same
    mm = r.measurement()
    assert np.array_equal(mm.mean, out[:, :, 0]) and np.array_equal(mm.rms, out[:, :, 1])
    assert np.array_equal(mm.harmonics, out[:, :, 4::2] + 1j * out[:, :, 5::2])
    assert np.array_equal(mm.peak, np.maximum(np.abs(out[:, :, 2]), np.abs(out[:, :, 3])))
    a = np.abs(mm.harmonics)
    assert np.allclose(mm.thd(), np.sqrt((a[:, :, 1:] ** 2).sum(axis=2)) / a[:, :, 0], rtol=1e-14)


# ---- 2. bit-identity across every path ------------------------------------------------------------------------------------
def test_slices_calls_memory_entry_points_and_y_null_are_bit_identical(emu_lib, monkeypatch):
    from acme_jl_amd.runner import ModelRunner
    m = load("birdie_var", HS)
    N, T = 3, 60
    u = birdie_u(N, T)
    spec = dict(start=4, f0=Fraction(1000, FS), harmonics=4)

    def fresh():
        return runner(m, N, emu_lib).set_measurement(**spec)
    r = fresh()
    y = r.run(u, time_major=True)
    ref = raw(r)
    assert_measured(ref[0], np_measure(y, 4, 0, (10, 441), 4)[0])
    results = {}
    for sl in ("1", "7"):                                  # (7 does not divide T)
        monkeypatch.setenv("ACME_OS_SLICE", sl)
        rs = fresh()
        assert np.array_equal(rs.run(u, time_major=True), y)
        results[f"slice {sl}"] = raw(rs)
        results[f"slice {sl}, y NULL"] = raw(fresh().measure(u, time_major=True))
    monkeypatch.delenv("ACME_OS_SLICE")
    r2 = fresh()                                           # split calls
    r2.run(np.ascontiguousarray(u[:, :13]), time_major=True)
    r2.measure(np.ascontiguousarray(u[:, 13:]), time_major=True)
    results["split"] = raw(r2)
    rd = fresh()                                           # "device" memory (the emulator's device is host memory)
    yd = np.zeros_like(y)
    ModelRunner.run_device(rd, u.ctypes.data, yd.ctypes.data, T)
    assert np.array_equal(yd, y)
    results["device"] = raw(rd)
    rdn = fresh()
    ModelRunner.run_device(rdn, u.ctypes.data, 0, T)
    results["device, y NULL"] = raw(rdn)
    rc = fresh()                                           # run_const: row 1 (the volume) constant
    assert np.array_equal(rc.run_const(np.ascontiguousarray(u[:, :, :1]), np.ascontiguousarray(u[:, 0, :]), [1]), y)
    results["run_const"] = raw(rc)
    results["run_const, y NULL"] = raw(fresh().measure_const(np.ascontiguousarray(u[:, :, :1]), np.ascontiguousarray(u[:, 0, :]), [1]))
    results["y NULL"] = raw(fresh().measure(u, time_major=True))
    ra = fresh()                                           # run_async, with and without y
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


def test_measured_host_run_in_many_slices_reports_progress(emu_lib, monkeypatch):
    """a measured run from host arrays in 63 slices of 16 samples (ACME_OS_SLICE=16, T = 1 000), y stored and y = NULL: progress
    after every slice, outputs and accumulators those of the run in one slice"""
    m = load("birdie_var", HS)
    N, T = 3, 1000
    u = birdie_u(N, T)
    spec = dict(start=4, f0=Fraction(1000, FS), harmonics=4)
    got = {}
    for sl in ("4096", "16"):
        monkeypatch.setenv("ACME_OS_SLICE", sl)
        for keep in (True, False):
            seen = []
            r = runner(m, N, emu_lib, showprogress=lambda done, total: seen.append((done, total))).set_measurement(**spec)
            y = r.run(u, time_major=True) if keep else None
            if not keep:
                r.measure(u, time_major=True)
            got[sl, keep] = (y, raw(r))
            assert seen == ([(T, T)] if sl == "4096" else [(d, T) for d in list(range(16, T, 16)) + [T]]), (sl, keep)
    monkeypatch.delenv("ACME_OS_SLICE")
    assert np.array_equal(got["16", True][0], got["4096", True][0])
    for key, (_, (out, count)) in got.items():
        assert count == got["4096", True][1][1] and np.array_equal(out, got["4096", True][1][0]), key


# ---- 3. windows ------------------------------------------------------------------------------------------------------------
def test_windows_straddle_calls_and_slices_and_reset_restarts(emu_lib, monkeypatch):
    m = clipper()
    N, T = 3, 90
    u = clipper_u(N, T, f=2000.0)
    y = runner(m, N, emu_lib).run(u, time_major=True)
    monkeypatch.setenv("ACME_OS_SLICE", "7")
    for start, length in ((5, 23), (0, 1), (11, 0), (30, 200), (95, 10)):
        r = runner(m, N, emu_lib).set_measurement(start=start, length=length, f0=(2, 44), harmonics=3)
        for a, b in ((0, 10), (10, 41), (41, 90)):
            r.measure(np.ascontiguousarray(u[:, a:b]), time_major=True)
        out, count = raw(r)
        ref, n = np_measure(y, start, length, (2, 44), 3)
        assert count == n, (start, length)
        if n == 0:
            assert np.isnan(out[:, :, 0]).all()
            continue
        assert_measured(out, ref)
    # reset: the window's clock restarts with the next sample
    r = runner(m, N, emu_lib).set_measurement(start=3, length=30, f0=(2, 44), harmonics=3)
    r.measure(np.ascontiguousarray(u[:, :40]), time_major=True)
    r.reset_measurement()
    y2 = r.run(np.ascontiguousarray(u[:, 40:]), time_major=True)
    assert np.array_equal(y2, y[:, 40:])
    out, count = raw(r)
    assert count == 30
    assert_measured(out, np_measure(y2, 3, 30, (2, 44), 3)[0])


# ---- 4. oversampled batches: the base-rate outputs --------------------------------------------------------------------------
def test_oversampled_batch_measures_its_base_rate_outputs(emu_lib, monkeypatch):
    from test_oversampling import clipper_176k
    m = clipper_176k()
    N, T = 3, 70
    u = clipper_u(N, T, f=3000.0)
    r = runner(m, N, emu_lib).set_oversampling(4).set_measurement(start=6, f0=(1, 14), harmonics=6)
    y = r.run(u, time_major=True)
    out, count = raw(r)
    assert count == T - 6
    assert_measured(out, np_measure(y, 6, 0, (1, 14), 6)[0])
    monkeypatch.setenv("ACME_OS_SLICE", "9")
    rn = runner(m, N, emu_lib).set_oversampling(4).set_measurement(start=6, f0=(1, 14), harmonics=6)
    rn.measure(np.ascontiguousarray(u[:, :33]), time_major=True)
    rn.measure(np.ascontiguousarray(u[:, 33:]), time_major=True)
    assert np.array_equal(raw(rn)[0], out)


# ---- 5. acme_batch_set_matrices keeps the accumulators ----------------------------------------------------------------------
def test_set_matrices_keeps_the_accumulators_also_off_the_condensed_shape(emu_lib):
    from test_emu_parity import superover_models_with_their_own_diodes
    from helpers import sweep_inputs
    models = superover_models_with_their_own_diodes(3, HS)
    u = np.ascontiguousarray(sweep_inputs("superover_var", 3, 60, seed=2).transpose(0, 2, 1))
    r = runner(models[0], 3, emu_lib, models=[models[0]] * 3)
    assert r.batch_kernel_variant()[0] > 0
    r.set_measurement(start=10, f0=(1, 30), harmonics=3)
    ya = r.run(np.ascontiguousarray(u[:, :25]), time_major=True)
    r.set_models(1, [models[0]])                            # (the batch stays condensed)
    r.set_models(2, [models[2]])                            # ... and now moves to the plain shape
    assert r.batch_kernel_variant() == (0, "tuned")
    yb = r.run(np.ascontiguousarray(u[:, 25:]), time_major=True)
    out, count = raw(r)
    assert count == 50
    assert_measured(out, np_measure(np.concatenate([ya, yb], axis=1), 10, 0, (1, 30), 3)[0])
    # set_state, reset_report and set_oversampling leave them alone, too
    r.set_state(*r.get_state())
    r.reset_report()
    r.set_oversampling(1)
    assert np.array_equal(raw(r)[0], out)


# ---- 6. argument errors -------------------------------------------------------------------------------------------------------
def test_argument_errors(emu_lib):
    from acme_jl_amd.runner import ACME_MEM_HOST, AcmeError
    m = clipper()
    r = runner(m, 2, emu_lib)
    L = emu_lib.L

    def arm(**kw):
        s = dict(start=0, length=0, f_num=1, f_den=10, harmonics=2, rows=0)
        s.update(kw)
        return L.acme_batch_set_measurement(r.h, s["start"], s["length"], s["f_num"], s["f_den"], s["harmonics"], s["rows"])
    assert arm(harmonics=33) == -1 and "harmonics" in L.acme_last_error().decode()
    assert arm(f_den=0) == -1 and arm(f_den=-3) == -1 and arm(f_den=1 << 31) == -1
    assert arm(rows=0b10) == -1 and "row" in L.acme_last_error().decode()        # (the clipper has one output)
    assert arm(start=-1) == -1 and arm(length=-1) == -1
    with pytest.raises(AcmeError):
        r.measurement()                                     # (nothing armed)
    assert L.acme_batch_reset_measurement(r.h) == -1
    u = clipper_u(2, 20)
    # y = NULL without an armed measurement: still ACME_ERR_INVALID, on every entry point
    assert L.acme_batch_run(r.h, u.ctypes.data, None, 20, ACME_MEM_HOST, None) == -1
    assert "null u or y" in L.acme_last_error().decode()
    assert L.acme_batch_run_const(r.h, u.ctypes.data, u[:, 0].copy().ctypes.data, 0, None, 20, ACME_MEM_HOST, None) == -1
    assert L.acme_batch_run_async(r.h, u.ctypes.data, None, 20, ACME_MEM_HOST, None) == 0
    assert L.acme_batch_wait(r.h) == -1
    # isolation and measurement refuse each other
    r.set_isolation(2.0)
    assert arm() == -2
    r.set_isolation(0.0)
    assert arm() == 0
    with pytest.raises(AcmeError, match="measurement"):
        r.set_isolation(2.0)
    # off again: y = NULL is refused again
    r.clear_measurement()
    assert L.acme_batch_run(r.h, u.ctypes.data, None, 20, ACME_MEM_HOST, None) == -1
    with pytest.raises(ValueError):
        r.set_measurement(harmonics=3)                      # (no fundamental)


# ---- 7. non-finite instances ---------------------------------------------------------------------------------------------------
def test_a_non_finite_instance_measures_nan_only_itself(emu_lib):
    m = clipper()
    N, T = 3, 50
    u = clipper_u(N, T)
    u[1, 20, 0] = np.nan
    r = runner(m, N, emu_lib).set_measurement(f0=(1, 10), harmonics=2)
    y = r.run(u, time_major=True, check=False)
    assert r.report_arrays()["first_nonfinite"].tolist()[1] >= 0
    out, _ = raw(r)
    assert np.isnan(out[1]).all()
    keep = [0, 2]
    assert np.isfinite(out[keep]).all()
    assert_measured(out[keep], np_measure(y[keep], f0=(1, 10), H=2)[0])


# ---- 8. a row mask ------------------------------------------------------------------------------------------------------------
def two_output_clipper():
    """a diode clipper followed by an RC lowpass, probed at both nodes (ny = 2)"""
    from acme_jl_amd.circuit import capacitor, diode, resistor, voltageprobe, voltagesource
    from acme_jl_amd.examples import build
    from acme_jl_amd.model import DiscreteModel
    c = build([
        ("j_in", voltagesource(), {"-": "gnd"}),
        ("r1", resistor(1e3), {1: ("j_in", "+")}),
        ("c1", capacitor(47e-9), {1: ("r1", 2), 2: "gnd"}),
        ("d1", diode(is_=1e-15), {"-": "gnd", "+": ("r1", 2)}),
        ("d2", diode(is_=1.8e-15), {"-": ("r1", 2), "+": "gnd"}),
        ("r2", resistor(2.2e3), {1: ("r1", 2)}),
        ("c2", capacitor(22e-9), {1: ("r2", 2), 2: "gnd"}),
        ("p1", voltageprobe(), {"-": "gnd", "+": ("r1", 2)}),
        ("p2", voltageprobe(), {"-": "gnd", "+": ("r2", 2)}),
    ])
    return DiscreteModel(c, Fraction(1, FS), HS)


def test_a_row_mask_measures_the_rows_it_names(emu_lib):
    m = two_output_clipper()
    assert m.ny == 2
    N, T = 3, 60
    u = clipper_u(N, T)
    r_all = runner(m, N, emu_lib).set_measurement(f0=(1, 12), harmonics=3)
    y = r_all.run(u, time_major=True)
    out_all, _ = raw(r_all)
    assert_measured(out_all, np_measure(y, f0=(1, 12), H=3)[0])
    assert not np.array_equal(out_all[:, 0], out_all[:, 1])
    r1 = runner(m, N, emu_lib).set_measurement(f0=(1, 12), harmonics=3, rows=[1])
    r1.measure(u, time_major=True)
    out1, _ = raw(r1)
    assert out1.shape == (N, 1, 10) and r1.measurement().rows == (1,)
    assert np.array_equal(out1[:, 0], out_all[:, 1])
