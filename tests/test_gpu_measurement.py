"""Output measurements (acme_batch_set_measurement) on the MI355X: the accumulators against numpy applied to the GPU's own
stored outputs in every kernel family, their bit-identity across slices, split calls, host and device memory, run_const,
run_async and y stored or not, oversampled batches, parity with the CPU oracle, a physical check on the diode clipper (THD
against level, the fundamental's gain against the small-signal model) and a headline-shaped sweep without outputs."""
from fractions import Fraction

import numpy as np
import pytest

from helpers import FS, RTOL, load, oracle_run, sine, sweep_inputs
from measure_ref import assert_measured, np_measure
from test_measurement import birdie_u, cases, clipper, clipper_u, raw

pytestmark = pytest.mark.gpu

# The diode clipper's fundamental at 1 mV against linearize's transfer function at 1 kHz: 7.0e-14 relative on the CPU
# emulator (1 kHz coherent window of 4 410 samples after 882 of transient, f0 = 10/441); committed with a margin.
SMALL_SIGNAL_RTOL = 1e-11


def runner(model, n, **kw):
    from acme_jl_amd.runner import ModelRunner
    return ModelRunner(model, n, device=0, **kw)


@pytest.mark.parametrize("case", range(5))
def test_gpu_measurement_matches_numpy_on_the_stored_outputs(hip_lib, case):
    name, m, u = cases()[case]
    u = np.ascontiguousarray(np.tile(u, (1, 20, 1)))            # (longer: several tiles of the measurement kernel)
    f0, H = (3, 20), 5
    r = runner(m, u.shape[0]).set_measurement(start=7, f0=f0, harmonics=H)
    y = r.run(u, time_major=True)
    out, count = raw(r)
    assert count == u.shape[1] - 7
    assert np.abs(y).max() > 1e-3, name
    assert_measured(out, np_measure(y, 7, 0, f0, H)[0])


def test_gpu_memory_paths_slices_and_split_calls_are_bit_identical(hip_lib, monkeypatch):
    import torch
    m = load("birdie_var", "HomotopySolver{SimpleSolver}")
    N, T, t1 = 130, 9000, 4133                  # (three slices of 4 096 samples; the split falls inside one; 3 blocks of pairs)
    u = birdie_u(N, T)
    spec = dict(start=100, length=8000, f0=Fraction(1000, FS), harmonics=12)

    def fresh():
        return runner(m, N).set_measurement(**spec)
    r = fresh()
    y = r.run(u, time_major=True)
    ref = raw(r)
    assert ref[1] == 8000 and np.isfinite(y).all()
    assert_measured(ref[0], np_measure(y, 100, 8000, (10, 441), 12)[0])
    results = {"y NULL": raw(fresh().measure(u, time_major=True))}
    r = fresh()
    r.run(np.ascontiguousarray(u[:, :t1]), time_major=True)
    r.measure(np.ascontiguousarray(u[:, t1:]), time_major=True)
    results["split"] = raw(r)
    ud = torch.from_numpy(u).cuda()
    r = fresh()
    yd = r.run_torch(ud)
    torch.cuda.synchronize()
    assert np.array_equal(yd.cpu().numpy(), y)
    results["device"] = raw(r)
    r = fresh()
    r.run_device(ud.data_ptr(), 0, T, torch.cuda.current_stream().cuda_stream)
    results["device, y NULL"] = raw(r)
    uv, uc = np.ascontiguousarray(u[:, :, :1]), np.ascontiguousarray(u[:, 0, :])
    r = fresh()
    assert np.array_equal(r.run_const(uv, uc, [1]), y)
    results["run_const"] = raw(r)
    results["run_const, y NULL"] = raw(fresh().measure_const(uv, uc, [1]))
    r = fresh()
    r.run_async(u, None)
    r.wait()
    results["async, y NULL"] = raw(r)
    monkeypatch.setenv("ACME_OS_SLICE", "1000")
    results["slices of 1000"] = raw(fresh().measure(u, time_major=True))
    for k, (out, count) in results.items():
        assert count == ref[1], k
        assert np.array_equal(out, ref[0]), k


def test_gpu_oversampled_batch_measures_its_base_rate_outputs(hip_lib):
    from test_oversampling import clipper_176k
    N, T = 6, 5000
    u = clipper_u(N, T, f=3000.0)
    r = runner(clipper_176k(), N).set_oversampling(4).set_measurement(start=60, f0=(1, 14), harmonics=6)
    y = r.run(u, time_major=True)
    out, count = raw(r)
    assert count == T - 60
    assert_measured(out, np_measure(y, 60, 0, (1, 14), 6)[0])
    rn = runner(clipper_176k(), N).set_oversampling(4).set_measurement(start=60, f0=(1, 14), harmonics=6)
    rn.measure(u, time_major=True)
    assert np.array_equal(raw(rn)[0], out)


def test_gpu_measurement_matches_numpy_on_the_oracle_outputs(hip_lib):
    m = load("diodeclipper", "HomotopySolver{SimpleSolver}")
    N, T = 6, 1500
    u = sweep_inputs("diodeclipper", N, T)                      # [N, 1, T]
    r = runner(m, N).set_measurement(start=50, f0=(10, 441), harmonics=8)
    r.measure(u)
    out, count = raw(r)
    yref, _ = oracle_run(m, u)
    ref, n = np_measure(np.ascontiguousarray(yref.transpose(0, 2, 1)), 50, 0, (10, 441), 8)
    assert count == n
    scale = max(1.0, float(np.abs(yref).max()))
    assert np.abs(out - ref).max() <= 2 * RTOL * scale


def test_gpu_diode_clipper_distortion_and_small_signal_gain(hip_lib):
    from acme_jl_amd.analysis import linearize
    m = clipper()
    levels = np.array([1e-3, 0.03, 0.1, 0.2, 0.4, 0.8, 1.6, 3.2])
    S, L = 882, 4410                            # 20 ms of transient, then 100 periods of 1 kHz
    u = np.ascontiguousarray((levels[:, None] * sine(S + L)[None])[:, :, None])
    r = runner(m, len(levels)).set_measurement(start=S, length=L, f0=(10, 441), harmonics=10)
    r.measure(u, time_major=True)
    mm = r.measurement()
    assert mm.count == L
    thd = mm.thd()[:, 0]
    assert (np.diff(thd) > 0).all(), thd
    assert thd[-1] > 0.1 and thd[0] < 1e-9
    # the fundamental at 1 mV: u = a sin(w n) has A_1 = -j a over whole periods, so H = j A_1 / a
    lin = linearize(m, np.zeros(1))
    z = np.exp(2j * np.pi * 10 / 441)
    H = (lin.dy @ np.linalg.solve(z * np.eye(lin.nx) - lin.a, lin.b) + lin.ey)[0, 0]
    Hm = 1j * mm.harmonics[0, 0, 0] / levels[0]
    assert abs(Hm - H) / abs(H) <= SMALL_SIGNAL_RTOL, (Hm, H)


def test_gpu_headline_shaped_sweep_without_outputs(hip_lib):
    m = load("superover_var")
    N, T = 1024, FS // 4
    u = sweep_inputs("superover_var", N, T)                     # [N, 4, T]: the drive sine, three pots
    uv = np.ascontiguousarray(u[:, :1].transpose(0, 2, 1))
    uc = np.ascontiguousarray(u[:, :, 0])
    spec = dict(f0=(10, 441), harmonics=10)
    r = runner(m, N).set_measurement(**spec)
    y = r.run_const(uv, uc, [1, 2, 3])
    ref = raw(r)
    assert np.isfinite(y).all()
    assert_measured(ref[0], np_measure(y, 0, 0, (10, 441), 10)[0])
    rn = runner(m, N).set_measurement(**spec)
    rn.measure_const(uv, uc, [1, 2, 3])
    out, count = raw(rn)
    assert count == T
    assert np.array_equal(out, ref[0])
