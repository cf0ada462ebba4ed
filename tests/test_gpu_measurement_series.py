"""Measurement series (acme_batch_set_measurement_series) on the MI355X: acme_meas_series_kernel itself -- the walk over the
sub-ranges (window x tile), the slots' loads and stores, the broadcast loop of uniform waves and the 16-byte loads of mixed
waves -- which the CPU emulator only walks as plain loops.  Every window against the single-window form armed at
start + w hop, length win on an identical run, bit for bit (series_ref)."""
import numpy as np
import pytest

import measure_pi_ref as PI
import multitone_ref as MT
import series_ref as SR
from helpers import load
from series_ref import raw_series
from test_measurement import clipper, two_output_clipper
from test_measurement_per_instance import _freq_cases

pytestmark = pytest.mark.gpu


def mk(model, n, **kw):
    from acme_jl_amd.runner import ModelRunner
    return ModelRunner(model, n, device=0, **kw)


# ---- 1. boundary geometry ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("series", SR.GEOMETRY)
def test_gpu_boundary_geometry(hip_lib, series):
    SR.check_geometry(mk, clipper(), 131, 9000, 301, 10, series)


@pytest.mark.parametrize("H", [0, 1, 17, 32])
@pytest.mark.parametrize("series", [(441, 441, 25), (5, 7, 40)])
def test_gpu_boundary_geometry_over_the_harmonics(hip_lib, series, H):
    SR.check_geometry(mk, clipper(), 131, 9000, 301, H, series)


@pytest.mark.parametrize("rows", [[1], None])
def test_gpu_boundary_geometry_two_outputs(hip_lib, rows):
    SR.check_geometry(mk, two_output_clipper(), 99, 9000, 301, 10, (100, 257, 30), rows)


# ---- 2. forms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["F1", "F3-200-7-1", "F=N"])
def test_gpu_per_instance_windows(hip_lib, name):
    f_num, kinds = _freq_cases()[name]
    assert name != "F3-200-7-1" or kinds == (3, 1)
    SR.check_per_instance(mk, f_num, kinds, 4300)


@pytest.mark.parametrize("name", list(MT.tone_cases()))
def test_gpu_bins_windows(hip_lib, name):
    f_num, kinds = MT.tone_cases()[name]
    SR.check_bins(mk, f_num, kinds, 4300)


# ---- 3. paths -----------------------------------------------------------------------------------------------------------------
class TorchDevice:
    def put(self, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def run(self, r, u, keep, T):
        import torch
        if keep:                                            # run_torch: y a tensor of the library's making
            y = r.run_torch(u)
            torch.cuda.synchronize()
            return y.cpu().numpy()
        r.run_device(u.data_ptr(), 0, T, torch.cuda.current_stream().cuda_stream)
        return None


@pytest.mark.parametrize("k", [1, 3])
def test_gpu_paths_are_bit_identical(hip_lib, monkeypatch, k):
    SR.check_paths(mk, TorchDevice(), k, 9000, monkeypatch)


# ---- 4. exact pins ------------------------------------------------------------------------------------------------------------
def test_gpu_exact_moments_and_harmonics_per_window(hip_lib):
    worst = SR.check_exact(mk, N=77)
    print(f"series harmonics on the GPU: worst |error| / bound {worst:.2e}")


# ---- 5. use level -------------------------------------------------------------------------------------------------------------
def test_gpu_bode_plot_window_by_window(hip_lib):
    """sallenkey, one instance per frequency k / 441, three back-to-back windows of 441 samples from sample 0: windows 1 and
    2 start at or past BODE_START (172) and are the transfer function within BODE_ATOL; window 0 holds the transient"""
    m = load("sallenkey")
    f_den, f_num = 441, np.arange(1, 221)
    assert PI.BODE_START["sallenkey"] <= 441
    r = mk(m, len(f_num))
    r.set_source(0, "sine", f_den=f_den, f_num=f_num)
    r.set_measurement(start=0, harmonics=1, f0_from_source=0).set_measurement_series(441, 441, 3)
    r.measure(T=3 * 441)
    s = r.measurement_series()
    assert s.complete == 3 and s.starts.tolist() == [0, 441, 882]
    assert np.isfinite(s.harmonics[0]).all()
    for w in (1, 2):
        err = np.abs(s.harmonics[w][:, 0, 0] - PI.bode_expected(m, f_den, f_num, int(s.starts[w])))
        print(f"sallenkey window {w}: max |A_1 - expected| {err.max():.2e} at f_num {f_num[err.argmax()]}")
        assert err.max() <= PI.BODE_ATOL, (w, err.max(), f_num[err.argmax()])


# ---- 7. no-series invariance -------------------------------------------------------------------------------------------------
def test_gpu_a_batch_without_a_series_is_unchanged(hip_lib):
    SR.check_no_series_invariance(mk, 131, 9000)


def test_gpu_multi_device_runner_concatenates_the_shards(hip_lib):
    from acme_jl_amd.runner import MultiDeviceRunner
    from test_measurement import clipper_u
    m, N, T = clipper(), 70, 1000
    u = clipper_u(N, T)
    one = mk(m, N).set_measurement(start=3, f0=(10, 441), harmonics=4).set_measurement_series(100, 257, 5)
    one.measure(u, time_major=True)
    md = MultiDeviceRunner(m, N, devices=[0, 0]).set_measurement(start=3, f0=(10, 441), harmonics=4).set_measurement_series(100, 257, 5)
    md.measure(u)
    a, b = one.measurement_series(), md.measurement_series()
    assert a.counts.tolist() == b.counts.tolist() == [100, 100, 100, 100, 0]
    assert np.array_equal(a.harmonics, b.harmonics, equal_nan=True) and np.array_equal(a.rms, b.rms, equal_nan=True)
