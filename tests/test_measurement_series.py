"""Measurement series (acme_batch_set_measurement_series) on the CPU wave emulator: W windows of win samples, one every hop,
accumulated in one pass -- every window against the single-window form armed at start + w hop, length win on an identical run,
bit for bit (series_ref).

1. boundary geometry    2. the three forms    3. paths (what the emulator has)    4. exact pins on the pass-through model
6. argument errors      7. a batch without a series is what it was              8. the MeasurementSeries object

The series, start and T are those of the GPU file.  The instance counts are not: an emulated run of the diode clipper at
N = 131, T = 9000 takes 14 s and every compared window needs one, so the geometry runs at N = 3 (two outputs: N = 2) -- the
emulator walks the pairs one by one, a block of 64 pairs does not exist here -- with every reference run ended behind its
window; the forms, whose N the frequency cases fix at 130 and 208, run the pass-through model over T = 460 (one whole window
of 441, one partial, the rest unreached; the series of 5 every 7 whole), every reference window fed its own samples; the two
output rows run (5, 7, 40) over T = 1000; the paths run N = 6 over T = 2100.
test_gpu_measurement_series.py runs the full shapes."""
import ctypes as C

import numpy as np
import pytest

import multitone_ref as MT
import series_ref as SR
from series_ref import raw_series
from test_measurement import clipper, clipper_u, two_output_clipper
from test_measurement_per_instance import _freq_cases


def mk_for(lib):
    def mk(model, n, **kw):
        from acme_jl_amd.runner import ModelRunner
        return ModelRunner(model, n, lib=lib, **kw)
    return mk


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("series", SR.GEOMETRY)
def test_boundary_geometry(emu_lib, series):
    SR.check_geometry(mk_for(emu_lib), clipper(), 3, 9000, 301, 10, series, cut=True)


@pytest.mark.parametrize("H", [0, 1, 17, 32])
@pytest.mark.parametrize("series", [(441, 441, 25), (5, 7, 40)])
def test_boundary_geometry_over_the_harmonics(emu_lib, series, H):
    SR.check_geometry(mk_for(emu_lib), clipper(), 3, 9000, 301, H, series, cut=True)


@pytest.mark.parametrize("rows", [[1], None])
def test_boundary_geometry_two_outputs(emu_lib, rows):
    SR.check_geometry(mk_for(emu_lib), two_output_clipper(), 2, 1000, 301, 10, (5, 7, 40), rows, cut=True)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["F1", "F3-200-7-1", "F=N"])
def test_per_instance_windows(emu_lib, name):
    f_num, kinds = _freq_cases()[name]
    SR.check_per_instance(mk_for(emu_lib), f_num, kinds, 460, wire=True)


@pytest.mark.parametrize("name", list(MT.tone_cases()))
def test_bins_windows(emu_lib, name):
    f_num, kinds = MT.tone_cases()[name]
    SR.check_bins(mk_for(emu_lib), f_num, kinds, 460, wire=True)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
class HostDevice:
    """the emulator's "device memory" is host memory"""

    def put(self, a):
        return np.ascontiguousarray(a)

    def run(self, r, u, keep, T):
        from acme_jl_amd.runner import ModelRunner
        y = np.zeros((r.n, T, r.model.ny)) if keep else None
        ModelRunner.run_device(r, u.ctypes.data, y.ctypes.data if keep else 0, T)
        return y


@pytest.mark.parametrize("k", [1, 3])
def test_paths_are_bit_identical(emu_lib, monkeypatch, k):
    SR.check_paths(mk_for(emu_lib), HostDevice(), k, 2100, monkeypatch, N=6)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_exact_moments_and_harmonics_per_window(emu_lib):
    worst = SR.check_exact(mk_for(emu_lib))
    print(f"series harmonics on the emulator: worst |error| / bound {worst:.2e}")


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(emu_lib):
    from acme_jl_amd.runner import AcmeError
    mk = mk_for(emu_lib)
    L = emu_lib.L
    m, u = clipper(), clipper_u(2, 10)

    def refused(r, what, *args):
        rc = L.acme_batch_set_measurement_series(r.h, *args)
        msg = L.acme_last_error().decode()
        assert rc == -1 and what in msg, (args, rc, msg)
    r = mk(m, 2)
    refused(r, "no measurement is armed", 4, 4, 2)
    with pytest.raises(AcmeError, match="no measurement is armed"):
        r.set_measurement_series(4)
    refused(r.set_measurement(start=1, length=5), "length", 4, 4, 2)
    r.set_measurement(start=1).measure(u, time_major=True)
    refused(r, "samples have been fed", 4, 4, 2)
    r.reset_measurement()
    refused(r, "win", 0, 4, 2)
    refused(r, "win", -3, 4, 2)
    refused(r, "hop", 5, 4, 2)
    refused(r, "windows", 4, 4, 0)
    refused(r, "windows", 4, 4, 2 ** 20 + 1)
    refused(r, "overflows", 4, 2 ** 62, 4)
    refused(r, "overflows", 2 ** 63 - 1, 2 ** 63 - 1, 1)
    out, cnt = np.zeros(64), C.c_longlong(0)
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_longlong)
    assert L.acme_batch_get_measurement_series(r.h, 0, 1, out.ctypes.data_as(dp), C.byref(cnt)) == -1       # no series yet
    assert "no measurement series" in L.acme_last_error().decode()
    with pytest.raises(AcmeError, match="no measurement series"):
        r.measurement_series()
    r.set_measurement_series(4, 4, 2)                       # (after the reset: accepted)
    assert L.acme_batch_get_measurement(r.h, out.ctypes.data_as(dp), C.byref(cnt)) == -1
    assert "acme_batch_get_measurement_series" in L.acme_last_error().decode()
    with pytest.raises(AcmeError):
        r.measurement()
    for first, n in ((0, 3), (2, 1), (3, 0), (-1, 1), (0, -1)):
        assert L.acme_batch_get_measurement_series(r.h, first, n, out.ctypes.data_as(dp), None) == -1, (first, n)
        assert "first" in L.acme_last_error().decode()
    assert L.acme_batch_get_measurement_series(r.h, 2, 0, None, None) == 0
    counts = np.full(2, -1, dtype=np.int64)                 # either pointer may be NULL
    assert L.acme_batch_get_measurement_series(r.h, 0, 2, None, counts.ctypes.data_as(lp)) == 0 and not counts.any()
    assert L.acme_batch_get_measurement_series(r.h, 1, 1, out.ctypes.data_as(dp), None) == 0
    assert np.isnan(out[0]) and out[2] == np.inf and out[3] == -np.inf      # a window never reached
    r.clear_measurement()
    with pytest.raises(AcmeError):
        r.measurement_series()
    # the largest series is accepted where its accumulators fit: one instance, no harmonics
    big = mk(m, 1).set_measurement().set_measurement_series(1, 1, 2 ** 20)
    big.measure(clipper_u(1, 10), time_major=True)
    assert big.measurement_series(0, 12).counts.tolist() == [1] * 10 + [0, 0]


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def test_a_batch_without_a_series_is_unchanged(emu_lib):
    SR.check_no_series_invariance(mk_for(emu_lib), 67, 300)


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
def test_measurement_series_object(emu_lib):
    mk = mk_for(emu_lib)
    m, N, T = two_output_clipper(), 5, 200
    u = clipper_u(N, T)
    r = mk(m, N).set_measurement(start=7, f0=(10, 441), harmonics=3).set_measurement_series(50, windows=5)
    r.measure(u, time_major=True)
    out, counts = raw_series(r)
    s = r.measurement_series()
    assert len(s) == 5 and s.counts.tolist() == counts.tolist() == [50, 50, 50, 43, 0] and s.complete == 3
    assert s.starts.tolist() == [7, 57, 107, 157, 207] and (s.win, s.hop) == (50, 50)
    assert s.mean.shape == s.peak.shape == s.thd().shape == (5, N, 2) and s.harmonics.shape == s.bins.shape == (5, N, 2, 3)
    for k, name in enumerate(("mean", "rms", "min", "max")):
        assert np.array_equal(getattr(s, name), out[..., k], equal_nan=True)
    one = mk(m, N).set_measurement(start=57, length=50, f0=(10, 441), harmonics=3).measure(u, time_major=True).measurement()
    w = s[1]
    assert w.count == one.count == 50 and np.array_equal(w.harmonics, one.harmonics) and np.array_equal(w.thd(), one.thd())
    assert np.array_equal(s.thd()[1], one.thd()) and np.array_equal(s.imd([0], [1, 2])[1], one.imd([0], [1, 2]))
    assert np.array_equal(s[-1].mean, s.mean[4], equal_nan=True) and s[-1].count == 0
    with pytest.raises(IndexError):
        s[5]
    part = r.measurement_series(2, 2)
    assert len(part) == 2 and part.starts.tolist() == [107, 157] and np.array_equal(part.rms, s.rms[2:4])
    from acme_jl_amd.runner import MeasurementSeries
    both = MeasurementSeries.concatenate([s, s])
    assert both.mean.shape == (5, 2 * N, 2) and both.counts.tolist() == s.counts.tolist()
