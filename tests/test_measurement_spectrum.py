"""The measurement spectrum (acme_batch_set_measurement_spectrum, Welch-averaged periodograms) on the CPU wave emulator: the
window cut into overlapping segments, windowed, transformed and |X_k|^2 accumulated, every bin against the replay on the
stored y of an identical run without a spectrum, bit for bit (spectrum_ref).

1. segment geometry, windows, rows, forms, fold + spectrum   2. paths (what the emulator has)   3. life cycle, errors
4. exact pins   5. the table   6. accuracy against long double   7. Bode plot   8. noise floor

The segment geometry, start and T are those of the GPU file.  The instance counts are not: the emulator walks the pairs one
by one, so the diode clipper runs at N = 3 (two outputs: N = 2); the forms, whose N the case fixes at 130, run the
pass-through model; the paths run the diode clipper at L = 64 (N = 6, T = 2100) and the pass-through model at L = 4096
(N = 2, T = 5200 from start = 23) and, oversampled by 3, at L = 64 over T = 460; the exact pins run without the long lead and at L = 4096 over
T = 12 000; the multi-device check runs the pass-through model (N = 4); the noise check runs the first 40 of the 400 segments
(K = 320 periodograms, the standard error that of 320), the noise REFERENCE's own statistic, which needs no library, both 40
and 400."""
import numpy as np
import pytest

import spectrum_ref as SR

_MK = {}


def mk_for(lib):
    """one maker per library, so that spectrum_ref's shared plain runs are shared"""
    if id(lib) not in _MK:
        def mk(model, n, **kw):
            from acme_jl_amd.runner import ModelRunner
            return ModelRunner(model, n, lib=lib, **kw)
        _MK[id(lib)] = mk
    return _MK[id(lib)]


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L, hop", SR.GEOMETRY)
def test_segment_geometry(emu_lib, L, hop):
    SR.check_geometry(mk_for(emu_lib), 3, 9000, 301, 10, L, hop)


def test_hop_of_one_sample(emu_lib):
    assert SR.check_geometry(mk_for(emu_lib), 3, 9000, 301, 10, 64, 1, length=700)[2] == 637


def test_a_bounded_window_cuts_a_segment(emu_lib):
    got = SR.check_geometry(mk_for(emu_lib), 3, 9000, 301, 10, 1024, 512, length=2000)
    assert got[2:] == (2, 2000)


def test_fewer_samples_than_a_segment(emu_lib):
    got = SR.check_geometry(mk_for(emu_lib), 3, 9000, 301, 10, 4096, 2048, length=4095)
    assert got[2:] == (0, 4095) and np.isnan(got[0]).all() and np.isnan(got[1]).all()


def test_exactly_one_segment(emu_lib):
    assert SR.check_geometry(mk_for(emu_lib), 3, 9000, 301, 10, 4096, 2048, length=4096)[2:] == (1, 4096)


@pytest.mark.parametrize("win", ["rect", "hann", "random"])
def test_windows(emu_lib, win):
    SR.check_geometry(mk_for(emu_lib), 3, 9000, 301, 10, 128, 96, win=win)


@pytest.mark.parametrize("rows", [[1], None])
def test_two_outputs(emu_lib, rows):
    SR.check_geometry(mk_for(emu_lib), 2, 1000, 301, 10, 64, 37, rows=rows, two=True)


def test_a_fold_and_a_spectrum_together(emu_lib):
    SR.check_fold_and_spectrum(mk_for(emu_lib), 3, 9000)


def test_all_three_forms_carry_a_spectrum(emu_lib):
    SR.check_forms(mk_for(emu_lib), 460, 64, 37, wire=True)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
class HostDevice:
    """the emulator's "device memory" is host memory"""

    def put(self, a):
        return np.ascontiguousarray(a)

    def run(self, r, u, keep, T):
        from acme_jl_amd.runner import ModelRunner
        y = np.zeros((r.n, T, r.model.ny)) if keep else None
        ModelRunner.run_device(r, u.ctypes.data, y.ctypes.data if keep else 0, T)
        return y


def test_paths_are_bit_identical(emu_lib, monkeypatch):
    SR.check_paths(mk_for(emu_lib), HostDevice(), 1, 2100, 64, 37, monkeypatch, N=6)


def test_paths_are_bit_identical_at_the_longest_segment(emu_lib, monkeypatch):
    SR.check_paths(mk_for(emu_lib), HostDevice(), 1, 5200, 4096, 1000, monkeypatch, N=2, S=23, wire=True)


def test_paths_are_bit_identical_oversampled(emu_lib, monkeypatch):
    SR.check_paths(mk_for(emu_lib), HostDevice(), 3, 460, 64, 32, monkeypatch, N=6, S=3, wire=True)


@pytest.mark.parametrize("L, hop", [(64, 37), (4096, 1000)])
def test_multi_device_runner_concatenates_the_shards(emu_lib, L, hop):
    from acme_jl_amd.runner import MultiDeviceRunner
    SR.check_multi_device(mk_for(emu_lib), lambda m, n: MultiDeviceRunner(m, n, devices=[0, 0], lib=emu_lib), L, hop, N=4, wire=True)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def test_life_cycle(emu_lib):
    SR.check_life_cycle(mk_for(emu_lib))


def test_set_matrices_carries_the_spectrum(emu_lib):
    SR.check_set_matrices_carries_the_spectrum(mk_for(emu_lib))


def test_argument_errors(emu_lib):
    SR.check_errors(mk_for(emu_lib))


def test_a_batch_without_a_spectrum_is_unchanged(emu_lib):
    SR.check_no_spectrum_invariance(mk_for(emu_lib), 67, 300)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_exact_segment_order(emu_lib):
    SR.check_exact(mk_for(emu_lib), 7, 256, 100, 2037)


def test_exact_segment_order_at_the_longest_segment(emu_lib):
    SR.check_exact(mk_for(emu_lib), 3, 4096, 2048, 12000)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_the_table(emu_lib):
    worst = SR.check_table(mk_for(emu_lib))
    print(f"twiddle table: worst |tw - exact| = {worst:.3f} x 2^-53 (bound 1.5)")


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [64, 1024, 4096])
def test_accuracy_against_long_double(emu_lib, L):
    wx, wb = SR.check_accuracy(mk_for(emu_lib), L)
    print(f"L = {L}: worst |X^ - X| / E_s = {wx:.3e}, worst bin error / bound = {wb:.3e}")


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def test_bode_plot_from_the_spectrum(emu_lib):
    worst = SR.check_bode(mk_for(emu_lib))
    print(f"sallenkey, amplitude() at bin 16 k against |A_1|: worst |error| / bound {worst:.3e}")
    assert worst <= 1.0


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("segments", [None, 40])
def test_the_noise_reference_alone_holds_four_standard_errors(segments):
    z = SR.noise_reference_statistic(segments)
    print(f"noise reference (noise_ref + numpy FFT), {segments or 400} segments: worst bin {np.abs(z).max():.3f} standard errors")
    assert len(z) == 127 and np.abs(z).max() <= 4.0


def test_noise_floor_of_a_gaussian_row(emu_lib):
    worst = SR.check_noise(mk_for(emu_lib), segments=40)
    print(f"GAUSSIAN row, 127 bins over 320 periodograms: worst deviation {worst:.3f} standard errors")
    assert worst <= 4.0


def test_measurement_spectrum_object(emu_lib):
    from acme_jl_amd.runner import MeasurementSpectrum
    import exact_ref as X
    from helpers import FS
    N, L, T = 3, 64, 64 * 6
    n = np.arange(T)
    u = (0.25 + 1.5 * np.cos(2 * np.pi * 4 * n / L))[None, :, None] * np.array([1.0, 2.0, 0.5])[:, None, None]
    r = mk_for(emu_lib)(X.wire_model(1, FS), N).set_measurement().set_measurement_spectrum(L)
    r.measure(u, time_major=True)
    s = r.measurement_spectrum()
    assert s.segments == 11 and s.count == T and s.rows == (0,) and s.nfft == L and s.hop == 32 and s.power.shape == (N, 1, 33)
    assert np.allclose(s.amplitude()[:, 0, 4], [1.5, 3.0, 0.75], rtol=1e-13)          # a line on a bin, any window
    assert np.allclose(s.freqs(FS), np.arange(33) * FS / L)
    # the density integrates to the mean square: DC 0.25^2 (Hann spreads it over bins 0, 1) and the line's 1.5^2 / 2 (bins 3 ... 5)
    ms = s.band_power(FS, 0, FS / 2)
    assert np.allclose(ms[:, 0], (0.25 ** 2 + 1.5 ** 2 / 2) * np.array([1.0, 4.0, 0.25]), rtol=1e-12)
    assert np.allclose(s.band_power(FS, 2.5 * FS / L, 5.5 * FS / L)[:, 0], 1.5 ** 2 / 2 * np.array([1.0, 4.0, 0.25]), rtol=1e-12)
    both = MeasurementSpectrum.concatenate([s, s])
    assert both.power.shape == (2 * N, 1, 33) and both.segments == 11
    with pytest.raises(ValueError, match="differ"):
        MeasurementSpectrum.concatenate([s, MeasurementSpectrum(s.power, 10, s.count, s.rows, s.window, s.hop)])
    sums = r.measurement_spectrum(raw=True).power
    assert np.array_equal(sums / 11, s.power)
