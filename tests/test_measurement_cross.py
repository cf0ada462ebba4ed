"""The measurement cross-spectrum (acme_batch_set_measurement_cross: transfer function and coherence) on the CPU wave
emulator: the window cut into the spectrum's segments, one input row and a measured row packed into one complex transform,
|X|^2, |Y|^2 and conj(X) Y accumulated, every bin against the replay on the stored u and y of an identical run without a
cross-spectrum, bit for bit (cross_ref).

1. segment geometry, windows, rows, the input row   2. fold + spectrum + cross, forms   3. paths (what the emulator has)
4. life cycle, errors   5. exact pins   6. accuracy against long double   7. system identification   8. noise   9. the object

The segment geometry, start and T are those of the GPU file.  The instance counts are not: the emulator walks the pairs one
by one, so the diode clipper runs at N = 3 (two outputs: N = 2); the forms, whose N the case fixes at 130, run the
pass-through model; the paths run the diode clipper at L = 64 (N = 6, T = 2100) and the pass-through model at L = 4096
(N = 2, T = 5200 from start = 23) and, oversampled by 3, at L = 64 over T = 460; the exact pins run without the long lead and
at L = 4096 over T = 12 000; the multi-device check runs the pass-through model (N = 4); the noise check runs the first 40 of
the 400 segments, the noise REFERENCE's own statistic, which needs no library, both 40 and 400."""
import numpy as np
import pytest

import cross_ref as CR
from test_measurement_spectrum import HostDevice, mk_for


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L, hop", CR.GEOMETRY)
def test_segment_geometry(emu_lib, L, hop):
    CR.check_geometry(mk_for(emu_lib), 3, 9000, 301, 10, L, hop)


def test_hop_of_one_sample(emu_lib):
    assert CR.check_geometry(mk_for(emu_lib), 3, 9000, 301, 10, 64, 1, length=700)[2] == 637


def test_a_bounded_window_cuts_a_segment(emu_lib):
    assert CR.check_geometry(mk_for(emu_lib), 3, 9000, 301, 10, 1024, 512, length=2000)[2:] == (2, 2000)


def test_fewer_samples_than_a_segment(emu_lib):
    got = CR.check_geometry(mk_for(emu_lib), 3, 9000, 301, 10, 4096, 2048, length=4095)
    assert got[2:] == (0, 4095) and np.isnan(got[0]).all() and np.isnan(got[1]).all()


def test_exactly_one_segment(emu_lib):
    assert CR.check_geometry(mk_for(emu_lib), 3, 9000, 301, 10, 4096, 2048, length=4096)[2:] == (1, 4096)


@pytest.mark.parametrize("win", ["rect", "hann", "random"])
def test_windows(emu_lib, win):
    CR.check_geometry(mk_for(emu_lib), 3, 9000, 301, 10, 128, 96, win=win)


@pytest.mark.parametrize("rows", [[1], None])
def test_two_outputs(emu_lib, rows):
    CR.check_geometry(mk_for(emu_lib), 2, 1000, 301, 10, 64, 37, rows=rows, two=True)


def test_the_second_input_row_beside_a_constant_one(emu_lib):
    CR.check_in_row(mk_for(emu_lib), 3, 700, 64, 37)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def test_a_fold_a_spectrum_and_a_cross_spectrum_together(emu_lib):
    CR.check_together(mk_for(emu_lib), 3, 9000)


def test_all_three_forms_carry_a_cross_spectrum(emu_lib):
    CR.check_forms(mk_for(emu_lib), 460, 64, 37, wire=True)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def test_paths_are_bit_identical(emu_lib, monkeypatch):
    CR.check_paths(mk_for(emu_lib), HostDevice(), 1, 2100, 64, 37, monkeypatch, N=6)


def test_paths_are_bit_identical_at_the_longest_segment(emu_lib, monkeypatch):
    CR.check_paths(mk_for(emu_lib), HostDevice(), 1, 5200, 4096, 1000, monkeypatch, N=2, S=23, wire=True)


def test_paths_are_bit_identical_oversampled(emu_lib, monkeypatch):
    CR.check_paths(mk_for(emu_lib), HostDevice(), 3, 460, 64, 32, monkeypatch, N=6, S=3, wire=True)


@pytest.mark.parametrize("L, hop", [(64, 37), (4096, 1000)])
def test_multi_device_runner_concatenates_the_shards(emu_lib, L, hop):
    from acme_jl_amd.runner import MultiDeviceRunner
    CR.check_multi_device(mk_for(emu_lib), lambda m, n: MultiDeviceRunner(m, n, devices=[0, 0], lib=emu_lib), L, hop, N=4, wire=True)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_life_cycle(emu_lib):
    CR.check_life_cycle(mk_for(emu_lib))


def test_set_matrices_carries_the_cross_spectrum(emu_lib):
    CR.check_set_matrices_carries_the_cross(mk_for(emu_lib))


def test_argument_errors(emu_lib):
    CR.check_errors(mk_for(emu_lib))


def test_a_batch_without_a_cross_spectrum_is_unchanged(emu_lib):
    CR.check_no_cross_invariance(mk_for(emu_lib), 67, 300)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_exact_segment_order(emu_lib):
    CR.check_exact(mk_for(emu_lib), 7, 256, 100, 2037)


def test_exact_segment_order_at_the_longest_segment(emu_lib):
    CR.check_exact(mk_for(emu_lib), 3, 4096, 2048, 12000)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 1000.0])
@pytest.mark.parametrize("L", [64, 1024, 4096])
def test_accuracy_against_long_double(emu_lib, L, scale):
    """worst ratios, emulator (the replay's, hence also the MI355X's): DESIGN.md 2.5k"""
    wx, wy, wb = CR.check_accuracy(mk_for(emu_lib), L, scale)
    print(f"L = {L}, |y| / |x| = {scale:g}: worst |X^ - X| / Ex = {wx:.3e}, |Y^ - Y| / Ey = {wy:.3e}, worst plane error / bound = {wb:.3e}")


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def test_transfer_function_of_the_sallen_key_filter(emu_lib):
    CR.check_sysid(mk_for(emu_lib))


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("segments", [None, 40])
def test_the_noise_reference_alone_is_incoherent(segments):
    K = segments or 400
    worst, dev = CR.noise_reference_statistic(segments)
    print(f"noise reference (noise_ref + numpy FFT), {K} segments: worst coherence {worst:.4f} (limit {CR.coherence_limit(K):.4f}), "
          f"pooled mean {dev:+.2f} standard errors from 1 / K")
    assert worst < CR.coherence_limit(K) and abs(dev) <= 4.0


def test_coherence_of_gaussian_rows(emu_lib):
    worst0, worst, dev = CR.check_noise(mk_for(emu_lib), segments=40)
    print(f"GAUSSIAN rows, 40 segments: y = x within {worst0:.3e} of its bound; independent rows: worst coherence {worst:.4f} "
          f"(limit {CR.coherence_limit(40):.4f}), pooled mean {dev:+.2f} standard errors from 1 / K")


# ---- 9 ------------------------------------------------------------------------------------------------------------------------
def test_measurement_cross_object(emu_lib):
    from acme_jl_amd.runner import MeasurementCross
    import exact_ref as X
    from helpers import FS
    N, L, T = 3, 64, 64 * 6
    n = np.arange(T)
    lv = np.array([1.0, 2.0, 0.5])[:, None]
    u = np.stack([lv * (0.25 + 1.5 * np.cos(2 * np.pi * 4 * n / L))[None],                          # row 0: DC and a line on bin 4
                  lv * (3.0 * np.cos(2 * np.pi * 4 * (n - 4) / L))[None]], axis=2)                  # row 1: twice the level, a quarter period late
    r = mk_for(emu_lib)(X.wire_model(2, FS), N).set_measurement().set_measurement_cross(0, L)
    r.measure(u, time_major=True)
    c = r.measurement_cross()
    assert c.segments == 11 and c.count == T and c.rows == (0, 1) and c.in_row == 0 and c.nfft == L and c.hop == 32
    assert c.sxx.shape == c.syy.shape == c.sxy.shape == (N, 2, 33) and c.sxy.dtype == np.complex128
    assert np.allclose(c.transfer()[:, 0, 4], 1.0, rtol=1e-13) and np.allclose(c.transfer()[:, 1, 4], -2.0j, rtol=1e-13)
    assert np.allclose(c.transfer("h2")[:, 1, 4], -2.0j, rtol=1e-13)
    assert np.allclose(c.coherence()[:, :, 4], 1.0, rtol=1e-13)
    with pytest.raises(ValueError, match="estimator"):
        c.transfer("h3")
    assert np.allclose(c.freqs(FS), np.arange(33) * FS / L)
    # the densities integrate to the rows' mean squares
    width = FS / L
    assert np.allclose(c.input_psd(FS).sum(axis=-1)[:, 0] * width, (0.25 ** 2 + 1.5 ** 2 / 2) * lv[:, 0] ** 2, rtol=1e-12)
    assert np.allclose(c.input_psd(FS)[:, 1], c.input_psd(FS)[:, 0], rtol=1e-9)                     # (the same x beside either row)
    assert np.allclose(c.output_psd(FS).sum(axis=-1)[:, 1] * width, (3.0 ** 2 / 2) * lv[:, 0] ** 2, rtol=1e-12)
    assert np.allclose(c.output_psd(FS)[:, 0], c.input_psd(FS)[:, 0], rtol=1e-12)                   # (row 0 is x itself)
    both = MeasurementCross.concatenate([c, c])
    assert both.sxx.shape == both.sxy.shape == (2 * N, 2, 33) and both.segments == 11 and both.in_row == 0
    with pytest.raises(ValueError, match="differ"):
        MeasurementCross.concatenate([c, MeasurementCross(c.sxx, c.syy, c.sxy, 10, c.count, c.rows, c.in_row, c.window, c.hop)])
    raw = r.measurement_cross(raw=True)
    assert np.array_equal(raw.sxx / 11, c.sxx) and np.array_equal(raw.sxy.imag / 11, c.sxy.imag)
