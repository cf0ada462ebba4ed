"""The measurement spectrum (acme_batch_set_measurement_spectrum, Welch-averaged periodograms) on the MI355X:
acme_meas_spectrum_kernel itself -- a block per pair, the transform in LDS with two stages a pass in registers, several short
segments side by side, the carry ring across chunks -- which the CPU emulator only walks as a plain loop.  Every bin against
the replay on the stored y of an identical run without a spectrum, bit for bit (spectrum_ref).

Worst ratios observed on the MI355X are recorded in DESIGN.md 2.5j."""
import numpy as np
import pytest

import spectrum_ref as SR

pytestmark = pytest.mark.gpu


def mk(model, n, **kw):
    from acme_jl_amd.runner import ModelRunner
    return ModelRunner(model, n, device=0, **kw)


# ---- 1. bit for bit: segment geometry, windows, rows, forms ------------------------------------------------------------------
@pytest.mark.parametrize("L, hop", SR.GEOMETRY)
def test_gpu_segment_geometry(hip_lib, L, hop):
    SR.check_geometry(mk, 131, 9000, 301, 10, L, hop)


def test_gpu_hop_of_one_sample(hip_lib):
    assert SR.check_geometry(mk, 131, 9000, 301, 10, 64, 1, length=700)[2] == 637


def test_gpu_a_bounded_window_cuts_a_segment(hip_lib):
    assert SR.check_geometry(mk, 131, 9000, 301, 10, 1024, 512, length=2000)[2:] == (2, 2000)


def test_gpu_fewer_samples_than_a_segment(hip_lib):
    got = SR.check_geometry(mk, 131, 9000, 301, 10, 4096, 2048, length=4095)
    assert got[2:] == (0, 4095) and np.isnan(got[0]).all() and np.isnan(got[1]).all()


def test_gpu_exactly_one_segment(hip_lib):
    assert SR.check_geometry(mk, 131, 9000, 301, 10, 4096, 2048, length=4096)[2:] == (1, 4096)


@pytest.mark.parametrize("win", ["rect", "hann", "random"])
def test_gpu_windows(hip_lib, win):
    SR.check_geometry(mk, 131, 9000, 301, 10, 128, 96, win=win)


@pytest.mark.parametrize("rows", [[1], None])
def test_gpu_two_outputs(hip_lib, rows):
    SR.check_geometry(mk, 99, 9000, 301, 10, 1024, 512, rows=rows, two=True)


def test_gpu_a_fold_and_a_spectrum_together(hip_lib):
    SR.check_fold_and_spectrum(mk, 131, 9000)


def test_gpu_all_three_forms_carry_a_spectrum(hip_lib):
    SR.check_forms(mk, 4300, 1024, 512)


# ---- 2. paths -----------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("k, L, hop", [(1, 64, 37), (1, 4096, 1000), (3, 64, 37), (3, 4096, 1000)])
def test_gpu_paths_are_bit_identical(hip_lib, monkeypatch, k, L, hop):
    SR.check_paths(mk, TorchDevice(), k, 9000, L, hop, monkeypatch)


@pytest.mark.parametrize("L, hop", [(64, 37), (4096, 1000)])
def test_gpu_multi_device_runner_concatenates_the_shards(hip_lib, L, hop):
    from acme_jl_amd.runner import MultiDeviceRunner
    SR.check_multi_device(mk, lambda m, n: MultiDeviceRunner(m, n, devices=[0, 0]), L, hop)


# ---- 3. life cycle and errors -------------------------------------------------------------------------------------------------
def test_gpu_life_cycle(hip_lib):
    SR.check_life_cycle(mk)


def test_gpu_set_matrices_carries_the_spectrum(hip_lib):
    SR.check_set_matrices_carries_the_spectrum(mk)


def test_gpu_argument_errors(hip_lib):
    SR.check_errors(mk)


def test_gpu_a_batch_without_a_spectrum_is_unchanged(hip_lib):
    SR.check_no_spectrum_invariance(mk, 131, 9000)


# ---- 4. exact pins ------------------------------------------------------------------------------------------------------------
def test_gpu_exact_segment_order_behind_a_long_lead(hip_lib):
    """N = 77, (L, hop) = (256, 100), the window 2^20 + 1 samples behind arming.  No run has m >= 2^31: that a segment's sample
    numbers and the ring's slots are right there rests on the code, which forms them in 64-bit integers throughout
    (acme_meas_spectrum_kernel: `(s0 + g) * A.hop + j`, `m & (L - 1)`; meas_spec_segments)."""
    SR.check_exact(mk, 77, 256, 100, 8237, lead=2 ** 20 + 1 - 37)


def test_gpu_exact_at_the_longest_segment(hip_lib):
    SR.check_exact(mk, 3, 4096, 2048, 140000)


# ---- 5. the table -------------------------------------------------------------------------------------------------------------
def test_gpu_the_table(hip_lib):
    worst = SR.check_table(mk)
    print(f"twiddle table: worst |tw - exact| = {worst:.3f} x 2^-53 (bound 1.5)")


# ---- 6. accuracy against exact arithmetic -------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [64, 1024, 4096])
def test_gpu_accuracy_against_long_double(hip_lib, L):
    wx, wb = SR.check_accuracy(mk, L)
    print(f"L = {L}: worst |X^ - X| / E_s = {wx:.3e}, worst bin error / bound = {wb:.3e}")


# ---- 7, 8. use level ----------------------------------------------------------------------------------------------------------
def test_gpu_bode_plot_from_the_spectrum(hip_lib):
    worst = SR.check_bode(mk)
    print(f"sallenkey, amplitude() at bin 16 k against |A_1|: worst |error| / bound {worst:.3e}")
    assert worst <= 1.0


def test_gpu_noise_floor_of_a_gaussian_row(hip_lib):
    worst = SR.check_noise(mk)
    print(f"GAUSSIAN row, 127 bins over 3 200 periodograms: worst deviation {worst:.3f} standard errors")
    assert worst <= 4.0
