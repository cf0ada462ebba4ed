"""The measurement cross-spectrum (acme_batch_set_measurement_cross: transfer function and coherence) on the MI355X:
acme_meas_cross_kernel itself -- a block per pair, one input row and a measured row packed into one complex transform in LDS,
two stages a pass in registers, several short segments side by side, the two rings across chunks, the split and the four
chains per bin -- which the CPU emulator only walks as a plain loop.  Every bin against the replay on the stored u and y of an
identical run without a cross-spectrum, bit for bit (cross_ref).

Worst ratios observed on the MI355X are recorded in DESIGN.md 2.5k."""
import numpy as np
import pytest

import cross_ref as CR
from test_gpu_measurement_spectrum import TorchDevice, mk

pytestmark = pytest.mark.gpu


# ---- 1. bit for bit: segment geometry, windows, rows, the input row -------------------------------------------------------------
@pytest.mark.parametrize("L, hop", CR.GEOMETRY)
def test_gpu_segment_geometry(hip_lib, L, hop):
    CR.check_geometry(mk, 131, 9000, 301, 10, L, hop)


def test_gpu_hop_of_one_sample(hip_lib):
    assert CR.check_geometry(mk, 131, 9000, 301, 10, 64, 1, length=700)[2] == 637


def test_gpu_a_bounded_window_cuts_a_segment(hip_lib):
    assert CR.check_geometry(mk, 131, 9000, 301, 10, 1024, 512, length=2000)[2:] == (2, 2000)


def test_gpu_fewer_samples_than_a_segment(hip_lib):
    got = CR.check_geometry(mk, 131, 9000, 301, 10, 4096, 2048, length=4095)
    assert got[2:] == (0, 4095) and np.isnan(got[0]).all() and np.isnan(got[1]).all()


def test_gpu_exactly_one_segment(hip_lib):
    assert CR.check_geometry(mk, 131, 9000, 301, 10, 4096, 2048, length=4096)[2:] == (1, 4096)


@pytest.mark.parametrize("win", ["rect", "hann", "random"])
def test_gpu_windows(hip_lib, win):
    CR.check_geometry(mk, 131, 9000, 301, 10, 128, 96, win=win)


@pytest.mark.parametrize("rows", [[1], None])
def test_gpu_two_outputs(hip_lib, rows):
    CR.check_geometry(mk, 99, 9000, 301, 10, 1024, 512, rows=rows, two=True)


def test_gpu_the_second_input_row_beside_a_constant_one(hip_lib):
    CR.check_in_row(mk, 131, 9000, 1024, 512)


# ---- 2. together ----------------------------------------------------------------------------------------------------------------
def test_gpu_a_fold_a_spectrum_and_a_cross_spectrum_together(hip_lib):
    CR.check_together(mk, 131, 9000)


def test_gpu_all_three_forms_carry_a_cross_spectrum(hip_lib):
    CR.check_forms(mk, 4300, 1024, 512)


# ---- 3. paths -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, L, hop", [(1, 64, 37), (1, 4096, 1000), (3, 64, 37), (3, 4096, 1000)])
def test_gpu_paths_are_bit_identical(hip_lib, monkeypatch, k, L, hop):
    CR.check_paths(mk, TorchDevice(), k, 9000, L, hop, monkeypatch)


@pytest.mark.parametrize("L, hop", [(64, 37), (4096, 1000)])
def test_gpu_multi_device_runner_concatenates_the_shards(hip_lib, L, hop):
    from acme_jl_amd.runner import MultiDeviceRunner
    CR.check_multi_device(mk, lambda m, n: MultiDeviceRunner(m, n, devices=[0, 0]), L, hop)


# ---- 4. life cycle and errors ---------------------------------------------------------------------------------------------------
def test_gpu_life_cycle(hip_lib):
    CR.check_life_cycle(mk)


def test_gpu_set_matrices_carries_the_cross_spectrum(hip_lib):
    CR.check_set_matrices_carries_the_cross(mk)


def test_gpu_argument_errors(hip_lib):
    CR.check_errors(mk)


def test_gpu_a_batch_without_a_cross_spectrum_is_unchanged(hip_lib):
    CR.check_no_cross_invariance(mk, 131, 9000)


# ---- 5. exact pins --------------------------------------------------------------------------------------------------------------
def test_gpu_exact_segment_order_behind_a_long_lead(hip_lib):
    """N = 77, (L, hop) = (256, 100), the window 2^20 + 1 samples behind arming.  No run has m >= 2^31: that a segment's sample
    numbers and the rings' slots are right there rests on the code, which forms them in 64-bit integers throughout
    (acme_meas_cross_kernel: `(s0 + g) * A.hop + j`, `m & (L - 1)`; meas_spec_segments)."""
    CR.check_exact(mk, 77, 256, 100, 8237, lead=2 ** 20 + 1 - 37)


def test_gpu_exact_at_the_longest_segment(hip_lib):
    CR.check_exact(mk, 3, 4096, 2048, 140000)


# ---- 6. accuracy against exact arithmetic ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 1000.0])
@pytest.mark.parametrize("L", [64, 1024, 4096])
def test_gpu_accuracy_against_long_double(hip_lib, L, scale):
    wx, wy, wb = CR.check_accuracy(mk, L, scale)
    print(f"L = {L}, |y| / |x| = {scale:g}: worst |X^ - X| / Ex = {wx:.3e}, |Y^ - Y| / Ey = {wy:.3e}, worst plane error / bound = {wb:.3e}")


# ---- 7, 8. use level ------------------------------------------------------------------------------------------------------------
def test_gpu_transfer_function_of_the_sallen_key_filter(hip_lib):
    CR.check_sysid(mk)


def test_gpu_coherence_of_gaussian_rows(hip_lib):
    worst0, worst, dev = CR.check_noise(mk)
    print(f"GAUSSIAN rows, 400 segments: y = x within {worst0:.3e} of its bound; independent rows: worst coherence {worst:.4f} "
          f"(limit {CR.coherence_limit(400):.4f}), pooled mean {dev:+.2f} standard errors from 1 / K")
