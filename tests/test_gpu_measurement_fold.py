"""The measurement fold (acme_batch_set_measurement_fold, synchronous averaging) on the MI355X: acme_meas_fold_kernel itself
-- a wave per pair, the phase of the chunk's first sample, the slot blocks side by side, periods below 64, the slots a short
chunk covers -- which the CPU emulator only walks as a plain loop.  Every slot against numpy on the stored y of an identical
run without a fold, bit for bit (fold_ref)."""
import numpy as np
import pytest

import fold_ref as FR

pytestmark = pytest.mark.gpu


def mk(model, n, **kw):
    from acme_jl_amd.runner import ModelRunner
    return ModelRunner(model, n, device=0, **kw)


# ---- 1. period geometry -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", FR.GEOMETRY)
def test_gpu_period_geometry(hip_lib, P):
    FR.check_geometry(mk, 131, 9000, 301, 10, P)


def test_gpu_the_last_slot_receives_one_sample(hip_lib):
    got, count = FR.check_geometry(mk, 131, 9000, 301, 10, 8699)
    assert count == 8699 and not np.isnan(got[1]).any()


def test_gpu_slots_no_sample_reaches_read_nan(hip_lib):
    got, count = FR.check_geometry(mk, 131, 9000, 301, 10, 9000)
    assert np.isnan(got[1][:, :, count:]).all() and not np.isnan(got[1][:, :, :count]).any()


def test_gpu_a_bounded_window(hip_lib):
    assert FR.check_geometry(mk, 131, 9000, 301, 10, 441, length=2000)[1] == 2000


# ---- 2. per-instance periods --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FR.period_cases()))
def test_gpu_per_instance_periods(hip_lib, name):
    FR.check_per_instance(mk, FR.period_cases()[name], 9000)


# ---- 3. rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [[1], None])
def test_gpu_two_outputs(hip_lib, rows):
    FR.check_geometry(mk, 99, 9000, 301, 10, 441, rows=rows, two=True)


# ---- 4. paths -----------------------------------------------------------------------------------------------------------------
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
    FR.check_paths(mk, TorchDevice(), k, 9000, monkeypatch)


# ---- 5. all three forms carry a fold ------------------------------------------------------------------------------------------
def test_gpu_all_three_forms_carry_a_fold(hip_lib):
    FR.check_forms(mk, 4300, [441])


# ---- 6. exact pins ------------------------------------------------------------------------------------------------------------
def test_gpu_exact_chain_order_behind_a_long_lead(hip_lib):
    """N = 77, P = 300, the window 2^20 + 1 samples behind arming.  Not 2^31: the pass-through model runs as two waves whose
    samples follow one another; 2^20 zeros are fed in four calls, and the whole test takes 1.2 s on the MI355X, so a lead of
    2^31, 2 048 times this one, extrapolates to minutes, not seconds (not run).  No run has m0 >= 2^31: that the phase of a
    chunk's first sample is right there rests on the code, which forms it in 64-bit integers throughout
    (acme_meas_fold_kernel: `A.m0 % P`)."""
    FR.check_exact(mk, 77, 300, 8237, lead=2 ** 20 + 1 - 37)


def test_gpu_exact_at_the_cap(hip_lib):
    FR.check_exact(mk, 3, FR.CAP, 140000)


# ---- 7. use level -------------------------------------------------------------------------------------------------------------
def test_gpu_bode_plot_from_the_folded_period(hip_lib):
    worst = FR.check_bode(mk)
    print(f"sallenkey, fold's line k against A_1: worst |error| / bound {worst:.3e}")
    assert worst <= 1.0


# ---- 8. life cycle and errors -------------------------------------------------------------------------------------------------
def test_gpu_life_cycle(hip_lib):
    FR.check_life_cycle(mk)


def test_gpu_set_matrices_carries_the_fold(hip_lib):
    FR.check_set_matrices_carries_the_fold(mk)


def test_gpu_argument_errors(hip_lib):
    FR.check_errors(mk)


def test_gpu_a_batch_without_a_fold_is_unchanged(hip_lib):
    FR.check_no_fold_invariance(mk, 131, 9000)


def test_gpu_multi_device_runner_concatenates_the_shards(hip_lib):
    from acme_jl_amd.runner import MultiDeviceRunner
    from test_measurement import clipper, clipper_u
    m, N, T = clipper(), 70, 1000
    u = clipper_u(N, T)
    per = np.where(np.arange(N) % 2, 441, 64)
    one = mk(m, N).set_measurement(start=3, f0=(10, 441), harmonics=4).set_measurement_fold(per)
    one.measure(u, time_major=True)
    md = MultiDeviceRunner(m, N, devices=[0, 0]).set_measurement(start=3, f0=(10, 441), harmonics=4).set_measurement_fold(per)
    md.measure(u)
    a, b = one.measurement_fold(), md.measurement_fold()
    assert a.count == b.count == T - 3 and np.array_equal(a.period, b.period)
    assert np.array_equal(a.mean, b.mean, equal_nan=True)
