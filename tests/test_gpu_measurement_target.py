"""The measurement target (acme_batch_set_measurement_target) on the MI355X: acme_meas_target_kernel itself -- the chains of a
pair split over three waves, the phase of the chunk's first sample, uniform waves that broadcast their target tile and mixed
waves that gather per lane, the carries across chunks -- which the CPU emulator only walks as a plain loop.  Every chain
against numpy on the stored y of an identical run without a target, bit for bit (target_ref)."""
import numpy as np
import pytest

import target_ref as TR

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]


def mk(model, n, **kw):
    from acme_jl_amd.runner import ModelRunner
    return ModelRunner(model, n, device=0, **kw)


# ---- 1. exact pins ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["t = u", "t = 0", "t = -u"])
def test_gpu_exact_pins(hip_lib, case):
    TR.check_exact_pins(mk, case)


# ---- 2. the target's length against the chunk and the tile --------------------------------------------------------------------
@pytest.mark.parametrize("P", TR.GEOMETRY)
def test_gpu_target_length_geometry(hip_lib, P):
    """N = 131: two whole waves and a remainder.  A shared lag: uniform waves throughout; per instance: mixed waves"""
    TR.check_geometry(mk, 131, 9000, 301, P, [0, 1, P - 1, "per instance"])


def test_gpu_a_bounded_window(hip_lib):
    assert TR.check_geometry(mk, 131, 9000, 301, 65, [0, "per instance"], length=4200) == 4200


# ---- 3. per-instance which and lag --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [130, 131])
def test_gpu_per_instance_which_and_lag(hip_lib, N):
    TR.check_per_instance(mk, N, 5000)


def test_gpu_per_instance_arrays_of_one_tuple(hip_lib):
    TR.check_per_instance(mk, 130, 5000, one_tuple=True)


# ---- 4. rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [[1], None])
def test_gpu_two_outputs(hip_lib, rows):
    TR.check_geometry(mk, 99, 9000, 301, 65, [3, "per instance"], rows=rows, two=True)


# ---- 5. paths -----------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("k, P", [(1, 1), (1, 5), (1, 64), (1, 97), (1, 4099), (3, 97)])
def test_gpu_paths_are_bit_identical(hip_lib, monkeypatch, k, P):
    TR.check_paths(mk, TorchDevice(), k, 9000, monkeypatch, P=P)


# ---- 6. c = 0, and a reset zeroes the carries ---------------------------------------------------------------------------------
def test_gpu_c_zero_and_a_reset_zeroes_the_carries(hip_lib):
    TR.check_c_zero_and_reset(mk, 131, 5000)


# ---- 7. coexistence ------------------------------------------------------------------------------------------------------------
def test_gpu_coexists_with_fold_spectrum_and_cross(hip_lib):
    TR.check_coexistence(mk, 131, 5000)


# ---- 8. use level -------------------------------------------------------------------------------------------------------------
def test_gpu_esr_of_candidates_against_a_recording(hip_lib):
    mt = TR.check_use_level(mk)
    print("ESR per level:", np.array2string(mt.esr[:, 0], precision=3))


# ---- 9. life cycle and errors -------------------------------------------------------------------------------------------------
def test_gpu_life_cycle(hip_lib):
    TR.check_life_cycle(mk)


def test_gpu_set_matrices_carries_the_target(hip_lib):
    TR.check_set_matrices_carries_the_target(mk)


def test_gpu_argument_errors(hip_lib):
    TR.check_errors(mk)


def test_gpu_a_batch_without_a_target_is_unchanged(hip_lib):
    TR.check_no_target_invariance(mk, 131, 9000)


# ---- 10. a non-finite instance ------------------------------------------------------------------------------------------------
def test_gpu_a_non_finite_instance_reads_nan_only_itself(hip_lib):
    TR.check_nan_instance(mk)


def test_gpu_multi_device_runner_shards_which_and_lag(hip_lib):
    from acme_jl_amd.runner import MultiDeviceRunner
    N, T = 70, 1000
    m, u = TR.wire_data(N, T)
    tgt = TR.table(5, 3, 1, 41)
    which, lag = np.arange(N) % 3, (5 * np.arange(N)) % 41
    one = mk(m, N).set_measurement(start=3).set_measurement_target(tgt, which=which, lag=lag, preemphasis=TR.C_PATHS)
    one.measure(u, time_major=True)
    md = MultiDeviceRunner(m, N, devices=[0, 0]).set_measurement(start=3)
    md.set_measurement_target(tgt, which=which, lag=lag, preemphasis=TR.C_PATHS).measure(u)
    a, b = one.measurement_target(), md.measurement_target()
    assert a.count == b.count == T - 3 and np.array_equal(a.sums, b.sums) and np.array_equal(a.error_mean, b.error_mean)
