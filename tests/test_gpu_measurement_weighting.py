"""The measurement weighting (acme_batch_set_measurement_weighting) on the MI355X: acme_meas_weight_kernel itself -- four
waves staging a tile jointly through two LDS buffers, the first wave walking the chains in place, partial waves, blocks and
tiles, the states across slices and calls -- which the CPU emulator only walks as a plain loop.  The weighted samples against
a numpy replay of the contract on the stored y of an identical run without a weighting, bit for bit, and every form on them
through the existing replays (weighting_ref)."""
import numpy as np
import pytest

import weighting_ref as WR

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]


def mk(model, n, **kw):
    from acme_jl_amd.runner import ModelRunner
    return ModelRunner(model, n, device=0, **kw)


# ---- 1. exact pins ------------------------------------------------------------------------------------------------------------
def test_gpu_identity_section_changes_nothing(hip_lib):
    WR.check_identity(mk)


@pytest.mark.parametrize("case", ["delay", "delay, split", "1 2 1", "running sum", "8 delays"])
def test_gpu_exact_pins(hip_lib, case):
    WR.check_integer_pins(mk, case)


# ---- 2. geometry: a partial wave (N = 3), one block, a block and a pair, two blocks and a partial wave --------------------------
@pytest.mark.parametrize("name", ["S = 1", "S = 2", "S = 3", "S = 8", "A"])
@pytest.mark.parametrize("N", [3, 64, 65, 130, 131])
def test_gpu_geometry(hip_lib, N, name):
    WR.check_geometry(mk, N, 9000, 301, name)


@pytest.mark.parametrize("rows", [[1], None])
def test_gpu_two_outputs(hip_lib, rows):
    WR.check_geometry(mk, 99, 9000, 301, "S = 3", rows=rows, two=True)


# ---- 3. every path ------------------------------------------------------------------------------------------------------------
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
    WR.check_paths(mk, TorchDevice(), k, 9000, monkeypatch)


# ---- 4. coexistence -----------------------------------------------------------------------------------------------------------
def test_gpu_coexists_with_fold_spectrum_cross_and_target(hip_lib):
    WR.check_coexistence(mk, 131, 5000)


def test_gpu_series_and_per_instance_harmonics_read_the_weighted_rows(hip_lib):
    WR.check_series_and_per_instance(mk, 131, 5000)


# ---- 5. life cycle and errors -------------------------------------------------------------------------------------------------
def test_gpu_life_cycle(hip_lib):
    WR.check_life_cycle(mk)


def test_gpu_set_matrices_carries_the_weighting(hip_lib):
    WR.check_set_matrices_carries_the_weighting(mk)


def test_gpu_argument_errors(hip_lib):
    WR.check_errors(mk)


def test_gpu_a_batch_without_a_weighting_is_unchanged(hip_lib):
    WR.check_no_weighting_invariance(mk, 131, 9000)


# ---- 6. a non-finite instance -------------------------------------------------------------------------------------------------
def test_gpu_a_non_finite_instance_reads_nan_only_itself(hip_lib):
    WR.check_nan_instance(mk)


# ---- 7. use level -------------------------------------------------------------------------------------------------------------
def test_gpu_loudness_of_the_bs1770_sine(hip_lib):
    """(d) 997 Hz, unit amplitude, K weighting, blocks of 19 200 samples every 4 800 at 48 kHz: -3.01 +- 0.01 LKFS from the third
    block on"""
    WR.check_loudness(mk)


def test_gpu_target_behind_the_a_weighting(hip_lib):
    """(e) See == 0.0 at the recorded instance, and it is the argmin of the ESR"""
    mt = WR.check_target_behind_a_weighting(mk)
    print("ESR per level behind the A weighting:", np.array2string(mt.esr[:, 0], precision=3))


# ---- 8. MultiDeviceRunner -----------------------------------------------------------------------------------------------------
def test_gpu_multi_device_runner_hands_every_shard_the_cascade(hip_lib):
    from acme_jl_amd.runner import MultiDeviceRunner
    WR.check_multi_device(mk, lambda m, n: MultiDeviceRunner(m, n, devices=[0, 0]))
