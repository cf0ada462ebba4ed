"""The measurement ensemble (acme_batch_set_measurement_ensemble) on the MI355X: acme_meas_ensemble_kernel itself -- a lane per
recorded slot of the chunk, the walk over a group's member list with sixteen members' loads in flight and its remainder, the
four chains split over the waves of a block or four tiles a block, slots written once by the chunk that holds them -- which the
CPU emulator only walks as a plain loop.  Every chain against numpy on the stored y of an identical run without an ensemble,
bit for bit (ensemble_ref)."""
import numpy as np
import pytest

import ensemble_ref as ER

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]


def mk(model, n, **kw):
    from acme_jl_amd.runner import ModelRunner
    return ModelRunner(model, n, device=0, **kw)


# ---- 1. exact pins ------------------------------------------------------------------------------------------------------------
def test_gpu_exact_pins(hip_lib):
    ER.check_exact_pins(mk)


# ---- 2. geometry, 3. groups ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case, N", [("one group", 131), ("interleaved", 131), ("blocks", 200), ("one member each", 131)])
@pytest.mark.parametrize("stride", ER.STRIDES)
def test_gpu_geometry_and_groups(hip_lib, stride, case, N):
    """N = 131: two whole waves of members and a remainder (one group: the chains split over the waves of a block; one member
    each: four tiles a block); N = 200: blocks of 1, 63, 64 and 65 members, an empty group, seven instances in no group"""
    assert ER.check_geometry(mk, N, stride, case) == ER.slots(ER.LENGTH, stride)


# ---- 4. rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [[1], None])
def test_gpu_two_outputs(hip_lib, rows):
    ER.check_geometry(mk, 99, 3, "interleaved", rows=rows, two=True)
    ER.check_geometry(mk, 99, 1, "one member each", rows=rows, two=True)


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


@pytest.mark.parametrize("k, stride, weighted", [(1, 1, False), (1, 3, False), (1, 64, False), (1, 4097, False), (3, 3, False),
                                                 (1, 3, True), (3, 1, True)])
def test_gpu_paths_are_bit_identical(hip_lib, monkeypatch, k, stride, weighted):
    ER.check_paths(mk, TorchDevice(), k, 9000, monkeypatch, stride, weighted)


# ---- 6. coexistence ------------------------------------------------------------------------------------------------------------
def test_gpu_coexists_with_fold_spectrum_cross_and_target(hip_lib):
    ER.check_coexistence(mk, 131, 5000)


# ---- 7. a real circuit ---------------------------------------------------------------------------------------------------------
def test_gpu_band_of_the_clipper_over_its_levels(hip_lib):
    e = ER.check_use_level(mk)
    print("peak of the band per group:", np.array2string(e.max[:, 0].max(axis=1), precision=3))


# ---- 8. life cycle and refusals ------------------------------------------------------------------------------------------------
def test_gpu_life_cycle(hip_lib):
    ER.check_life_cycle(mk)


def test_gpu_set_matrices_carries_the_ensemble(hip_lib):
    ER.check_set_matrices_carries_the_ensemble(mk)


def test_gpu_refusals(hip_lib):
    ER.check_errors(mk)


# ---- 9. a non-finite instance --------------------------------------------------------------------------------------------------
def test_gpu_a_non_finite_instance_reads_nan_in_its_group_alone(hip_lib):
    ER.check_nan_instance(mk)


def test_gpu_two_non_finite_members_the_last_one_keeps_the_indices(hip_lib):
    ER.check_two_nan_members(mk)


# ---- 10. MultiDeviceRunner -----------------------------------------------------------------------------------------------------
def test_gpu_multi_device_runner_joins_by_group(hip_lib):
    from acme_jl_amd.runner import MultiDeviceRunner
    N, T = 70, 1000
    m, u = ER.wire_data(N, T)
    md = MultiDeviceRunner(m, N, devices=[0, 0])
    lo = md.ranges[1][0]
    groups = np.where(np.arange(N) < lo, np.arange(N) % 2, 2 + np.arange(N) % 3)        # groups 0, 1 | 2, 3, 4; 5 empty
    groups[[3, lo + 1]] = -1
    one = mk(m, N).set_measurement(start=3, length=900).set_measurement_ensemble(groups, 6, stride=3)
    one.measure(u, time_major=True)
    md.set_measurement(start=3, length=900).set_measurement_ensemble(groups, 6, stride=3).measure(u)
    a, b = ER.got(one), ER.got(md)
    assert a["filled"] == 300 and (a["argmax"][2:5] >= lo).all() and ER.same(a, b)
    groups[lo] = 0                                          # group 0 now straddles the shards
    with pytest.raises(ValueError, match="group 0"):
        MultiDeviceRunner(m, N, devices=[0, 0]).set_measurement(start=3, length=900).set_measurement_ensemble(groups, 6)
