"""The measurement histogram (acme_batch_set_measurement_histogram) on the MI355X: acme_meas_hist_kernel itself -- a wave per
pair, the lanes' strided loads and their ragged end, LDS atomic adds into the wave's own counters with and without the runs of
equal counters aggregated, the blocks' waves following from B, the plain add into the 64-bit counters -- which the CPU emulator
only walks as a plain loop.  Every counter against numpy on the stored y of an identical run without a histogram, integer for
integer (histogram_ref)."""
import numpy as np
import pytest

import histogram_ref as HR

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]


def mk(model, n, **kw):
    from acme_jl_amd.runner import ModelRunner
    return ModelRunner(model, n, device=0, **kw)


# ---- 1. exact pins ------------------------------------------------------------------------------------------------------------
def test_gpu_exact_pins(hip_lib):
    HR.check_exact_pins(mk)


# ---- 2. geometry --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [131, 200])
@pytest.mark.parametrize("name", HR.SIGNALS)
@pytest.mark.parametrize("B", HR.BINS)
def test_gpu_geometry(hip_lib, B, name, N):
    """N = 131 and 200 pairs: 131 is no multiple of the four or two waves of a block (B up to 2 045; 4 096 has one), and both
    leave the last block's waves without a pair"""
    HR.check_geometry(mk, N, B, name)


@pytest.mark.parametrize("agg", ["0", "1"])
@pytest.mark.parametrize("name", ["constant", "noise"])
def test_gpu_both_shapes_of_the_kernel(hip_lib, monkeypatch, agg, name):
    monkeypatch.setenv("ACME_HIST_AGG", agg)
    for B in (65, 4096):
        HR.check_geometry(mk, 131, B, name)


# ---- 3. rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [[1], None])
def test_gpu_two_outputs(hip_lib, rows):
    HR.check_geometry(mk, 99, 65, "sine", rows=rows, two=True)
    HR.check_geometry(mk, 99, 1000, "noise", rows=rows, two=True)


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


@pytest.mark.parametrize("k, B, mode, weighted", [(1, 64, "signed", False), (1, 1000, "abs", False), (1, 4096, "signed", False),
                                                  (3, 65, "signed", False), (3, 63, "abs", True), (1, 63, "signed", True)])
def test_gpu_paths_are_identical(hip_lib, monkeypatch, k, B, mode, weighted):
    HR.check_paths(mk, TorchDevice(), k, 9000, monkeypatch, B, mode, weighted)


# ---- 5. coexistence ------------------------------------------------------------------------------------------------------------
def test_gpu_coexists_with_fold_spectrum_cross_target_and_ensemble(hip_lib):
    HR.check_coexistence(mk, 131, 5000)


# ---- 6. life cycle and refusals ------------------------------------------------------------------------------------------------
def test_gpu_life_cycle(hip_lib):
    HR.check_life_cycle(mk)


def test_gpu_set_matrices_carries_the_histogram(hip_lib):
    HR.check_set_matrices_carries_the_histogram(mk)


def test_gpu_refusals(hip_lib):
    HR.check_errors(mk)


def test_gpu_the_cap_is_accepted_and_one_counter_more_refused(hip_lib):
    HR.check_cap(mk, 65536, accept=True)


# ---- 7. a non-finite instance --------------------------------------------------------------------------------------------------
def test_gpu_a_non_finite_instance_counts_in_nan_alone(hip_lib):
    HR.check_nan_instance(mk)


# ---- 8. MultiDeviceRunner -----------------------------------------------------------------------------------------------------
def test_gpu_multi_device_runner_equals_the_single_runner(hip_lib):
    from acme_jl_amd.runner import MultiDeviceRunner
    N, T = 70, 1000
    u, _, _ = HR.signal(mk, "sine", N, T)
    m = HR.X.wire_model(1, HR.FS)
    amp = np.linspace(0.05, 1.3, N)
    one = mk(m, N).set_measurement(start=3, length=900).set_measurement_histogram(65, -0.9 * amp, 0.8 * amp, "abs")
    one.measure(u, time_major=True)
    md = MultiDeviceRunner(m, N, devices=[0, 0])
    md.set_measurement(start=3, length=900).set_measurement_histogram(65, -0.9 * amp, 0.8 * amp, "abs").measure(u)
    a, b = one.measurement_histogram(), md.measurement_histogram()
    assert a.count == b.count == 900 and a.mode == b.mode == "abs"
    for k in ("counts", "under", "over", "nan", "lo", "hi", "scale"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert (a.counts.sum(axis=-1) + a.under + a.over + a.nan == 900).all()
    # a scalar range on every shard
    md.set_measurement(start=3, length=900).set_measurement_histogram(8, -1.0, 1.0).measure(u)
    one.set_measurement(start=3, length=900).set_measurement_histogram(8, -1.0, 1.0).measure(u, time_major=True)
    assert np.array_equal(md.measurement_histogram().counts, one.measurement_histogram().counts)


# ---- 9. a real circuit ---------------------------------------------------------------------------------------------------------
def test_gpu_clipper_over_its_levels(hip_lib):
    h, top, near = HR.check_use_level(mk)
    print("share in the top tenth of the range:", np.array2string(top, precision=3))
    print("share above 80 % of the clipped peak:", np.array2string(near, precision=3))


def test_gpu_measurement_histogram_object(hip_lib):
    HR.check_object(mk)
