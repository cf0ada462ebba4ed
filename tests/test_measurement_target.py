"""The measurement target (acme_batch_set_measurement_target) on the CPU wave emulator: the residual of the measured window
against a looped waveform of the caller's, every chain against numpy on the stored y of an identical run without a target,
bit for bit (target_ref).

1. exact pins   2. the target's length against the chunk and the tile   3. per-instance which / lag   4. rows   5. paths
6. c = 0 and the reset of the carries   7. coexistence with fold, spectrum and cross-spectrum   8. use level
9. life cycle, errors, a batch without a target is what it was   10. a non-finite instance

The lengths, start and T are those of the GPU file.  The instance counts are not where an emulated run is slow: the emulator
walks the pairs one by one (uniform and mixed waves do not exist here), so the geometry runs at N = 3 with the lags 0, 1 and
P - 1 dealt out over the instances in ONE run per length, the per-instance cases (N = 130 and 131, as the cases fix them) over
T = 200 with three of the distinct tuples against their shared arming, the paths at N = 6 over T = 460 (no call reaches a
chunk boundary there: the slices of 150 and the chunks of one tile are what puts a chunk's first sample at every phase), and
the two-output model at N = 2 over T = 1000.  test_gpu_measurement_target.py runs the full shapes and MultiDeviceRunner."""
import numpy as np
import pytest

import target_ref as TR

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")

_MK = {}


def mk_for(lib):
    """one maker per library, so that target_ref's shared plain runs are shared"""
    if id(lib) not in _MK:
        def mk(model, n, **kw):
            from acme_jl_amd.runner import ModelRunner
            return ModelRunner(model, n, lib=lib, **kw)
        _MK[id(lib)] = mk
    return _MK[id(lib)]


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["t = u", "t = 0", "t = -u"])
def test_exact_pins(emu_lib, case):
    TR.check_exact_pins(mk_for(emu_lib), case, N=3, T=1500)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", TR.GEOMETRY)
def test_target_length_geometry(emu_lib, P):
    TR.check_geometry(mk_for(emu_lib), 3, 9000, 301, P, ["per instance"])


def test_a_bounded_window(emu_lib):
    assert TR.check_geometry(mk_for(emu_lib), 3, 9000, 301, 65, ["per instance"], length=4200) == 4200


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [130, 131])
def test_per_instance_which_and_lag(emu_lib, N):
    TR.check_per_instance(mk_for(emu_lib), N, 200, shared=3)


def test_per_instance_arrays_of_one_tuple(emu_lib):
    TR.check_per_instance(mk_for(emu_lib), 130, 200, one_tuple=True)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [[1], None])
def test_two_outputs(emu_lib, rows):
    TR.check_geometry(mk_for(emu_lib), 2, 1000, 301, 65, ["per instance"], rows=rows, two=True)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
class HostDevice:
    """the emulator's "device memory" is host memory"""

    def put(self, a):
        return np.ascontiguousarray(a)

    def run(self, r, u, keep, T):
        from acme_jl_amd.runner import ModelRunner
        y = np.zeros((r.n, T, r.model.ny)) if keep else None
        ModelRunner.run_device(r, u.ctypes.data, y.ctypes.data if keep else 0, T)
        return y


@pytest.mark.parametrize("k, P", [(1, 1), (1, 5), (1, 64), (1, 97), (3, 97)])
def test_paths_are_bit_identical(emu_lib, monkeypatch, k, P):
    TR.check_paths(mk_for(emu_lib), HostDevice(), k, 460, monkeypatch, N=6, P=P)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_c_zero_and_a_reset_zeroes_the_carries(emu_lib):
    TR.check_c_zero_and_reset(mk_for(emu_lib), 5, 300)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def test_coexists_with_fold_spectrum_and_cross(emu_lib):
    TR.check_coexistence(mk_for(emu_lib), 5, 400)


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
def test_esr_of_candidates_against_a_recording(emu_lib):
    TR.check_use_level(mk_for(emu_lib))


# ---- 9 ------------------------------------------------------------------------------------------------------------------------
def test_life_cycle(emu_lib):
    TR.check_life_cycle(mk_for(emu_lib))


def test_set_matrices_carries_the_target(emu_lib):
    TR.check_set_matrices_carries_the_target(mk_for(emu_lib))


def test_argument_errors(emu_lib):
    TR.check_errors(mk_for(emu_lib))


def test_a_batch_without_a_target_is_unchanged(emu_lib):
    TR.check_no_target_invariance(mk_for(emu_lib), 67, 300)


# ---- 10 -----------------------------------------------------------------------------------------------------------------------
def test_a_non_finite_instance_reads_nan_only_itself(emu_lib):
    TR.check_nan_instance(mk_for(emu_lib))


def test_measurement_target_object(emu_lib):
    from acme_jl_amd.runner import MeasurementTarget
    import exact_ref as X
    from helpers import FS
    N, T = 4, 64
    u = np.ones((N, T, 1)) * np.array([1.0, 2.0, 3.0, 4.0])[:, None, None]
    r = mk_for(emu_lib)(X.wire_model(1, FS), N).set_measurement().set_measurement_target(np.full(8, 2.0))
    r.measure(u, time_major=True)
    mt = r.measurement_target()
    assert mt.count == T and mt.rows == (0,) and mt.sums.shape == (N, 1, 7)
    assert mt.esr[:, 0].tolist() == [0.25, 0.0, 0.25, 1.0] and mt.gain[:, 0].tolist() == [0.5, 1.0, 1.5, 2.0]
    assert mt.error_rms[:, 0].tolist() == [1.0, 0.0, 1.0, 2.0] and mt.error_peak[:, 0].tolist() == [1.0, 0.0, 1.0, 2.0]
    assert mt.error_mean[:, 0].tolist() == [-1.0, 0.0, 1.0, 2.0]
    assert np.array_equal(mt.esr_preemphasis, mt.esr)       # (c = 0)
    assert np.allclose(mt.null_db[[0, 3], 0], [10 * np.log10(0.25), 0.0]) and mt.null_db[1, 0] == -np.inf
    both = MeasurementTarget.concatenate([mt, mt])
    assert both.sums.shape == (2 * N, 1, 7) and both.count == T and np.array_equal(both.error_mean[N:], mt.error_mean)
    with pytest.raises(ValueError, match="differ"):
        MeasurementTarget.concatenate([mt, MeasurementTarget(mt.sums, T - 1, mt.rows)])
    with pytest.raises(ValueError, match="error_mean"):
        r.measurement_target(raw=True).error_mean
