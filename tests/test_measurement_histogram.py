"""The measurement histogram (acme_batch_set_measurement_histogram) on the CPU wave emulator: the amplitude distribution of
every (instance, row) pair, every counter against numpy on the stored y of an identical run without a histogram, integer for
integer (histogram_ref).

1. exact pins   2. geometry (window, split calls, signals)   3. rows   4. paths   5. coexistence   6. life cycle and refusals
7. a non-finite instance   9. a real circuit   (8, MultiDeviceRunner, is in the GPU file)

The window and the bin counts are those of the GPU file.  The emulator walks every pair as a plain loop (waves, LDS counters and
the two shapes of the kernel do not exist here; an emulated run takes a second per instance and 5 000 samples), so the geometry
runs at N = 2 or 3 with every bin count and every signal once and not crossed, the paths at N = 4 over T = 460 and the
two-output model at N = 2 over T = 1000.
test_gpu_measurement_histogram.py runs the full shapes."""
import pytest

import histogram_ref as HR

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")

_MK = {}


def mk_for(lib):
    """one maker per library, so that histogram_ref's shared plain runs are shared"""
    if id(lib) not in _MK:
        def mk(model, n, **kw):
            from acme_jl_amd.runner import ModelRunner
            return ModelRunner(model, n, lib=lib, **kw)
        _MK[id(lib)] = mk
    return _MK[id(lib)]


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
def test_exact_pins(emu_lib):
    HR.check_exact_pins(mk_for(emu_lib))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, name, mode", [(1, "sine", "abs"), (2, "alternating", "signed"), (63, "noise", "signed"),
                                           (64, "constant", "abs"), (65, "missed ranges", "signed"), (1000, "sine", "signed"),
                                           (4096, "noise", "abs")])
def test_geometry(emu_lib, B, name, mode):
    """every bin count and every signal, paired, one mode each (the GPU file crosses them): the window of the GPU file for one
    pair of instances, a window of 600 samples for the others"""
    if (B, name) == (63, "noise"):
        HR.check_geometry(mk_for(emu_lib), 2, B, name, modes=(mode,))
    else:
        HR.check_geometry(mk_for(emu_lib), 3, B, name, T=700, length=600, cuts=(200, 450), modes=(mode,))


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [[1], None])
def test_two_outputs(emu_lib, rows):
    HR.check_geometry(mk_for(emu_lib), 2, 65, "sine", T=1000, length=600, rows=rows, two=True, cuts=(400, 650))


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
class HostDevice:
    """the emulator's "device memory" is host memory"""

    def put(self, a):
        import numpy as np
        return np.ascontiguousarray(a)

    def run(self, r, u, keep, T):
        import numpy as np
        from acme_jl_amd.runner import ModelRunner
        y = np.zeros((r.n, T, r.model.ny)) if keep else None
        ModelRunner.run_device(r, u.ctypes.data, y.ctypes.data if keep else 0, T)
        return y


@pytest.mark.parametrize("k, B, mode, weighted", [(1, 64, "signed", False), (1, 1000, "abs", False), (3, 65, "signed", False),
                                                  (1, 63, "signed", True)])
def test_paths_are_identical(emu_lib, monkeypatch, k, B, mode, weighted):
    HR.check_paths(mk_for(emu_lib), HostDevice(), k, 460, monkeypatch, B, mode, weighted, N=4)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_coexists_with_fold_spectrum_cross_target_and_ensemble(emu_lib):
    HR.check_coexistence(mk_for(emu_lib), 5, 400)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_life_cycle(emu_lib):
    HR.check_life_cycle(mk_for(emu_lib))


def test_set_matrices_carries_the_histogram(emu_lib):
    HR.check_set_matrices_carries_the_histogram(mk_for(emu_lib))


def test_refusals(emu_lib):
    HR.check_errors(mk_for(emu_lib))


def test_one_counter_beyond_the_cap_is_refused(emu_lib):
    HR.check_cap(mk_for(emu_lib), 65536, accept=False)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def test_a_non_finite_instance_counts_in_nan_alone(emu_lib):
    HR.check_nan_instance(mk_for(emu_lib))


# ---- 9 ------------------------------------------------------------------------------------------------------------------------
def test_clipper_over_its_levels(emu_lib):
    HR.check_use_level(mk_for(emu_lib))


def test_measurement_histogram_object(emu_lib):
    HR.check_object(mk_for(emu_lib))
