"""The measurement ensemble (acme_batch_set_measurement_ensemble) on the CPU wave emulator: per-sample statistics across the
instances of a group, every chain against numpy on the stored y of an identical run without an ensemble, bit for bit
(ensemble_ref).

1. exact pins   2. geometry (window, stride, split calls)   3. groups   4. rows   5. paths   6. coexistence   7. a real circuit
8. life cycle and refusals   9. a non-finite instance

The window, the strides and T are those of the GPU file.  The instance counts are not where an emulated run is slow: the
emulator walks every (group, row, slot) as a plain loop (waves, the members' loads in flight and the two shapes of the kernel do
not exist here), so the geometry runs at N = 4 (N = 6 with the blocks scaled to 1, 2, 1 and 1 members), every stride and every
grouping once and not crossed (an emulated run of 9 000 samples takes a second per instance), the paths at N = 6 over T = 460
(no call reaches a chunk boundary there: the slices of 150 and the chunks of one tile are what puts a chunk's first sample at
every phase of the stride) and the two-output model at N = 2 over T = 1000.  test_gpu_measurement_ensemble.py runs the full
shapes and MultiDeviceRunner."""
import numpy as np
import pytest

import ensemble_ref as ER

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")

_MK = {}


def mk_for(lib):
    """one maker per library, so that ensemble_ref's shared plain runs are shared"""
    if id(lib) not in _MK:
        def mk(model, n, **kw):
            from acme_jl_amd.runner import ModelRunner
            return ModelRunner(model, n, lib=lib, **kw)
        _MK[id(lib)] = mk
    return _MK[id(lib)]


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
def test_exact_pins(emu_lib):
    ER.check_exact_pins(mk_for(emu_lib))


# ---- 2, 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride, case", [(1, "one group"), (3, "interleaved"), (64, "blocks"), (4097, "one member each")])
def test_geometry_and_groups(emu_lib, stride, case):
    """every stride and every grouping, paired (the GPU file crosses them)"""
    assert ER.check_geometry(mk_for(emu_lib), 6 if case == "blocks" else 4, stride, case) == ER.slots(ER.LENGTH, stride)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [[1], None])
def test_two_outputs(emu_lib, rows):
    ER.check_geometry(mk_for(emu_lib), 2, 3, "one member each", T=1000, length=600, rows=rows, two=True, cuts=(400, 650))
    ER.check_geometry(mk_for(emu_lib), 2, 1, "one group", T=1000, length=600, rows=rows, two=True, cuts=(400, 650))


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


@pytest.mark.parametrize("k, stride, weighted", [(1, 1, False), (1, 3, False), (1, 64, False), (3, 3, False), (1, 3, True)])
def test_paths_are_bit_identical(emu_lib, monkeypatch, k, stride, weighted):
    ER.check_paths(mk_for(emu_lib), HostDevice(), k, 460, monkeypatch, stride, weighted, N=6)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_coexists_with_fold_spectrum_cross_and_target(emu_lib):
    ER.check_coexistence(mk_for(emu_lib), 5, 400)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def test_band_of_the_clipper_over_its_levels(emu_lib):
    ER.check_use_level(mk_for(emu_lib))


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
def test_life_cycle(emu_lib):
    ER.check_life_cycle(mk_for(emu_lib))


def test_set_matrices_carries_the_ensemble(emu_lib):
    ER.check_set_matrices_carries_the_ensemble(mk_for(emu_lib))


def test_refusals(emu_lib):
    ER.check_errors(mk_for(emu_lib))


# ---- 9 ------------------------------------------------------------------------------------------------------------------------
def test_a_non_finite_instance_reads_nan_in_its_group_alone(emu_lib):
    ER.check_nan_instance(mk_for(emu_lib))


def test_two_non_finite_members_the_last_one_keeps_the_indices(emu_lib):
    ER.check_two_nan_members(mk_for(emu_lib))


def test_measurement_ensemble_object(emu_lib):
    from acme_jl_amd.runner import MeasurementEnsemble
    import exact_ref as X
    from helpers import FS
    N, T = 5, 8
    u = np.ones((N, T, 1)) * np.array([1.0, 2.0, 3.0, 6.0, -4.0])[:, None, None]
    r = mk_for(emu_lib)(X.wire_model(1, FS), N).set_measurement(length=T).set_measurement_ensemble([0, 0, 0, 0, 1], 3, stride=2)
    r.measure(u, time_major=True)
    e = r.measurement_ensemble()
    assert e.filled == 4 and e.stride == 2 and e.rows == (0,) and e.sum.shape == (3, 1, 4) and e.members.tolist() == [4, 1, 0]
    assert e.sum[:2, 0, 0].tolist() == [12.0, -4.0] and e.sumsq[:2, 0, 0].tolist() == [50.0, 16.0]
    assert e.mean()[:2, 0, 1].tolist() == [3.0, -4.0] and np.isnan(e.mean()[2]).all()
    assert e.std()[0, 0].tolist() == [np.sqrt(3.5)] * 4 and e.std(ddof=1)[0, 0, 0] == np.sqrt(14.0 / 3.0) and e.std()[1, 0, 0] == 0.0
    lo, hi = e.band()
    assert lo[0, 0].tolist() == [1.0] * 4 and hi[0, 0].tolist() == [6.0] * 4 and e.argmax[0, 0].tolist() == [3] * 4
    lo, hi = e.band(sigmas=2)
    assert lo[0, 0, 0] == 3.0 - 2 * np.sqrt(3.5) and hi[0, 0, 0] == 3.0 + 2 * np.sqrt(3.5)
    assert e.trace(1).tolist() == [[-4.0] * 4]
    for g in (0, 2):
        with pytest.raises(ValueError, match="one-member"):
            e.trace(g)
    # joined by group: shard 0 holds groups 0 and 2 (empty), shard 1 group 1; the indices move by the shard's first instance
    a = MeasurementEnsemble(e.sum, e.sumsq, e.min, e.max, e.argmin, e.argmax, [4, 0, 0], 4, 2, (0,))
    fill = lambda v, dt=np.float64: np.full((3, 1, 4), v, dtype=dt)
    b = MeasurementEnsemble(fill(0.0), fill(0.0), fill(np.inf), fill(-np.inf), fill(-1, np.int64), fill(-1, np.int64), [0, 1, 0], 4, 2, (0,))
    b.sum[1], b.sumsq[1], b.min[1], b.max[1], b.argmin[1], b.argmax[1] = -4.0, 16.0, -4.0, -4.0, 0, 0
    j = MeasurementEnsemble.join([a, b], [0, 4])
    assert j.members.tolist() == [4, 1, 0] and np.array_equal(j.sum, e.sum) and np.array_equal(j.argmin, e.argmin)
    assert (j.argmax[1] == 4).all() and (j.argmax[2] == -1).all()
    with pytest.raises(ValueError, match="group 0"):
        MeasurementEnsemble.join([a, a], [0, 4])
