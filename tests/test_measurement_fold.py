"""The measurement fold (acme_batch_set_measurement_fold, synchronous averaging) on the CPU wave emulator: the window folded
onto one period per instance, every slot against numpy on the stored y of an identical run without a fold, bit for bit
(fold_ref).

1. period geometry   2. per-instance periods   3. rows   4. paths (what the emulator has)   5. the three forms
6. exact pins on the pass-through model   8. life cycle, errors, a batch without a fold is what it was

The periods, start and T are those of the GPU file.  The instance counts are not: an emulated run of the diode clipper at
N = 131, T = 9000 takes 14 s, so the geometry runs at N = 3 (two outputs: N = 2) -- the emulator walks the pairs one by one,
a wave per pair does not exist here --; the per-instance periods and the forms, whose N the cases fix at 130 and 131, run the
pass-through model (the periods over T = 120 from start = 3, three of the distinct periods against their shared fold; the
forms over T = 460 with the periods 1, 5, 63, 64, 65 and 441 shared out among them, 441 with each); the paths run the
pass-through model, N = 6 over T = 460 from start = 3, at each of the periods 1, 5, 63, 64, 65 and 441 (oversampled by 3, which takes 17 s a case here, at 5 and 441 only; no call reaches a
chunk boundary there: the slices of 150 and the chunks of one tile are what puts a chunk's first sample at every phase), and
the diode clipper, N = 6 over T = 2100, at P = 441; the exact pin runs over T = 2037 without the long lead, and the case at the cap (N = 3 over T = 140 000: two minutes here)
is the GPU file's; that the cap itself is accepted is part of the argument errors.  test_gpu_measurement_fold.py runs the full shapes and the use-level check."""
import numpy as np
import pytest

import fold_ref as FR


_MK = {}


def mk_for(lib):
    """one maker per library, so that fold_ref's shared plain runs are shared"""
    if id(lib) not in _MK:
        def mk(model, n, **kw):
            from acme_jl_amd.runner import ModelRunner
            return ModelRunner(model, n, lib=lib, **kw)
        _MK[id(lib)] = mk
    return _MK[id(lib)]


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", FR.GEOMETRY)
def test_period_geometry(emu_lib, P):
    FR.check_geometry(mk_for(emu_lib), 3, 9000, 301, 10, P)


def test_the_last_slot_receives_one_sample(emu_lib):
    got, count = FR.check_geometry(mk_for(emu_lib), 3, 9000, 301, 10, 8699)
    assert count == 8699 and not np.isnan(got[1]).any()


def test_slots_no_sample_reaches_read_nan(emu_lib):
    got, count = FR.check_geometry(mk_for(emu_lib), 3, 9000, 301, 10, 9000)
    assert np.isnan(got[1][:, :, count:]).all() and not np.isnan(got[1][:, :, :count]).any()


def test_a_bounded_window(emu_lib):
    assert FR.check_geometry(mk_for(emu_lib), 3, 9000, 301, 10, 441, length=2000)[1] == 2000


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FR.period_cases()))
def test_per_instance_periods(emu_lib, name):
    FR.check_per_instance(mk_for(emu_lib), FR.period_cases()[name], 120, start=3, wire=True, shared=3)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [[1], None])
def test_two_outputs(emu_lib, rows):
    FR.check_geometry(mk_for(emu_lib), 2, 1000, 301, 10, 65, rows=rows, two=True)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
class HostDevice:
    """the emulator's "device memory" is host memory"""

    def put(self, a):
        return np.ascontiguousarray(a)

    def run(self, r, u, keep, T):
        from acme_jl_amd.runner import ModelRunner
        y = np.zeros((r.n, T, r.model.ny)) if keep else None
        ModelRunner.run_device(r, u.ctypes.data, y.ctypes.data if keep else 0, T)
        return y


@pytest.mark.parametrize("k", [1, 3])
def test_paths_are_bit_identical(emu_lib, monkeypatch, k):
    FR.check_paths(mk_for(emu_lib), HostDevice(), k, 2100, monkeypatch, N=6)


@pytest.mark.parametrize("k, P", [(1, 1), (1, 5), (1, 63), (1, 64), (1, 65), (1, 441), (3, 5), (3, 441)])
def test_paths_are_bit_identical_on_the_pass_through_model(emu_lib, monkeypatch, k, P):
    FR.check_paths(mk_for(emu_lib), HostDevice(), k, 460, monkeypatch, N=6, P=P, S=3, wire=True)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form, periods", [("shared", [1, 64, 441]), ("per instance", [5, 63, 441]), ("bins", [65, 441])])
def test_all_three_forms_carry_a_fold(emu_lib, form, periods):
    FR.check_forms(mk_for(emu_lib), 460, periods, wire=True, forms=[form])


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_exact_chain_order(emu_lib):
    FR.check_exact(mk_for(emu_lib), 7, 300, 2037)


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
def test_life_cycle(emu_lib):
    FR.check_life_cycle(mk_for(emu_lib))


def test_set_matrices_carries_the_fold(emu_lib):
    FR.check_set_matrices_carries_the_fold(mk_for(emu_lib))


def test_argument_errors(emu_lib):
    FR.check_errors(mk_for(emu_lib))


def test_a_batch_without_a_fold_is_unchanged(emu_lib):
    FR.check_no_fold_invariance(mk_for(emu_lib), 67, 300)


def test_measurement_fold_object(emu_lib):
    from acme_jl_amd.runner import MeasurementFold
    import exact_ref as X
    from helpers import FS
    N, T, P = 4, 100, np.array([8, 8, 5, 8])
    n = np.arange(T)
    u = (1.5 + np.cos(2 * np.pi * n / 8) + 0.25 * np.sin(2 * np.pi * 3 * n / 8))[None, :, None] * np.ones((N, 1, 1))
    r = mk_for(emu_lib)(X.wire_model(1, FS), N).set_measurement(start=4, length=80).set_measurement_fold(P)
    r.measure(u, time_major=True)
    f = r.measurement_fold()
    assert f.count == 80 and f.period.tolist() == P.tolist() and f.rows == (0,) and f.mean.shape == (N, 1, 8)
    assert f.slot_counts(0).tolist() == [10] * 8 and f.slot_counts(2).tolist() == [16] * 5
    a = f.spectrum(0)                                       # the window starts at m = 0 <-> n = 4: half a period of line 1
    assert np.allclose(a, [1.5, -1.0, 0, 0.25j * np.exp(-2j * np.pi * 3 * 4 / 8) * -1, 0], atol=1e-14)
    both = MeasurementFold.concatenate([f, f])
    assert both.mean.shape == (2 * N, 1, 8) and both.period.tolist() == P.tolist() * 2 and both.count == 80
    with pytest.raises(ValueError, match="differ"):         # shards that disagree in count or rows do not concatenate
        MeasurementFold.concatenate([f, MeasurementFold(f.mean, f.period, 79, f.rows)])
    sums = r.measurement_fold(raw=True).mean                # the sums getter: the means times the slots' counts, before rounding
    assert np.array_equal(sums[0, 0] / f.slot_counts(0), f.mean[0, 0])
    assert r.lib.L.acme_batch_get_measurement_fold_sums(r.h, None) == -1 and "out" in r.lib.L.acme_last_error().decode()
