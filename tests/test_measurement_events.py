"""The measurement events (acme_batch_set_measurement_events) on the CPU wave emulator: the level crossings of every (instance,
row, level) triple, every integer and every copied value against the contract's sequential loop on the stored y of an identical
run without events (events_ref), ``==`` throughout.

1. hand-listed pins   2. geometry (window, split calls, signals, exactly E and E + 1 events)   3. rows   4. paths
5. coexistence   6. life cycle, refusals, the cap, two shards   7. a circuit

Both walks of the non-HIP backend run: ``chain``, the contract's loop (the default), and ``mask`` (ACME_EVENTS_WALK=mask), the
rounds of 64 samples through meas_events_masks and meas_events_slot -- the algebra and the slot logic the GPU kernel runs, with a
loop in place of the two ballots.  The window, the levels and the slots are those of the GPU file; an emulated run takes a
second per instance and 5 000 samples, so the geometry runs at N = 3 with every signal, every C and every E once and not
crossed (the full window for one of them), the paths at N = 4 over T = 460 and the two-output model at N = 2 over T = 1000.
test_gpu_measurement_events.py runs the full shapes."""
import numpy as np
import pytest

import events_ref as ER

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")

_MK = {}
WALKS = ["chain", "mask"]


def mk_for(lib):
    """one maker per library, so that events_ref's shared plain runs and replays are shared"""
    if id(lib) not in _MK:
        def mk(model, n, **kw):
            from acme_jl_amd.runner import ModelRunner
            return ModelRunner(model, n, lib=lib, **kw)
        _MK[id(lib)] = mk
    return _MK[id(lib)]


@pytest.fixture(params=WALKS)
def walk(request, monkeypatch):
    monkeypatch.setenv("ACME_EVENTS_WALK", request.param)
    return request.param


# ---- the algebra itself ---------------------------------------------------------------------------------------------------------
def test_the_reference_loops_agree():
    """the replay that carries the step across the triples with numpy == the rule in plain Python floats, triple by triple"""
    rng = np.random.default_rng(1)
    yw = rng.uniform(-1.0, 1.0, (3, 300, 2))
    yw[1, 100:, 0] = np.nan
    lo, hi = ER.levels2([-0.3, 0.1, 0.5], [0.3, 0.1, 0.6], 3)
    for E in (0, 2, 16):
        cnt, idx, ab = ER.replay(yw, lo, hi, E)
        for i in range(3):
            for r in range(2):
                for c in range(3):
                    one = ER.rule_loop(yw[i, :, r].tolist(), lo[c, i], hi[c, i], E)
                    assert cnt[i, r, c].tolist() == one[0] and idx[i, r, c].tolist() == one[1]
                    assert np.array_equal(ER.bits(ab[i, r, c]), ER.bits(np.array(one[2])))


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
def test_hand_listed_pins(emu_lib, walk):
    ER.check_pins(mk_for(emu_lib))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nC, E, name", [(1, 16, "alternating"), (3, 1, "noise"), (8, 0, "sine 64 then 63"), (3, 16, "constant"),
                                         (8, 1, "missed levels"), (1, 0, "noise"), (8, 16, "alternating")])
def test_geometry(emu_lib, walk, nC, E, name):
    """every signal, every C and every E, paired (the GPU file crosses them): the window of the GPU file for one case, a window
    of 600 samples for the others"""
    if (nC, name) == (3, "noise"):
        ER.check_geometry(mk_for(emu_lib), 2, nC, E, name)
    else:
        ER.check_geometry(mk_for(emu_lib), 3, nC, E, name, T=700, length=600, cuts=(200, 450))


def test_exactly_as_many_events_as_slots_and_one_more(emu_lib, walk):
    ER.check_slot_boundary(mk_for(emu_lib))


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [[1], None])
def test_two_outputs(emu_lib, walk, rows):
    ER.check_geometry(mk_for(emu_lib), 2, 3, 4, "sine 64 then 63", T=1000, length=600, rows=rows, two=True, cuts=(400, 650))


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


@pytest.mark.parametrize("k, nC, E, weighted", [(1, 3, 4, False), (3, 1, 16, False), (1, 8, 1, True)])
def test_paths_are_identical(emu_lib, walk, monkeypatch, k, nC, E, weighted):
    ER.check_paths(mk_for(emu_lib), HostDevice(), k, 460, monkeypatch, nC, E, weighted, N=4)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_coexists_with_every_other_form(emu_lib, walk):
    ER.check_coexistence(mk_for(emu_lib), 5, 400)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_life_cycle(emu_lib, walk):
    ER.check_life_cycle(mk_for(emu_lib))


def test_set_matrices_carries_the_events(emu_lib):
    ER.check_set_matrices_carries_the_events(mk_for(emu_lib))


def test_refusals(emu_lib):
    ER.check_errors(mk_for(emu_lib))


def test_one_record_beyond_the_cap_is_refused(emu_lib):
    ER.check_cap(mk_for(emu_lib), accept=False)


def test_two_shards_equal_the_single_runner(emu_lib):
    from acme_jl_amd.runner import MultiDeviceRunner
    ER.check_two_shards(lambda m, n: MultiDeviceRunner(m, n, devices=[0, 0], lib=emu_lib), mk_for(emu_lib), N=5, T=1000)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def test_clipper_frequency_and_duty(emu_lib, walk):
    ER.check_circuit(mk_for(emu_lib), N=4, periods=24)


def test_measurement_events_object(emu_lib):
    ER.check_object(mk_for(emu_lib))
