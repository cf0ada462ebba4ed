"""The measurement events (acme_batch_set_measurement_events) on the MI355X: acme_meas_events_kernel itself -- a wave per
pair, rounds of 64 consecutive samples and their ragged end, the two ballots per level, the neighbour exchange (DPP wave_shr:1,
lane 0 from the round before or the carry), the per-level registers kept in lane c and read by v_readlane, the event lanes'
slot stores, the carries from chunk to chunk.  The ballots, the neighbour exchange, the slot stores and the carries run as
written ONLY here: the CPU emulator walks loops (its mask walk shares the mask algebra and the slot rule, no more).  Every
integer and every copied value against the contract's sequential loop on the stored y of an identical run without events,
``==`` throughout (events_ref)."""
import numpy as np
import pytest

import events_ref as ER

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]


def mk(model, n, **kw):
    from acme_jl_amd.runner import ModelRunner
    return ModelRunner(model, n, device=0, **kw)


# ---- 1. hand-listed pins ------------------------------------------------------------------------------------------------------
def test_gpu_hand_listed_pins(hip_lib):
    ER.check_pins(mk)


# ---- 2. geometry --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [131, 200])
@pytest.mark.parametrize("name", ER.SIGNALS)
@pytest.mark.parametrize("E", ER.SLOTS)
@pytest.mark.parametrize("nC", ER.LEVELS)
def test_gpu_geometry(hip_lib, nC, E, name, N):
    """N = 131 pairs is no multiple of the four waves of a block, and 131 and 200 both leave levels' lanes idle; the window
    has a chunk boundary inside and a ragged last round"""
    ER.check_geometry(mk, N, nC, E, name)


def test_gpu_exactly_as_many_events_as_slots_and_one_more(hip_lib):
    ER.check_slot_boundary(mk)
    ER.check_slot_boundary(mk, E=16)
    ER.check_slot_boundary(mk, E=1)


# ---- 3. rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [[1], None])
def test_gpu_two_outputs(hip_lib, rows):
    ER.check_geometry(mk, 99, 3, 4, "sine 64 then 63", rows=rows, two=True)
    ER.check_geometry(mk, 99, 8, 16, "noise", rows=rows, two=True)


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


@pytest.mark.parametrize("k, nC, E, weighted", [(1, 3, 4, False), (1, 8, 16, False), (3, 1, 16, False), (3, 3, 1, True),
                                                (1, 8, 1, True)])
def test_gpu_paths_are_identical(hip_lib, monkeypatch, k, nC, E, weighted):
    ER.check_paths(mk, TorchDevice(), k, 9000, monkeypatch, nC, E, weighted)


# ---- 5. coexistence ------------------------------------------------------------------------------------------------------------
def test_gpu_coexists_with_every_other_form(hip_lib):
    ER.check_coexistence(mk, 131, 5000)


# ---- 6. life cycle and refusals ------------------------------------------------------------------------------------------------
def test_gpu_life_cycle(hip_lib):
    ER.check_life_cycle(mk)


def test_gpu_set_matrices_carries_the_events(hip_lib):
    ER.check_set_matrices_carries_the_events(mk)


def test_gpu_refusals(hip_lib):
    ER.check_errors(mk)


def test_gpu_the_cap_is_accepted_and_one_record_more_refused(hip_lib):
    ER.check_cap(mk, accept=True)


def test_gpu_multi_device_runner_equals_the_single_runner(hip_lib):
    from acme_jl_amd.runner import MultiDeviceRunner
    ER.check_two_shards(lambda m, n: MultiDeviceRunner(m, n, devices=[0, 0]), mk)


# ---- 7. a circuit --------------------------------------------------------------------------------------------------------------
def test_gpu_clipper_frequency_and_duty(hip_lib):
    e, f, duty = ER.check_circuit(mk)
    print("frequency, relative to fs / P:", np.array2string(f / (ER.FS / 45) - 1.0, precision=2))
    print("duty at the level 0:", np.array2string(duty, precision=4))


def test_gpu_measurement_events_object(hip_lib):
    ER.check_object(mk)
