"""PULSE and BURST rows (acme_batch_set_source_pulse / _burst, csrc/acme_source.h) on the MI355X: the HIP kernels' PULSE rows against
pulse_ref bit for bit at every clock -- which is also the emulator-against-GPU statement in its strongest form --, BURST rows ==
the SINE row rendered beside them where the envelope is 1, == the offset where it is 0 and within source_ref.sine_bound of mpmath
on the ramps, the render's independence of the layout, both new instantiations next to the other kinds, the defining property of
the sources at small width in every mode and with oversampling, and the rows under an events measurement in closed form.  The
checks are test_pulse_sources.py's, run with the product library."""
import numpy as np
import pytest

import pulse_ref as pr
import source_ref as sr
import test_pulse_sources as tp
from test_gpu_sources import TorchArrays
from test_sources import MODES

pytestmark = pytest.mark.gpu


def runner(model, n, **kw):
    from acme_jl_amd.runner import ModelRunner
    return ModelRunner(model, n, device=0, **kw)


# ---- exact rows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clock", sr.CLOCKS)
def test_gpu_a_pulse_row_is_the_exact_one(hip_lib, clock):
    tp.check_exact_pulse(runner, clock)


@pytest.mark.parametrize("clock", [0, 2 ** 31 + 1, 2 ** 62])
def test_gpu_a_burst_row_is_the_sine_row_under_its_envelope(hip_lib, clock):
    tp.check_burst(runner, clock, "MI355X")


# ---- layout independence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds", ["1", "0"])
@pytest.mark.parametrize("nu", [1, 2, 3, 4, 5, 6])
def test_gpu_every_store_shape(hip_lib, monkeypatch, nu, lds):
    tp.check_every_store_shape(runner, monkeypatch, nu, lds)


def test_gpu_a_long_launch_and_split_renders(hip_lib, monkeypatch):
    tp.check_long_and_split_renders(runner, monkeypatch)


def test_gpu_a_render_from_a_clock_is_the_tail_of_an_earlier_one(hip_lib):
    tp.check_tail_renders(runner)


def test_gpu_next_to_the_other_kinds(hip_lib):
    tp.check_next_to_the_other_kinds(runner, 6, 4096 + 603, 2 ** 40 + 1)


# ---- the defining property, small width, every mode ---------------------------------------------------------------------------------
T_GPU = 2 * 4096 + 700          # three slices of run_os
SCALE = 100                     # the envelopes of pulse_ref.property_cases stretched to this length: bursts of 4 000 samples


@pytest.mark.parametrize("mode", range(len(MODES)))
@pytest.mark.parametrize("case", range(2))
def test_gpu_a_source_run_is_a_run_on_the_rendered_input(hip_lib, case, mode):
    name, m, N, kinds = pr.property_cases(scale=SCALE, clock=tp.PROP_CLOCK)[case]
    md = dict(MODES[mode])
    if md.get("split"):
        md["split"] = 4096 + 1234          # (the cut inside the second slice, on the pot's ramp)
    u = pr.check_defining_property(hip_lib, m, N, kinds, None, T_GPU, more=4096 + 77, clock=tp.PROP_CLOCK, arrays=TorchArrays(), **md)
    assert np.abs(u[:, :, 0]).max() > 1e-2 and np.isfinite(u).all()
    if case == 1:
        assert (u[:, :5, 2] == 0.25).all() and (np.diff(u[:, 5:5000, 2], axis=1) > 0).all()


@pytest.mark.parametrize("mode", [dict(mem=0, keep=True, split=4096 + 1234), dict(mem=1, keep=False)], ids=["host-split", "device-measured"])
@pytest.mark.parametrize("held", [False, True])
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("case", range(2))
def test_gpu_oversampled_source_runs(hip_lib, case, k, held, mode):
    name, m, N, kinds = pr.property_cases(scale=SCALE)[case]
    rows = [r for r, kd in enumerate(kinds) if kd["kind"] != "const"] if held else []
    pr.check_defining_property(hip_lib, m, N, kinds, None, T_GPU, k=k, held=rows, more=300, arrays=TorchArrays(), **mode)


# ---- with the forms it serves -------------------------------------------------------------------------------------------------------
def test_gpu_a_pulse_under_an_events_measurement(hip_lib):
    tp.check_pulse_under_events(runner)


def test_gpu_an_edge_time_sweep(hip_lib):
    tp.check_edge_time_sweep(runner)
