"""The condensed Newton loop's lean and general bookkeeping paths on the device (pytest -m gpu): waves that hold
instances of both kinds, independence from the wave-mates' path, the exit by maxiter, split launches.  The cases and
their bars are lean_pass_cases.py's; test_emu_lean_pass.py runs the same ones on the CPU wave emulator."""
import pytest

import lean_pass_cases as cases

pytestmark = pytest.mark.gpu


def test_mixed_waves(hip_lib):
    cases.check_mixed_waves(hip_lib)


def test_wave_mate_independence(hip_lib):
    cases.check_wave_mates(hip_lib)


def test_exit_by_maxiter(hip_lib):
    cases.check_maxiter(hip_lib)


def test_split_launches(hip_lib):
    cases.check_split_launches(hip_lib)
