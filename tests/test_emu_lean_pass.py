"""The condensed Newton loop's lean and general bookkeeping paths on the CPU wave emulator (tests/emu): waves that hold
instances of both kinds, independence from the wave-mates' path, the exit by maxiter, split launches.  The cases and
their bars are lean_pass_cases.py's; test_gpu_lean_pass.py runs the same ones on the device."""
import lean_pass_cases as cases


def test_emulated_mixed_waves(emu_lib):
    cases.check_mixed_waves(emu_lib)


def test_emulated_wave_mate_independence(emu_lib):
    cases.check_wave_mates(emu_lib)


def test_emulated_exit_by_maxiter(emu_lib):
    cases.check_maxiter(emu_lib)


def test_emulated_split_launches(emu_lib):
    cases.check_split_launches(emu_lib)
