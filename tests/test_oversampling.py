"""Oversampled runs (acme_batch_set_oversampling) on the CPU wave emulator: the default lowpass against its stated spec,
the plumbing bit for bit against a plain run at the model rate, the filters against a numpy composition, and the
bit-identity of split calls, run_const and switching the factor off."""
from fractions import Fraction

import numpy as np
import pytest

from helpers import FS, HS, RTOL, assert_close, beyond_the_tuned_shapes, load, mid_size_models, sine, sweep_inputs

PASSBAND_RIPPLE = 1e-4          # |H(f)| within 1 +- 1e-4 up to 0.40 fs_base (stated in include/acme_hip.h)


def runner(model, n, lib, **kw):
    from acme_jl_amd.runner import ModelRunner
    return ModelRunner(model, n, lib=lib, **kw)


def np_interpolate(u, k, g, held=()):
    """u [N, T, nu] -> [N, kT, nu] by the header's formula: zero-stuffed rows filtered with g (= k h_up), held rows
    repeated; the past of every row is its first sample"""
    N, T, nu = u.shape
    out = np.empty((N, k * T, nu))
    D = (len(g) - 1) // k
    for r in range(nu):
        if r in held:
            out[:, :, r] = np.repeat(u[:, :, r], k, axis=1)
            continue
        ext = np.concatenate([np.repeat(u[:, :1, r], D, axis=1), u[:, :, r]], axis=1)
        s = np.zeros((N, k * (T + D)))
        s[:, ::k] = ext
        acc = np.zeros_like(s)
        for j, gj in enumerate(g):
            acc[:, j:] += gj * s[:, :s.shape[1] - j]
        out[:, :, r] = acc[:, k * D:]
    return out


def np_decimate(y_os, k, h):
    """y_os [N, kT, ny] -> [N, T, ny]: y[n] = sum_j h[j] y_os[nk + k - 1 - j], the past being the first sample"""
    P = len(h) - 1
    ext = np.concatenate([np.repeat(y_os[:, :1], P, axis=1), y_os], axis=1)
    T = y_os.shape[1] // k
    m = np.arange(T) * k + k - 1 + P
    return sum(hj * ext[:, m - j] for j, hj in enumerate(h))


def clipper_176k():
    from acme_jl_amd import examples
    from acme_jl_amd.model import DiscreteModel
    return DiscreteModel(examples.diodeclipper(), Fraction(1, 4 * FS), HS)


def birdie_u(N, T):
    return np.ascontiguousarray(sweep_inputs("birdie_var", N, T).transpose(0, 2, 1))      # [N][T][2], vol in row 1


# ---- 1. the default design ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 4, 8])
def test_default_design_meets_its_spec(emu_lib, k):
    from acme_jl_amd.runner import design_oversampling_filter
    h = design_oversampling_filter(k, emu_lib)
    L = len(h)
    assert L % 2 == 1 and (L - 1) % k == 0, L
    assert np.array_equal(h, h[::-1])
    assert abs(h.sum() - 1.0) < 1e-12
    nfft = 1 << 18
    H = np.abs(np.fft.rfft(h, nfft))
    f = np.arange(len(H)) / nfft * k            # in units of the base rate
    assert 20 * np.log10(H[f >= 0.5].max()) <= -80.0
    assert np.abs(H[f <= 0.4] - 1.0).max() <= PASSBAND_RIPPLE
    # the same taps as the ABI hands out directly, and the delay the runner reports
    r = runner(clipper_176k(), 1, emu_lib)
    r.set_oversampling(k)
    assert r.oversampling_delay == (L - 1) // k


# ---- 2. the plumbing, bit for bit --------------------------------------------------------------------------------------
def plumbing_cases():
    mid = mid_size_models()[0]
    gen = [c for c in beyond_the_tuned_shapes() if c[0] == "9 sub-problems"][0]
    return [("birdie_var_176k", load("birdie_var_176k", "HomotopySolver{SimpleSolver}"), birdie_u(4, 24), "tuned"),
            ("diode clipper 176.4 kHz", clipper_176k(), np.logspace(-2, 1, 5)[:, None, None] * sine(30)[None, :, None], "tuned"),
            (mid[0], mid[1], np.ascontiguousarray(mid[2][:, :, :16].transpose(0, 2, 1)), "coop"),
            (gen[0], gen[1], np.ascontiguousarray(gen[2][:, :, :12].transpose(0, 2, 1)), "generic")]


@pytest.mark.parametrize("case", range(4))
def test_held_rows_and_a_unit_decimator_are_a_plain_run_at_the_model_rate(emu_lib, case):
    name, m, u, family = plumbing_cases()[case]
    k = 3 if case == 3 else 4
    N = u.shape[0]
    ref = runner(m, N, emu_lib)
    assert ref.batch_kernel_variant()[1] == family, name
    y_os = ref.run(np.repeat(u, k, axis=1), time_major=True)
    r = runner(m, N, emu_lib)
    r.set_oversampling(k, down=[1.0], held_rows=range(m.nu))
    y = r.run(u, time_major=True)
    assert y.shape == (N, u.shape[1], m.ny)
    assert np.array_equal(y, y_os[:, k - 1::k]), name
    # the reports count model-rate samples
    assert np.array_equal(r.report_arrays()["iters_total"], ref.report_arrays()["iters_total"])


# ---- 3. the filters against numpy ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["birdie_var_176k", "clipper"])
def test_filtered_run_matches_a_numpy_composition(emu_lib, which):
    from acme_jl_amd.runner import design_oversampling_filter
    k = 4
    if which == "clipper":
        m, u, held = clipper_176k(), 2.0 * np.array([0.3, 1.0, 3.0])[:, None, None] * sine(90, f=3000.0)[None, :, None], ()
    else:
        m, u, held = load(which, "HomotopySolver{SimpleSolver}"), birdie_u(3, 90), (1,)
    h = design_oversampling_filter(k, emu_lib)
    r = runner(m, u.shape[0], emu_lib)
    r.set_oversampling(k, held_rows=held)
    y = r.run(u, time_major=True)
    y_os = runner(m, u.shape[0], emu_lib).run(np_interpolate(u, k, k * h, held), time_major=True)
    assert_close(y, np_decimate(y_os, k, h), RTOL)
    assert np.abs(y).max() > 1e-3


# ---- 4. split calls, run_const, device memory, switching off --------------------------------------------------------------
@pytest.mark.parametrize("t1", [1, 37, 4096])
def test_split_calls_are_one_call(emu_lib, t1):
    m = clipper_176k()
    T = t1 + 45
    u = np.ascontiguousarray((np.array([0.5, 4.0])[:, None] * sine(T, f=2500.0)[None])[:, :, None])
    one = runner(m, 2, emu_lib).set_oversampling(4)
    y1 = one.run(u, time_major=True)
    two = runner(m, 2, emu_lib).set_oversampling(4)
    a = two.run(np.ascontiguousarray(u[:, :t1]), time_major=True)
    b = two.run(np.ascontiguousarray(u[:, t1:]), time_major=True)
    assert np.array_equal(y1, np.concatenate([a, b], axis=1))


def test_slices_device_memory_and_run_const_are_bit_identical(emu_lib, monkeypatch):
    from acme_jl_amd.runner import ModelRunner
    m = load("birdie_var_176k", "HomotopySolver{SimpleSolver}")
    u = birdie_u(3, 50)
    r = runner(m, 3, emu_lib).set_oversampling(4, held_rows=[1])
    y = r.run(u, time_major=True)
    # time slices of 7 base-rate samples (the histories carried across every boundary)
    monkeypatch.setenv("ACME_OS_SLICE", "7")
    rs = runner(m, 3, emu_lib).set_oversampling(4, held_rows=[1])
    assert np.array_equal(rs.run(u, time_major=True), y)
    # "device" memory (the emulator's device is host memory) through the device path's slices
    rd = runner(m, 3, emu_lib).set_oversampling(4, held_rows=[1])
    yd = np.zeros_like(y)
    ModelRunner.run_device(rd, u.ctypes.data, yd.ctypes.data, u.shape[1])
    assert np.array_equal(yd, y)
    monkeypatch.delenv("ACME_OS_SLICE")
    # run_const: the constant rows are held whatever held_rows says
    rc = runner(m, 3, emu_lib).set_oversampling(4)
    yc = rc.run_const(np.ascontiguousarray(u[:, :, :1]), np.ascontiguousarray(u[:, 0, :]), [1])
    assert np.array_equal(yc, y)


def test_factor_one_after_four_is_a_fresh_batch(emu_lib):
    m = clipper_176k()
    u = np.ascontiguousarray((np.array([0.5, 4.0])[:, None] * sine(40)[None])[:, :, None])
    r = runner(m, 2, emu_lib)
    r.set_oversampling(4)
    r.set_oversampling(1)
    assert r.oversampling == 1 and r.oversampling_delay == 0
    assert np.array_equal(r.run(u, time_major=True), runner(m, 2, emu_lib).run(u, time_major=True))


def test_histories_continue_across_set_state_and_restart_after_set_oversampling(emu_lib):
    m = clipper_176k()
    u = np.ascontiguousarray((np.array([0.5, 4.0])[:, None] * sine(60, f=2000.0)[None])[:, :, None])
    r = runner(m, 2, emu_lib).set_oversampling(4)
    y_first = r.run(u, time_major=True)
    x, p, z = r.get_state()
    r.set_oversampling(4)            # the histories restart: the first sample extends into the past again
    r.set_state(*runner(m, 2, emu_lib).get_state())
    assert np.array_equal(r.run(u, time_major=True), y_first)
    # set_state leaves the histories alone: the continuation is not a restart
    r2 = runner(m, 2, emu_lib).set_oversampling(4)
    r2.run(u, time_major=True)
    r2.set_state(*runner(m, 2, emu_lib).get_state())
    assert not np.array_equal(r2.run(u, time_major=True), y_first)


# ---- 5. argument errors --------------------------------------------------------------------------------------------------
def test_argument_errors_and_the_default_taps(emu_lib):
    import ctypes as C
    from acme_jl_amd.runner import AcmeError, design_oversampling_filter
    m = load("birdie_var_176k", "HomotopySolver{SimpleSolver}")
    r = runner(m, 2, emu_lib)
    for factor in (0, 17):
        with pytest.raises(AcmeError, match="factor"):
            r.set_oversampling(factor)
    with pytest.raises(AcmeError, match="taps"):
        r.set_oversampling(4, up=[])
    with pytest.raises(AcmeError, match="held row"):
        r.set_oversampling(4, held_rows=[2])
    with pytest.raises(AcmeError, match="factor"):
        design_oversampling_filter(0, emu_lib)
    # NULL taps: the default design, both ways
    h = design_oversampling_filter(4, emu_lib)
    u = birdie_u(2, 20)
    y_default = r.set_oversampling(4, held_rows=[1]).run(u, time_major=True)
    y_given = runner(m, 2, emu_lib).set_oversampling(4, up=h, down=h, held_rows=[1]).run(u, time_major=True)
    assert np.array_equal(y_default, y_given)
    # the design call with too small a buffer only reports the length
    buf = np.full(3, 7.0)
    assert emu_lib.L.acme_oversampling_design(4, buf.ctypes.data_as(C.POINTER(C.c_double)), 3) == len(h)
    assert (buf == 7.0).all()
    assert emu_lib.L.acme_oversampling_design(1, None, 0) == 1
