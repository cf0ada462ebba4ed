"""The resampling (csrc/acme_resample.h) and measurement (csrc/acme_measure.h) code on exactly known signals, on the CPU
wave emulator.  The model is exact_ref.wire_model -- y = u --, so an oversampled run is decimate(interpolate(u)) and a
measured run measures data chosen here; the expected values are exact_ref's, which share no code with the library.

Resampler: bit for bit against the headers' fma chains -- every factor 2 ... 16 with the default taps, tap shapes the
default design never has (1 tap, fewer taps than the factor, different counts up and down, 4096 taps, asymmetric taps),
histories longer than a slice, calls of one sample, run_const.
Measurement: sum, sq, min, max, mean and rms bit for bit; C_h and S_h within exact_ref.harmonic_bound of the mpmath value.

Thresholds: exact equality, or the derived bound (n + 16) 2^-53 sum |y_t| (exact_ref.harmonic_bound).  As a record, not a
threshold: the largest observed |error| / bound of the harmonics is 8.2e-3 on the emulator (this file; 3.7e-4 at n = 4133)
and 3.6e-4 on the MI355X (test_gpu_exact_kernels.py); one dropped sample is about 1e9 times the bound."""
import numpy as np
import pytest

import exact_ref as X
from helpers import FS
from test_measurement import raw

WIRE_FAILS = "precondition: a plain run of the wire model does not return u bit for bit -- nothing below means anything"


def runner(model, n, lib):
    from acme_jl_amd.runner import ModelRunner
    return ModelRunner(model, n, lib=lib)


def wire(lib, u, T=None):
    """the wire model for u [N, T, c], after the precondition of every test here: a plain run returns u (its first T samples:
    the emulator takes a second per thousand, and the measured runs compare their stored y in full) bit for bit"""
    m = X.wire_model(u.shape[2], FS)
    assert (m.nx, m.nn(), m.nu, m.ny) == (0, 0, u.shape[2], u.shape[2]), WIRE_FAILS
    u = np.ascontiguousarray(u[:, :T])
    y = runner(m, u.shape[0], lib).run(u, time_major=True)
    assert np.array_equal(y, u), WIRE_FAILS
    return m


def test_fma_fast_is_the_fraction_fma():
    rng = np.random.default_rng(0)
    v = (rng.standard_normal((2000, 3)) * 10.0 ** rng.integers(-12, 13, (2000, 3))).tolist()
    v += [[1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53, -1.0], [2.0 ** -537, 2.0 ** -537, 5e-324], [1e308, 1.0, -1e308],       # cancellation, subnormals,
          [3.0, 2.0 ** -53, 1.0], [1.0, 2.0 ** -53, 1.0], [0.1, 0.1, -0.010000000000000002], [0.0, 5.0, 0.0]]       # ties
    for a, b, c in v:
        assert X.fma_fast(a, b, c) == X.fma(a, b, c), (a, b, c)
    assert X.fma(0.1, 0.1, -0.010000000000000002) != 0.1 * 0.1 - 0.010000000000000002       # (one rounding, not two)


# ---- resampler ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(2, 17))
def test_every_factor_with_the_default_taps_is_the_fma_chain(emu_lib, k):
    from acme_jl_amd.runner import design_oversampling_filter
    u = X.scaled_rows(np.random.default_rng(k), 2, 23, 3)
    m = wire(emu_lib, u)
    h = design_oversampling_filter(k, emu_lib)
    y = runner(m, 2, emu_lib).set_oversampling(k, held_rows=[1]).run(u, time_major=True)
    ref = X.chain_resample(u, k, X.scaled_up_taps(k, h), h, (1,))
    assert np.array_equal(y, ref), (k, np.argwhere(y != ref)[:8])


# (k, Lu, Ld): one tap; fewer taps than k; Lu = k, k + 1 (Du = floor((Lu - 1) / k) goes 0 -> 1) and 2 k, 2 k + 1 (1 -> 2);
# one decimation tap; Lu != Ld both ways; OS_MAX_TAPS = 4096 either way
TAP_SHAPES = [(2, 1, 1), (5, 3, 2), (7, 7, 8), (7, 8, 3), (3, 6, 5), (3, 7, 5), (16, 5, 40), (3, 100, 1), (4, 4096, 1), (4, 1, 4096)]


@pytest.mark.parametrize("shape", TAP_SHAPES, ids=lambda s: "k%d-up%d-down%d" % s)
def test_tap_shapes_slices_and_one_sample_calls_are_the_fma_chain(emu_lib, monkeypatch, shape):
    k, lu, ld = shape
    rng = np.random.default_rng(lu * 10000 + ld)
    N, T = 2, 23
    u = X.scaled_rows(rng, N, T, 3)
    m = wire(emu_lib, u)
    up, down = rng.standard_normal(lu), rng.standard_normal(ld)        # (asymmetric, and not the same both ways)
    ref = X.chain_resample(u, k, X.scaled_up_taps(k, up), down, (1,))

    def fresh():
        return runner(m, N, emu_lib).set_oversampling(k, up=up, down=down, held_rows=[1])
    for sl in ("1", "5"):               # histories of Du = 2 ... 1023 and Ld - 1 = 1 ... 4095 samples against slices of 1 and 5
        monkeypatch.setenv("ACME_OS_SLICE", sl)
        y = fresh().run(u, time_major=True)
        assert np.array_equal(y, ref), (shape, "slice " + sl, np.argwhere(y != ref)[:8])
    monkeypatch.delenv("ACME_OS_SLICE")
    y = fresh().run(u, time_major=True)
    assert np.array_equal(y, ref), (shape, "one slice", np.argwhere(y != ref)[:8])
    r = fresh()
    y = np.concatenate([r.run(np.ascontiguousarray(u[:, t:t + 1]), time_major=True) for t in range(T)], axis=1)
    assert np.array_equal(y, ref), (shape, "calls of one sample", np.argwhere(y != ref)[:8])


def test_a_run_of_one_sample_is_the_fma_chain(emu_lib):
    rng = np.random.default_rng(5)
    u = X.scaled_rows(rng, 3, 1, 3)
    m = wire(emu_lib, u)
    for k, lu, ld in ((2, 5, 4), (9, 30, 11), (16, 16, 16)):
        up, down = rng.standard_normal(lu), rng.standard_normal(ld)
        y = runner(m, 3, emu_lib).set_oversampling(k, up=up, down=down, held_rows=[1]).run(u, time_major=True)
        assert np.array_equal(y, X.chain_resample(u, k, X.scaled_up_taps(k, up), down, (1,))), (k, lu, ld)


def test_run_const_holds_its_constant_row(emu_lib, monkeypatch):
    rng = np.random.default_rng(6)
    N, T, k = 2, 19, 6
    u = X.scaled_rows(rng, N, T, 3)
    u[:, :, 1] = u[:, :1, 1]
    m = wire(emu_lib, u)
    up, down = rng.standard_normal(15), rng.standard_normal(10)
    ref = X.chain_resample(u, k, X.scaled_up_taps(k, up), down, (1,))
    monkeypatch.setenv("ACME_OS_SLICE", "5")
    uv, uc = np.ascontiguousarray(u[:, :, [0, 2]]), np.ascontiguousarray(u[:, 0, :])
    y = runner(m, N, emu_lib).set_oversampling(k, up=up, down=down).run_const(uv, uc, [1])        # (no held row named: the constant row is)
    assert np.array_equal(y, ref), np.argwhere(y != ref)[:8]


# ---- measurement --------------------------------------------------------------------------------------------------------------
def check_measurement(lib_runner, u, start, length, f0, H, rows, check=True):
    """arm, run u [N, T, c] with y stored and with y = NULL, and hold both to exact_ref"""
    N, T, c = u.shape
    rows = list(range(c)) if rows is None else rows
    spec = dict(start=start, length=length, f0=f0 if H else None, harmonics=H, rows=rows)
    r = lib_runner().set_measurement(**spec)
    y = r.run(u, time_major=True, check=check)
    assert np.array_equal(y, u), WIRE_FAILS
    out, count = raw(r)
    rn = lib_runner().set_measurement(**spec)
    rn.measure(u, time_major=True, check=check)
    out_null, count_null = raw(rn)
    assert count_null == count and np.array_equal(out_null, out, equal_nan=True), "y = NULL differs from y stored"
    seg = u[:, start:start + length if length else T][:, :, rows]
    n = seg.shape[1]
    assert count == n and out.shape == (N, len(rows), 4 + 2 * H)
    s, sq, mn, mx = X.exact_moments(seg)
    mean, rms = X.reported((s, sq), n)
    for name, got, want in (("mean", out[:, :, 0], mean), ("rms", out[:, :, 1], rms), ("min", out[:, :, 2], mn), ("max", out[:, :, 3], mx)):
        assert np.array_equal(got, want, equal_nan=True), (name, np.argwhere(got != want)[:8])
    mm = r.measurement()
    assert mm.count == n and mm.rows == tuple(rows)
    assert np.array_equal(mm.mean, mean, equal_nan=True) and np.array_equal(mm.rms, rms, equal_nan=True)
    if H:
        C_, S_, l1 = X.ld_harmonics(seg, f0, H)
        bound = X.harmonic_bound(n, l1)[:, :, None]
        gc, gs = X.unscale(out, n)
        ec, es = np.abs(gc - C_) / bound, np.abs(gs - S_) / bound
        worst = float(max(ec.max(), es.max()))
        print(f"harmonics: f0 {f0} H {H} n {n}: max |error| / bound {worst:.2e}")
        assert worst <= 1.0, (worst, np.argwhere(ec > 1.0)[:8], np.argwhere(es > 1.0)[:8])
        for h in range(1, H + 1):
            if h * f0[0] % f0[1] == 0:      # th = 0 at every sample: C_h is the sum, S_h a sum of zeros
                inv = 1.0 / n
                assert np.array_equal(out[:, :, 2 + 2 * h], 2.0 * s * inv) and not out[:, :, 3 + 2 * h].any(), h
    return out


# H = 0, 1 (one wave), 15 (a full block of 16 units), 16, 17 (two groups), 32 (the most) x the four fundamentals; the window
# 301 ... 4433 crosses the 4096-sample chunk and ends inside a 64-sample tile (4133 = 64 * 64 + 37)
M31 = 2 ** 31 - 1
MEAS_CASES = [(0, None, 301, 4133), (1, (M31 - 1, M31), 301, 4133), (15, (1, 3), 301, 4133), (16, (1234567, M31), 301, 4133),
              (17, (M31 - 1, M31), 301, 4133), (32, (3, 20), 301, 4133), (32, (1234567, M31), 0, 700), (17, (1, 3), 5, 0)]


@pytest.mark.parametrize("case", MEAS_CASES, ids=lambda c: f"H{c[0]}-f{c[1][0] if c[1] else 0}-{c[2]}-{c[3]}")
def test_measurement_moments_exact_harmonics_within_the_bound(emu_lib, case):
    H, f0, start, length = case
    N, T = 3, 4500 if length else 800
    u = X.scaled_rows(np.random.default_rng(H + start), N, T, 3)
    m = wire(emu_lib, u, 300)
    if f0 == (1, 3):
        assert any(h * f0[0] % f0[1] == 0 for h in range(1, H + 1))
    check_measurement(lambda: runner(m, N, emu_lib), u, start, length, f0, H, None)


@pytest.mark.parametrize("rows", [[3], [1, 4], None])
def test_measurement_row_masks(emu_lib, rows):
    N, T = 4, 300
    u = X.scaled_rows(np.random.default_rng(7), N, T, 5)
    m = wire(emu_lib, u)
    out = check_measurement(lambda: runner(m, N, emu_lib), u, 10, 200, (7, 50), 3, rows)
    assert out.shape[1] == (5 if rows is None else len(rows))


# (a window that starts beyond 2^20 samples needs 2^20 samples through the emulator's run kernel first -- 28 minutes here --:
# test_gpu_exact_kernels.py::test_gpu_measurement_window_far_from_the_start holds it on the GPU alone)
