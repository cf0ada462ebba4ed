"""Oversampled runs (acme_batch_set_oversampling) on the MI355X: the plumbing bit for bit against the GPU's own run at the
model rate in every kernel family, the filters against the CPU oracle, the bit-identity of host / device memory, run_async,
run_const and split calls, BASELINE config 5 at the base rate, and what oversampling is for: less aliasing."""
import warnings
from fractions import Fraction

import numpy as np
import pytest

from helpers import FS, HS, RTOL, assert_close, load, oracle_run, sine, sweep_inputs
from test_oversampling import birdie_u, clipper_176k, np_decimate, np_interpolate, plumbing_cases

pytestmark = pytest.mark.gpu

# Aliasing test: a 5 kHz sine of 5 V into the diode clipper.  Energy in the bins that are not harmonics of 5 kHz, plain
# run at 44.1 kHz against the 176.4 kHz model with k = 4 and the default filters: 41.1 dB lower on the CPU oracle with the
# same numpy-composed filters (53.8 dB at 2 V, 41.0 dB at 10 V); committed with a margin.
ALIAS_REDUCTION_DB = 30.0


def runner(model, n, **kw):
    from acme_jl_amd.runner import ModelRunner
    return ModelRunner(model, n, device=0, **kw)


@pytest.mark.parametrize("case", range(4))
def test_gpu_plumbing_is_a_plain_run_at_the_model_rate(hip_lib, case):
    name, m, u, family = plumbing_cases()[case]
    k = 3 if case == 3 else 4
    N = u.shape[0]
    ref = runner(m, N)
    assert ref.batch_kernel_variant()[1] == family, name
    y_os = ref.run(np.repeat(u, k, axis=1), time_major=True)
    r = runner(m, N).set_oversampling(k, down=[1.0], held_rows=range(m.nu))
    assert r.batch_kernel_variant()[1] == family, name
    y = r.run(u, time_major=True)
    assert np.array_equal(y, y_os[:, k - 1::k]), name
    assert np.array_equal(r.report_arrays()["iters_total"], ref.report_arrays()["iters_total"])


@pytest.mark.parametrize("which", ["birdie_var_176k", "clipper"])
def test_gpu_filtered_run_matches_the_oracle(hip_lib, which):
    from acme_jl_amd.runner import design_oversampling_filter
    k = 4
    if which == "clipper":
        m, u, held = clipper_176k(), 2.0 * np.array([0.3, 1.0, 3.0])[:, None, None] * sine(600, f=3000.0)[None, :, None], ()
    else:
        m, u, held = load(which, HS), birdie_u(4, 600), (1,)
    h = design_oversampling_filter(k)
    y = runner(m, u.shape[0]).set_oversampling(k, held_rows=held).run(u, time_major=True)
    uo = np_interpolate(u, k, k * h, held)
    y_os, _ = oracle_run(m, uo.transpose(0, 2, 1))
    assert_close(y, np_decimate(np.ascontiguousarray(y_os.transpose(0, 2, 1)), k, h), RTOL)
    assert np.abs(y).max() > 1e-3


def test_gpu_memory_paths_and_split_calls_are_bit_identical(hip_lib):
    import torch
    m = load("birdie_var_176k", HS)
    N, T, t1 = 64, 9000, 4133                   # (three time slices of 4 096 base-rate samples; the split falls inside one)
    u = birdie_u(N, T)

    def fresh():
        return runner(m, N).set_oversampling(4, held_rows=[1])
    y = fresh().run(u, time_major=True)
    assert np.isfinite(y).all() and np.abs(y).max() > 1e-3
    # device memory
    r = fresh()
    yd = r.run_torch(torch.from_numpy(u).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(yd.cpu().numpy(), y)
    # run_async on host buffers
    r = fresh()
    ya = np.empty_like(y)
    r.run_async(u, ya)
    r.wait()
    assert np.array_equal(ya, y)
    # run_const, host and device memory
    uv, uc = np.ascontiguousarray(u[:, :, :1]), np.ascontiguousarray(u[:, 0, :])
    assert np.array_equal(runner(m, N).set_oversampling(4).run_const(uv, uc, [1]), y)
    r = runner(m, N).set_oversampling(4)
    yc = torch.empty((N, T, 1), dtype=torch.float64, device="cuda")
    uvd, ucd = torch.from_numpy(uv).cuda(), torch.from_numpy(uc).cuda()
    r.lib.check(r.lib.L.acme_batch_run_const(r.h, uvd.data_ptr(), ucd.data_ptr(), 2, yc.data_ptr(), T, 1,
                                             torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert np.array_equal(yc.cpu().numpy(), y)
    # split calls, host and device
    r = fresh()
    a = r.run(np.ascontiguousarray(u[:, :t1]), time_major=True)
    b = r.run(np.ascontiguousarray(u[:, t1:]), time_major=True)
    assert np.array_equal(np.concatenate([a, b], axis=1), y)
    r = fresh()
    ud = torch.from_numpy(u).cuda()
    a = r.run_torch(ud[:, :t1].contiguous())
    b = r.run_torch(ud[:, t1:].contiguous())
    torch.cuda.synchronize()
    assert np.array_equal(torch.cat([a, b], dim=1).cpu().numpy(), y)


def test_gpu_config5_at_the_base_rate(hip_lib):
    """BASELINE config 5 as worded: birdie at 4x oversampling -- 2 048 instances, one second of 44.1 kHz audio, vol held"""
    import torch
    from acme_jl_amd.runner import design_oversampling_filter
    m = load("birdie_var_176k")
    N, T, k = 2048, FS, 4
    u = np.ascontiguousarray(sweep_inputs("birdie_var", N, T).transpose(0, 2, 1))
    r = runner(m, N).set_oversampling(k, held_rows=[1])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        y = r.run_torch(torch.from_numpy(u).cuda()).cpu().numpy()
        r.check()
    assert np.isfinite(y).all()
    ra = r.report_arrays()
    assert (ra["n_warn"] == 0).all() and (ra["first_nonfinite"] < 0).all()
    # today's way on the same interpolated input (instances are independent: a spread of 16 of them)
    pick = np.linspace(0, N - 1, 16).astype(int)
    h = design_oversampling_filter(k)
    uo = np_interpolate(u[pick], k, k * h, held=(1,))
    y_os = runner(m, len(pick)).run(uo, time_major=True)
    assert_close(y[pick], np_decimate(y_os, k, h), RTOL)


def _non_harmonic_energy(y, skip, W, period_bins):
    X = np.abs(np.fft.rfft(y[skip:skip + W])) ** 2
    harm = np.zeros(len(X), bool)
    harm[::period_bins] = True
    return X[~harm].sum()


def test_gpu_oversampling_reduces_aliasing(hip_lib):
    from acme_jl_amd import examples
    from acme_jl_amd.model import DiscreteModel
    skip, W = 2205, 8820                        # (W: 1 000 periods of 5 kHz -- the harmonics fall on every 1 000th bin)
    u = 5.0 * np.sin(2 * np.pi * 5000 / FS * np.arange(skip + W))
    plain = runner(DiscreteModel(examples.diodeclipper(), Fraction(1, FS), HS), 1).run(u[None])
    os4 = runner(clipper_176k(), 1).set_oversampling(4).run(u[None])
    e_plain = _non_harmonic_energy(plain[0], skip, W, 1000)
    e_os = _non_harmonic_energy(os4[0], skip, W, 1000)
    reduction = 10 * np.log10(e_plain / e_os)
    print(f"aliasing: non-harmonic energy {reduction:.1f} dB lower with 4x oversampling")
    assert reduction >= ALIAS_REDUCTION_DB, reduction
