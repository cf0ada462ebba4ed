"""The resampling (csrc/acme_resample.h) and measurement (csrc/acme_measure.h) kernels on the MI355X on exactly known
signals: exact_ref's references (no code shared with the library) at shapes that exercise the launch geometry -- several
blocks, instances straddling block edges, all 15 instantiations of the interpolator, and the measurement kernel's LDS
tiles, readlane broadcasts, 1024-thread blocks, blockIdx.y groups, pairs straddling instances and strided row loads, none
of which the CPU emulator runs.

Thresholds: exact equality, exact_ref.ld_bound (two stacked fma chains) or exact_ref.harmonic_bound ((n + 16) 2^-53
sum |y_t|), both derived there.  Observed on the MI355X, as a record: resampler |error| / ld_bound at most 2.8e-1
(k = 2; 4.6e-2 ... 2.4e-1 for the other factors), harmonics |error| / bound at most 3.6e-4.

Every case is one library call in this process; the references (Fraction-exact chains, mpmath twiddles) are the run time."""
import numpy as np
import pytest

import exact_ref as X
from test_exact_kernels import M31, check_measurement, runner, wire

pytestmark = pytest.mark.gpu

N_OS, T_OS, SLICE = 45, 150, 37         # 6 750 threads a signal, not a multiple of 256; slices of 37 samples: 7 blocks each


def test_gpu_wire_precondition_over_many_blocks(hip_lib):
    u = X.scaled_rows(np.random.default_rng(0), 3000, 100, 3)
    wire(hip_lib, u)


def os_positions():
    """(instance, sample): the first and last instance and the one whose threads straddle the first block edge (instance 6
    of a 37-sample slice: threads 222 ... 258), at the first and last sample and either side of slice boundaries"""
    return [(i, t) for i in (0, 6, N_OS - 1) for t in (0, SLICE - 1, SLICE, 4 * SLICE - 1, 4 * SLICE, T_OS - 1)]


def check_resampled(y, u, k, up, down, held):
    g = X.scaled_up_taps(k, up)
    ref, bound = X.ld_resample(u, k, g, down, held), X.ld_bound(u, k, g, down, held)
    err = np.abs(y - ref)
    assert (err <= bound).all(), (k, len(up), len(down), np.argwhere(err > bound)[:8])
    pos = os_positions()
    exact = X.chain_decim(X.LazyInterp(u, k, g, held), k, down, pos)
    got = np.array([y[i, t] for i, t in pos])
    assert np.array_equal(got, exact), (k, len(up), len(down), [pos[n] for n in np.argwhere(got != exact)[:8, 0]])
    return float((err[bound > 0] / bound[bound > 0]).max())


@pytest.mark.parametrize("k", range(2, 17))
def test_gpu_every_factor_default_and_odd_taps(hip_lib, monkeypatch, k):
    from acme_jl_amd.runner import design_oversampling_filter
    rng = np.random.default_rng(100 + k)
    u = X.scaled_rows(rng, N_OS, T_OS, 3)
    m = wire(hip_lib, u)
    monkeypatch.setenv("ACME_OS_SLICE", str(SLICE))
    h = design_oversampling_filter(k)
    y = runner(m, N_OS, hip_lib).set_oversampling(k, held_rows=[1]).run(u, time_major=True)
    worst = check_resampled(y, u, k, h, h, (1,))
    # an odd shape per factor: Du = 1 or 2, fewer taps down than up or more, asymmetric random taps, different both ways
    lu, ld = 2 * k + 1 - k % 3, k + 3 + k % 5
    up, down = rng.standard_normal(lu), rng.standard_normal(ld)
    y = runner(m, N_OS, hip_lib).set_oversampling(k, up=up, down=down, held_rows=[1]).run(u, time_major=True)
    worst = max(worst, check_resampled(y, u, k, up, down, (1,)))
    print(f"resampler k = {k}: max |error| / ld_bound {worst:.2e}")


@pytest.mark.parametrize("k", [2, 5, 16])
def test_gpu_host_device_and_split_calls_agree(hip_lib, monkeypatch, k):
    import torch
    rng = np.random.default_rng(200 + k)
    u = X.scaled_rows(rng, N_OS, T_OS, 3)
    m = wire(hip_lib, u)
    monkeypatch.setenv("ACME_OS_SLICE", str(SLICE))
    up, down = rng.standard_normal(3 * k + 2), rng.standard_normal(2 * k + 5)

    def fresh():
        return runner(m, N_OS, hip_lib).set_oversampling(k, up=up, down=down, held_rows=[1])
    y = fresh().run(u, time_major=True)
    check_resampled(y, u, k, up, down, (1,))
    ud = torch.from_numpy(u).cuda()
    yd = fresh().run_torch(ud)
    torch.cuda.synchronize()
    assert np.array_equal(yd.cpu().numpy(), y), "device memory"
    r, t1 = fresh(), 2 * SLICE + 9                      # (the split falls inside a slice)
    a = r.run(np.ascontiguousarray(u[:, :t1]), time_major=True)
    b = r.run(np.ascontiguousarray(u[:, t1:]), time_major=True)
    assert np.array_equal(np.concatenate([a, b], axis=1), y), "split call"
    r = fresh()
    a, b = r.run_torch(ud[:, :t1].contiguous()), r.run_torch(ud[:, t1:].contiguous())
    torch.cuda.synchronize()
    assert np.array_equal(torch.cat([a, b], dim=1).cpu().numpy(), y), "split call, device memory"


# (H, f0, N, measured rows of 5): P = N nrows pairs, never a multiple of 64, so that a block's 64 pairs straddle instances
# and rows; H = 15 a 1024-thread block, 16 and 17 two groups (17: 9 waves each, the last one idle), 32 the most.  The window
# 301 ... 8800 runs over three 4096-sample chunks and ends 52 samples into a tile.
GPU_MEAS = [(0, None, 45, [1, 3]), (15, (1, 3), 43, [0, 2, 4]), (16, (M31 - 1, M31), 27, None),
            (17, (1234567, M31), 77, [0, 4]), (32, (3, 20), 43, [1, 2, 3])]


@pytest.mark.parametrize("case", GPU_MEAS, ids=lambda c: f"H{c[0]}-N{c[2]}-rows{5 if c[3] is None else len(c[3])}")
def test_gpu_measurement_moments_exact_harmonics_within_the_bound(hip_lib, case):
    H, f0, N, rows = case
    assert N * (5 if rows is None else len(rows)) % 64 != 0
    u = X.scaled_rows(np.random.default_rng(300 + H), N, 9000, 5)
    m = wire(hip_lib, u)
    check_measurement(lambda: runner(m, N, hip_lib), u, 301, 8500, f0, H, rows)


def test_gpu_measurement_window_far_from_the_start(hip_lib):
    """a window that starts beyond 2^20 samples, reached by y = NULL runs of constant input: the position arithmetic of the
    measurement step at large values; the twiddles' phase counts from the window's start, so the results are those of the
    same window at the start of a fresh batch, bit for bit -- and those are held to the references"""
    from test_measurement import raw
    N, lead, n, f0, H = 5, 2 ** 20 + 77, 4133, (1234567, M31), 4
    u = X.scaled_rows(np.random.default_rng(8), N, n + 40, 3)
    m = wire(hip_lib, u)
    const = np.ascontiguousarray(np.broadcast_to(u[:, :1], (N, 2 ** 16, 3)))
    outs = []
    for keep in (True, False):
        r = runner(m, N, hip_lib).set_measurement(start=lead, length=n, f0=f0, harmonics=H)
        done = 0
        while done < lead - 20:
            step = min(2 ** 16, lead - 20 - done)
            r.measure(np.ascontiguousarray(const[:, :step]), time_major=True)
            done += step
        if keep:
            assert np.array_equal(r.run(u, time_major=True), u)
        else:
            r.measure(u, time_major=True)
        outs.append(raw(r))
    assert outs[0][1] == n and outs[1][1] == n and np.array_equal(outs[0][0], outs[1][0])
    ref = check_measurement(lambda: runner(m, N, hip_lib), np.ascontiguousarray(u[:, 20:]), 0, n, f0, H, None)
    assert np.array_equal(outs[0][0], ref)
