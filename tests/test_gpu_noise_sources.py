"""NOISE rows (acme_batch_set_source_noise, csrc/acme_source.h) on the MI355X: the HIP kernel's UNIFORM rows against noise_ref bit
for bit -- which is also the emulator-against-GPU statement in its strongest form --, GAUSSIAN rows against mpmath within
noise_ref.gauss_bound, the render's independence of the layout, the defining property of the sources at small width in every
mode and with oversampling, the moments through the measurement, and one run at the headline grid's width."""
import numpy as np
import pytest

import noise_ref as nr
import source_ref as sr
from helpers import FS, load
from test_gpu_sources import TorchArrays
from test_sources import MODES

pytestmark = pytest.mark.gpu


def runner(model, n, **kw):
    from acme_jl_amd.runner import ModelRunner
    return ModelRunner(model, n, device=0, **kw)


# ---- exact rows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clock", sr.CLOCKS)
def test_gpu_rendered_rows_are_the_exact_ones(hip_lib, clock):
    from test_noise_sources import exact_kinds
    N, T = 7, 2 * 4096 + 1111                            # (three slices; the last ends mid-tile)
    rng = np.random.default_rng(1)
    kinds = exact_kinds(N, rng)
    r = nr.apply_sources(runner(sr.wire_model(3, FS), N), kinds)
    r.source_clock = clock
    u = r.render_sources(T)
    for row in (0, 2):                                   # UNIFORM: every element, bit for bit
        want = nr.uniform_row(kinds[row], row, N, T, clock)
        assert np.array_equal(u[:, :, row], want), (row, np.argwhere(u[:, :, row] != want)[:4])
    # GAUSSIAN: the slices' edges, the tiles' first threads and a random sample of the rest against mpmath
    worst = 0.0
    for i in range(N):
        ts = sorted(set([0, 1, 255, 256, 511, 512, 4095, 4096, 4097, 8191, 8192, T - 1]) | set(rng.integers(0, T, 120).tolist()))
        worst = max(worst, nr.check_gauss_row(u[:, :, 1], kinds[1], 1, N, clock, [(i, t) for t in ts]))
    print(f"clock {clock}: worst Gaussian error {worst:.3f} of its bound")
    q = (clock + np.arange(T)) // 7                      # the held row: blocks of 7 aligned to the clock
    assert (u[:, 1:, 2] == u[:, :-1, 2])[:, q[1:] == q[:-1]].all() and (u[:, 1:, 2] != u[:, :-1, 2])[:, q[1:] != q[:-1]].all()
    y = r.run_sources(T)
    assert np.array_equal(y, u) and r.source_clock == clock + T


# ---- layout independence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold", [1, 4096 + 5])
@pytest.mark.parametrize("nu", [1, 2, 3, 5, 6])
def test_gpu_every_store_shape(hip_lib, nu, hold):
    """a row's values are those of the six-row layout -- they depend on (stream, row, clock) alone --, and the UNIFORM rows are
    noise_ref's with =="""
    N, clock = 6, 2 ** 40 + 1
    kinds = nr.layout_kinds(N, hold)
    for T in (4096 + 5, 4096 + 600):
        uv = np.random.default_rng(T).standard_normal((N, T, 1))
        six = nr.apply_sources(runner(sr.wire_model(6, FS), N), kinds)
        six.source_clock = clock
        ref = six.render_sources(T, uv)
        r = nr.apply_sources(runner(sr.wire_model(nu, FS), N), kinds[:nu])
        r.source_clock = clock
        u = r.render_sources(T, uv if nu >= 3 else None)
        assert np.array_equal(u, ref[:, :, :nu]), (T, np.argwhere(u != ref[:, :, :nu])[:4])
        if nu >= 3:
            assert np.array_equal(u[:, :, 2], uv[:, :, 0])
        for row in (1, 5):
            assert np.array_equal(ref[:, :, row], nr.uniform_row(kinds[row], row, N, T, clock)), (row, T)
        tab = sr.expected_rows([None] * 3 + [kinds[3]], N, 29, 0)[:, :, 3]
        assert np.array_equal(ref[:, :, 3], tab[:, (clock + np.arange(T)) % 29])
        nr.check_gauss_row(ref[:, :, 4], kinds[4], 4, N, clock, [(i, t) for i in range(N) for t in (0, 4095, 4096, T - 1)])


def test_gpu_noise_next_to_a_multisine(hip_lib):
    from test_noise_sources import check_noise_next_to_a_multisine
    check_noise_next_to_a_multisine(runner, 6, 4096 + 600, 2 ** 40 + 1)


# ---- the defining property, small width, every mode ---------------------------------------------------------------------------------
T_GPU = 2 * 4096 + 700          # three slices of run_os


@pytest.mark.parametrize("mode", range(len(MODES)))
@pytest.mark.parametrize("case", range(2))
def test_gpu_a_noise_source_run_is_a_run_on_the_rendered_input(hip_lib, case, mode):
    name, m, N, kinds = nr.property_cases()[case]
    md = dict(MODES[mode])
    if md.get("split"):
        md["split"] = 4096 + 1234          # (the cut inside the second slice)
    u = nr.check_defining_property(hip_lib, m, N, kinds, None, T_GPU, more=4096 + 77, clock=2 ** 31 - 20, arrays=TorchArrays(), **md)
    assert np.abs(u[:, :, 0]).max() > 1e-2 and np.isfinite(u).all()


@pytest.mark.parametrize("mode", [dict(mem=0, keep=True, split=4096 + 1234), dict(mem=1, keep=False)], ids=["host-split", "device-measured"])
@pytest.mark.parametrize("held", [False, True])
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("case", range(2))
def test_gpu_oversampled_noise_source_runs(hip_lib, case, k, held, mode):
    name, m, N, kinds = nr.property_cases()[case]
    nr.check_defining_property(hip_lib, m, N, kinds, None, T_GPU, k=k, held=[0] if held else [], more=300, arrays=TorchArrays(), **mode)


# ---- moments through the measurement ------------------------------------------------------------------------------------------------
def test_gpu_moments_of_a_measured_uniform_row(hip_lib):
    from exact_ref import exact_moments, reported
    N, T = 4, 2 * 4096 + 5
    rng = np.random.default_rng(4)
    k = nr.noise("uniform", amp=np.logspace(-2, 1, N), offset=rng.standard_normal(N), seed=1)
    r = nr.apply_sources(runner(sr.wire_model(1, FS), N), [k])
    r.source_clock = 2 ** 40
    r.set_measurement(harmonics=0)
    u = r.render_sources(T)
    assert np.array_equal(u[:, :, 0], nr.uniform_row(k, 0, N, T, 2 ** 40))
    r.measure(T=T)
    out, count = sr.raw_measurement(r)
    assert count == T
    s, sq, mn, mx = exact_moments(u)
    mean, rms = reported((s, sq), count)
    for name, got, want in (("mean", out[:, :, 0], mean), ("rms", out[:, :, 1], rms), ("min", out[:, :, 2], mn), ("max", out[:, :, 3], mx)):
        assert np.array_equal(got, want), name


# ---- at width -------------------------------------------------------------------------------------------------------------------------
def test_gpu_headline_grid_driven_by_noise(hip_lib):
    """8 192 instances of superover (caching solver stack), 4 096 + 700 samples (two slices show everything width can show),
    Gaussian noise with levels over 40 dB on the signal row (0.00316 ... 0.316 V RMS: white noise peaks at 4.5 sigma, so the top
    level peaks where the sine of test_gpu_sources' grid does, at 1.4 V), the grid's pot positions as CONST rows, a measurement
    armed, y = NULL, device memory.  A contiguous quarter of the grid (2 048 instances, its streams those of the global index) run
    through acme_batch_run on its rendered u measures the same, with ==, and reports the same n_warn and iters_total."""
    import torch
    from acme_jl_amd.model import CachingHomotopySolver
    m = load("superover_var", CachingHomotopySolver)
    N, T, Q = 8192, 4096 + 700, 2048
    idx = np.arange(N)          # (bench.py's superover grid: level fastest, then tone, then drive)
    pots = np.stack([(idx // 256) / float(N // 256), ((idx // 16) % 16) / 15.0, (idx % 16) / 15.0], axis=1)
    amp = 10.0 ** (-2.5 + 2.0 * ((idx * 2654435761) % N) / (N - 1.0))           # 40 dB, spread over the grid's cells
    spec = dict(f0=(10, 441), harmonics=8)

    def arm(r, lo, hi):
        r.set_source(0, "noise", amp=amp[lo:hi], stream=idx[lo:hi])
        for c in range(3):
            r.set_source(1 + c, "const", offset=pots[lo:hi, c])
        return r.set_measurement(**spec)
    st = torch.cuda.current_stream().cuda_stream
    full = arm(runner(m, N), 0, N)
    full.lib.check(full.lib.L.acme_batch_run_sources(full.h, None, None, T, 1, st))
    torch.cuda.synchronize()
    got, count = sr.raw_measurement(full)
    rep = full.report_arrays()
    assert count == T and full.source_clock == T
    lo = 3 * Q                  # (the quarter with the highest drive)
    part = arm(runner(m, Q), lo, lo + Q)
    ud = torch.empty((Q, T, 4), dtype=torch.float64, device="cuda")
    part.lib.check(part.lib.L.acme_batch_render_sources(part.h, None, ud.data_ptr(), T, 1, st))
    assert bool(torch.isfinite(ud).all()) and float(ud[:, :, 0].abs().max()) > 1.0
    twin = runner(m, Q).set_measurement(**spec)
    twin.lib.check(twin.lib.L.acme_batch_run(twin.h, ud.data_ptr(), None, T, 1, st))
    torch.cuda.synchronize()
    want, count2 = sr.raw_measurement(twin)
    assert count2 == T
    print("non-finite measurements:", int((~np.isfinite(want)).sum()), "largest rms", float(np.nanmax(want[:, 0, 1])))
    assert np.isfinite(want).all() and np.abs(want[:, 0, 1]).max() > 1e-3
    assert np.array_equal(got[lo:lo + Q], want)
    rt = twin.report_arrays()
    assert np.array_equal(rep["n_warn"][lo:lo + Q], rt["n_warn"]) and np.array_equal(rep["iters_total"][lo:lo + Q], rt["iters_total"])
    # the rendered quarter is what the issue says it is: the noise at its level, the pots in their rows
    u0 = ud[:3, :5].cpu().numpy()
    assert np.array_equal(u0[:, :, 1:], np.broadcast_to(pots[lo:lo + 3, None, :], (3, 5, 3)))
    nr.check_gauss_row(u0[:, :, 0], nr.noise("gaussian", amp=amp[lo:lo + 3], stream=idx[lo:lo + 3]), 0, 3, 0, [(i, t) for i in range(3) for t in range(5)])
