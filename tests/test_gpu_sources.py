"""Sources (acme_batch_set_source_*, csrc/acme_source.h) on the MI355X: the HIP kernel's rendered values against exact
arithmetic (CONST / TABLE bit for bit, SINE against mpmath at the phase reduced in unbounded integers, within
source_ref.sine_bound), the defining property -- a source run is acme_batch_run on the rendered u, bit for bit -- at small
width in every mode and at the headline grid's width, and the measurement end to end."""
import numpy as np
import pytest

import source_ref as sr
from helpers import FS, HS, load
from test_sources import MODES, awkward_kinds, property_cases

pytestmark = pytest.mark.gpu


def runner(model, n, **kw):
    from acme_jl_amd.runner import ModelRunner
    return ModelRunner(model, n, device=0, **kw)


class TorchArrays:
    """device memory for source_ref.check_defining_property"""

    def put(self, a):
        import torch
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def empty(self, shape):
        import torch
        return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")

    def ptr(self, a):
        return None if a is None else a.data_ptr()

    def get(self, a):
        import torch
        torch.cuda.synchronize()
        return a.cpu().numpy()


# ---- 1. rendered values against exact arithmetic -----------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 4099, 10007])         # one entry, a prime, more than a slice (and than the LDS window)
@pytest.mark.parametrize("clock", sr.CLOCKS)
def test_gpu_rendered_values_are_the_exact_ones(hip_lib, clock, P):
    N, T = 7, 2 * 4096 + 1111                            # (three slices; the last ends mid-period of every row)
    rng = np.random.default_rng(P)
    kinds = awkward_kinds(N, rng, P)
    r = sr.apply_sources(runner(sr.wire_model(3, FS), N), kinds)
    r.source_clock = clock
    u = r.render_sources(T)
    # CONST and TABLE: every element, bit for bit
    assert np.array_equal(u[:, :, 1], np.broadcast_to(kinds[1]["offset"][:, None], (N, T)))
    w, amp, off = kinds[2]["table"], kinds[2]["amp"], kinds[2]["offset"]
    tab = np.array([[sr.exact_table_value(amp[i], off[i], w, j) for j in range(P)] for i in range(N)])
    assert np.array_equal(u[:, :, 2], tab[:, (clock + np.arange(T)) % P])
    # SINE: the slices' edges, the tiles' first threads and a random sample of the rest against mpmath
    ts = sorted(set([0, 1, 255, 256, 511, 512, 4095, 4096, 4097, 8191, 8192, T - 1]) | set(rng.integers(0, T, 120).tolist()))
    worst = sr.check_sine_row(u[:, :, 0], kinds[0], N, clock, [(i, t) for i in range(N) for t in ts])
    print(f"clock {clock}, P {P}: worst sine error {worst:.3f} of its bound")
    y = r.run_sources(T)
    assert np.array_equal(y, u) and r.source_clock == clock + T


@pytest.mark.parametrize("nu,lds", [(1, "1"), (1, "0"), (2, "0"), (3, "1"), (5, "1"), (6, "0")])
def test_gpu_every_store_shape_and_both_table_paths(hip_lib, monkeypatch, nu, lds):
    monkeypatch.setenv("ACME_SOURCE_LDS", lds)
    N = 9
    rng = np.random.default_rng(nu)
    tabs = [rng.standard_normal(P) for P in (1, 13, 4099, 29, 5, 2)]
    kinds = [dict(kind="table", table=tabs[c], amp=None if c % 2 else rng.standard_normal(N), offset=None if c % 3 else rng.standard_normal(N))
             for c in range(nu)]
    if nu >= 3:
        kinds[1] = None
        kinds[2] = dict(kind="sine", f_den=48, f_num=None, phase=np.arange(N) * 5)
    for T in (4096 + 5, 4096 + 600):
        r = sr.apply_sources(runner(sr.wire_model(nu, FS), N), kinds)
        r.source_clock = 2 ** 40 + 1
        uv = rng.standard_normal((N, T, 1)) if nu >= 3 else None
        u = r.render_sources(T, uv)
        for c, k in enumerate(kinds):
            if k is None:
                assert np.array_equal(u[:, :, c], uv[:, :, 0])
            elif k["kind"] == "table":
                a, o = sr.par(k.get("amp"), N, 1.0), sr.par(k.get("offset"), N, 0.0)
                P = len(k["table"])
                tab = np.array([[sr.exact_table_value(a[i], o[i], k["table"], j) for j in range(P)] for i in range(N)])
                assert np.array_equal(u[:, :, c], tab[:, (2 ** 40 + 1 + np.arange(T)) % P]), (c, T)
            else:
                sr.check_sine_row(u[:, :, c], k, N, 2 ** 40 + 1, [(i, t) for i in range(N) for t in range(0, T, 97)])


# ---- 2. the defining property, small width, every mode --------------------------------------------------------------------------
T_GPU = 2 * 4096 + 700          # three slices of run_os


@pytest.mark.parametrize("mode", range(len(MODES)))
@pytest.mark.parametrize("case", range(4))
def test_gpu_a_source_run_is_a_run_on_the_rendered_input(hip_lib, case, mode):
    name, m, N, kinds, u_var = gpu_cases()[case]
    md = dict(MODES[mode])
    if md.get("split"):
        md["split"] = 4096 + 1234          # (the cut inside the second slice)
    u = sr.check_defining_property(hip_lib, m, N, kinds, u_var, T_GPU, more=4096 + 77, clock=2 ** 31 - 20, arrays=TorchArrays(), **md)
    assert np.abs(u).max() > 1e-3 and np.isfinite(u).all()


def gpu_cases():
    """property_cases with a caller's row long enough for the GPU's slices"""
    out = property_cases()
    name, m, N, kinds, u_var = out[3]
    out[3] = (name, m, N, kinds, 0.3 * np.random.default_rng(3).standard_normal((N, T_GPU + 4096 + 77, 1)))
    return out


@pytest.mark.parametrize("held", [False, True])
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("case", range(4))
def test_gpu_oversampled_source_runs(hip_lib, case, k, held):
    name, m, N, kinds, u_var = gpu_cases()[case]
    rows = [r for r, kd in enumerate(kinds) if kd is not None and kd["kind"] != "const"][:1] if held else []
    for mode in (dict(mem=0, keep=True, split=4096 + 1234), dict(mem=1, keep=False)):
        sr.check_defining_property(hip_lib, m, N, kinds, u_var, T_GPU, k=k, held=rows, more=4096 + 77, arrays=TorchArrays(), **mode)


# ---- 3. end to end with the measurement -----------------------------------------------------------------------------------------
def test_gpu_a_measured_sine_source_is_found_in_its_bin(hip_lib):
    from exact_ref import U, exact_moments, harmonic_bound, ld_harmonics, reported, unscale
    N, f_den, f_num, periods = 6, 441, 10, 30
    T = f_den * periods                                  # 13 230 samples: four slices, whole periods
    rng = np.random.default_rng(2)
    amp, off = np.logspace(-2, 1, N), rng.standard_normal(N)
    phase = np.array([0, 7, 110, 220, 221, 440])
    r = runner(sr.wire_model(1, FS), N)
    r.set_source(0, "sine", amp=amp, offset=off, f_den=f_den, f_num=f_num, phase=phase)
    H = 4
    r.set_measurement(f0=(f_num, f_den), harmonics=H)
    u = r.render_sources(T)
    r.measure(T=T)
    out, count = sr.raw_measurement(r)
    assert count == T
    C_, S_, l1 = ld_harmonics(u, (f_num, f_den), H)
    Cg, Sg = unscale(out, count)
    bound = harmonic_bound(T, l1)[:, :, None]
    assert (np.abs(Cg - C_) <= bound).all() and (np.abs(Sg - S_) <= bound).all()
    A = out[:, 0, 4::2] + 1j * out[:, 0, 5::2]
    th = 2 * np.pi * phase / f_den - np.pi / 2
    per_sample = np.array([sr.sine_bound(a, o) for a, o in zip(amp, off)])
    tol = 2.0 / T * (harmonic_bound(T, l1)[:, 0] + T * per_sample) + 4 * U * amp
    assert (np.abs(A[:, 0] - amp * np.exp(1j * th)) <= np.sqrt(2) * tol).all(), np.abs(A[:, 0] - amp * np.exp(1j * th)) / tol
    assert (np.abs(A[:, 1:]) <= np.sqrt(2) * tol[:, None]).all()
    s, sq, mn, mx = exact_moments(u)
    assert np.array_equal(out[:, :, 0], reported((s, sq), count)[0])
    assert (np.abs(out[:, 0, 0] - off) <= (T + 2) * U * l1[:, 0] / T + per_sample).all()


def test_gpu_a_frequency_sweep_is_one_batch(hip_lib):
    N, f_den = 4, 4410
    f_num = np.array([3, 100, 441, 1000])
    T = 2 * f_den
    r = runner(sr.wire_model(1, FS), N)
    r.set_source(0, "sine", f_den=f_den, f_num=f_num, amp=2.0)
    for i in range(N):
        r.source_clock = 0
        r.set_measurement(f0=(int(f_num[i]), f_den), harmonics=1)
        r.measure(T=T)
        a1 = np.abs(r.measurement().harmonics[:, 0, 0])
        assert abs(a1[i] - 2.0) < 1e-11
        assert (np.delete(a1, i) < 1e-11).all(), a1


# ---- 5. at width ----------------------------------------------------------------------------------------------------------------
def test_gpu_headline_grid_as_a_source_run(hip_lib):
    """The headline grid's shape: 8 192 instances of superover (caching solver stack), one second at 44.1 kHz, sine levels
    spaced over 40 dB on the signal row, the grid's pot positions as CONST rows, H = 8 harmonics measured, y = NULL, device
    memory.  A contiguous quarter of the grid (2 048 instances) run through acme_batch_run on its rendered u measures the
    same, with ==, and reports the same n_warn and iters_total."""
    import torch
    from acme_jl_amd.model import CachingHomotopySolver
    m = load("superover_var", CachingHomotopySolver)
    N, T, Q = 8192, FS, 2048
    idx = np.arange(N)          # (bench.py's superover grid: level fastest, then tone, then drive)
    pots = np.stack([(idx // 256) / float(N // 256), ((idx // 16) % 16) / 15.0, (idx % 16) / 15.0], axis=1)
    amp = 10.0 ** (-2.0 + 2.0 * ((idx * 2654435761) % N) / (N - 1.0))           # 40 dB, spread over the grid's cells
    spec = dict(f0=(10, 441), harmonics=8)

    def arm(r, lo, hi):
        r.set_source(0, "sine", f_den=441, f_num=10, amp=amp[lo:hi])
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
    twin = runner(m, Q).set_measurement(**spec)
    twin.lib.check(twin.lib.L.acme_batch_run(twin.h, ud.data_ptr(), None, T, 1, st))
    torch.cuda.synchronize()
    want, count2 = sr.raw_measurement(twin)
    assert count2 == T
    assert np.isfinite(want).all() and np.abs(want[:, 0, 4:6]).max() > 1e-3
    assert np.array_equal(got[lo:lo + Q], want)
    rt = twin.report_arrays()
    assert np.array_equal(rep["n_warn"][lo:lo + Q], rt["n_warn"]) and np.array_equal(rep["iters_total"][lo:lo + Q], rt["iters_total"])
    # the rendered quarter is what the issue says it is: the sine at its level, the pots in their rows
    u0 = ud[:3, :5].cpu().numpy()
    assert np.array_equal(u0[:, :, 1:], np.broadcast_to(pots[lo:lo + 3, None, :], (3, 5, 3)))
    sr.check_sine_row(u0[:, :, 0], dict(f_den=441, f_num=10, amp=amp[lo:lo + 3]), 3, 0, [(i, t) for i in range(3) for t in range(5)])
