"""The multisine source (acme_batch_set_source_multisine) and measurement bins (acme_batch_set_measurement_bins) on the
MI355X: the multi-tone instantiation of the source kernel (acme_source_multi_kernel) and the bins' twiddle kernel
(acme_meas_bins_tw_kernel) ahead of acme_meas_pi_kernel's uniform and mixed waves, which the CPU emulator only walks as plain
loops.  The cases are those of test_multitone.py at the GPU's slice and chunk lengths, and the headline grid at width."""
import numpy as np
import pytest

import exact_ref as X
import measure_pi_ref as PI
import multitone_ref as MT
import source_ref as sr
from helpers import FS, HS, load
from test_gpu_sources import TorchArrays
from test_measurement import clipper, clipper_u, raw, two_output_clipper
from test_multitone import M31, MODES, property_cases

pytestmark = pytest.mark.gpu


def runner(model, n, **kw):
    from acme_jl_amd.runner import ModelRunner
    return ModelRunner(model, n, device=0, **kw)


# ---- source ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clock", sr.CLOCKS)
def test_gpu_one_tone_is_the_sine_row(hip_lib, clock):
    """f_den = 2^31 - 1 with f_num near it, every store shape (nu = 1 ... 6), an odd and an even length beyond a tile"""
    N = 9
    rng = np.random.default_rng(1)
    one = MT.awkward_tones(1, N, rng)
    sine = dict(one, kind="sine", f_num=one["f_num"][0], phase=one["phase"][0], amp=one["amp"][0])
    for nu in range(1, 7):
        row = (nu - 1) // 2
        for T in (4096 + 5, 4096 + 600):
            us = []
            for k in (one, sine):
                kinds = [dict(kind="const", offset=rng.standard_normal(N)) if c % 2 else None for c in range(nu)]
                kinds[row] = k
                r = sr.apply_sources(runner(sr.wire_model(nu, FS), N), kinds)
                r.source_clock = clock
                us.append(r.render_sources(T)[:, :, row])
            assert np.array_equal(us[0], us[1]), (nu, T)
            assert np.abs(us[0]).max() > 1e-3


@pytest.mark.parametrize("tones", [2, 3, 4])
@pytest.mark.parametrize("clock", sr.CLOCKS)
def test_gpu_tones_against_mpmath(hip_lib, clock, tones):
    N, T = 7, 2 * 4096 + 1111                            # (three slices; the last ends mid-period)
    rng = np.random.default_rng(tones)
    k = MT.awkward_tones(tones, N, rng)
    r = sr.apply_sources(runner(sr.wire_model(2, FS), N), [dict(kind="const", offset=1.0), k])
    r.source_clock = clock
    u = r.render_sources(T)
    ts = sorted(set([0, 1, 255, 256, 511, 512, 4095, 4096, 4097, 8191, 8192, T - 1]) | set(rng.integers(0, T, 60).tolist()))
    worst = MT.check_multisine_row(u[:, :, 1], k, N, clock, [(i, t) for i in range(N) for t in ts])
    print(f"clock {clock}, {tones} tones: worst error {worst:.3f} of its bound")
    assert np.array_equal(u[:, :, 0], np.ones((N, T)))
    y = r.run_sources(T)
    assert np.array_equal(y, u) and r.source_clock == clock + T


T_GPU = 2 * 4096 + 700          # three slices of a run


@pytest.mark.parametrize("mode", range(len(MODES)))
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("case", range(2))
def test_gpu_a_multisine_run_is_a_run_on_the_rendered_input(hip_lib, case, k, mode):
    name, m, N, kinds = property_cases()[case]
    md = dict(MODES[mode])
    if md.get("split"):
        md["split"] = 4096 + 1234          # (the cut inside the second slice)
    u = sr.check_defining_property(hip_lib, m, N, kinds, None, T_GPU, k=k, more=4096 + 77, clock=2 ** 31 - 20, arrays=TorchArrays(), **md)
    assert np.abs(u).max() > 1e-3 and np.isfinite(u).all()


# ---- bins -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MT.tone_cases()))
def test_gpu_each_bin_is_the_shared_measurement_at_its_frequency(hip_lib, name):
    f_num, kinds = MT.tone_cases()[name]
    coef = np.array([[-1, 1], [1, -1], [2, -2], [0, 0]]) if name == "F=N" else MT.COEF6
    # two chunks; 4 297 = 67 x 64 + 9 samples measured
    got, kb = MT.check_bins_against_shared(runner, clipper(), f_num, kinds, 441, 4300, dict(start=3), coef)
    assert (kb > 441 // 2).any()
    assert np.abs(got[0][:, 0, 4:6]).max() > 1e-3


@pytest.mark.parametrize("B", [0, 1, 10, 17, 32])
def test_gpu_one_tone_with_harmonic_coefficients_is_the_per_instance_form(hip_lib, B):
    for m, N, rows in ((clipper(), 131, None), (two_output_clipper(), 99, None), (two_output_clipper(), 99, [1])):
        u = clipper_u(N, 9000)                                  # (three chunks of 4 096 samples, the last tile ragged)
        f_num = np.array([10, 20, 30])[np.arange(N) % 3]
        spec = dict(start=301, length=8500, rows=rows)
        rp = runner(m, N).set_measurement(f_den=441, f_num=f_num, harmonics=B, **spec)
        y = rp.run(u, time_major=True)
        rb = runner(m, N).set_measurement_bins(1 + np.arange(B), f_den=441, f_num=f_num[None], **spec)
        assert np.array_equal(rb.run(u, time_major=True), y)
        (a, ca), (b, cb) = raw(rp), raw(rb)
        assert ca == cb == 8500 and (N * a.shape[1]) % 64 != 0
        assert np.array_equal(a, b), (B, N, rows, np.argwhere(a != b)[:8])
        pa, pb = rp.measurement_plan(), rb.measurement_plan()
        assert np.array_equal(pa["perm"], pb["perm"]) and np.array_equal(pa["wave_group"], pb["wave_group"])
        assert PI.wave_kinds(rb)[1] > 0                         # (mixed waves among them)


def test_gpu_bins_are_bit_identical_across_every_path(hip_lib, monkeypatch):
    import torch
    m = clipper()
    N, T, t1 = 130, 9000, 4133
    # 26 pairs a group, no whole wave: two mixed waves and the last 2 pairs of the fifth group a wave of their own
    f_num = np.stack([np.array([17, 18, 19, 21, 23])[np.arange(N) % 5], np.full(N, 20)])
    tt = dict(MT.two_tone(N, 441, 19, 20), f_num=f_num)
    spec = dict(start=100, length=8000, f_den=441, f_num=f_num)

    def fresh(sourced=False):
        r = runner(m, N)
        if sourced:
            sr.apply_sources(r, [tt])
        return r.set_measurement_bins(MT.COEF6, **spec)
    r = fresh(True)
    assert PI.wave_kinds(r) == (1, 2) and r.measurement_plan()["groups"] == 5
    u = r.render_sources(T)
    y = r.run_sources(T)
    ref = raw(r)
    assert ref[1] == 8000 and np.isfinite(ref[0]).all()
    results = {"sourced, y NULL": raw(fresh(True).measure(T=T)), "y NULL": raw(fresh().measure(u, time_major=True))}
    r = fresh()
    assert np.array_equal(r.run(np.ascontiguousarray(u[:, :t1]), time_major=True), y[:, :t1])
    r.measure(np.ascontiguousarray(u[:, t1:]), time_major=True)
    results["split"] = raw(r)
    ud = torch.from_numpy(u).cuda()
    r = fresh()
    yd = r.run_torch(ud)
    torch.cuda.synchronize()
    assert np.array_equal(yd.cpu().numpy(), y)
    results["device"] = raw(r)
    r = fresh()
    r.run_device(ud.data_ptr(), 0, T, torch.cuda.current_stream().cuda_stream)
    results["device, y NULL"] = raw(r)
    r = fresh(True)
    r.lib.check(r.lib.L.acme_batch_run_sources(r.h, None, None, T, 1, torch.cuda.current_stream().cuda_stream))
    results["sourced, device, y NULL"] = raw(r)
    r = fresh()
    r.run_async(u, None)
    r.wait()
    results["async, y NULL"] = raw(r)
    r = fresh(True)
    r.run_sources_async(T)
    r.wait()
    results["sources async, y NULL"] = raw(r)
    monkeypatch.setenv("ACME_OS_SLICE", "1000")
    results["slices of 1000"] = raw(fresh().measure(u, time_major=True))
    monkeypatch.delenv("ACME_OS_SLICE")
    monkeypatch.setenv("ACME_MEAS_TABLE_BUDGET", "1")
    r = fresh(True)
    assert r.measurement_plan()["chunk"] == 64
    r.run_sources(t1)
    r.measure(T=T - t1)
    results["one-tile chunks, split, sourced"] = raw(r)
    for name, (out, count) in results.items():
        assert count == ref[1], name
        assert np.array_equal(out, ref[0]), name


def test_gpu_reset_rearming_and_set_matrices(hip_lib):
    from helpers import sweep_inputs
    from test_emu_parity import superover_models_with_their_own_diodes
    m = clipper()
    N = 70
    uc = clipper_u(N, 9000, f=2000.0)
    f_num = np.stack([np.array([1, 2, 3, 4, 5, 6, 7])[np.arange(N) % 7], np.full(N, 9)])
    coef = np.array([[1, 0], [0, 1], [1, -1]])
    kb = MT.bin_frequencies(coef, f_num, 44)
    r = runner(m, N).set_measurement_bins(coef, start=60, f_den=44, f_num=f_num)
    r.measure(np.ascontiguousarray(uc[:, :4000]), time_major=True)
    r.reset_measurement()
    r.measure(np.ascontiguousarray(uc[:, 4000:]), time_major=True)

    def shared():
        q = runner(m, N)
        q.run(np.ascontiguousarray(uc[:, :4000]), time_major=True)
        return q
    ref = MT.shared_by_bin(shared, lambda q: q.measure(np.ascontiguousarray(uc[:, 4000:]), time_major=True), 44, kb, dict(start=60))
    assert raw(r)[1] == 4940
    MT.assert_bin_by_bin(raw(r), kb, ref)
    r.set_measurement(f0=(2, 44), harmonics=2)
    assert r.lib.L.acme_batch_get_measurement_plan(r.h, None, None, None, None) == -1
    r.set_measurement_bins(coef, f_den=44, f_num=f_num)
    assert r.measurement_plan()["groups"] == 7
    models = superover_models_with_their_own_diodes(3, HS)
    us = np.ascontiguousarray(sweep_inputs("superover_var", 3, 600, seed=2).transpose(0, 2, 1))
    fn = np.array([[1, 2, 3], [5, 5, 4]])
    kb = MT.bin_frequencies(coef, fn, 30)

    def feed(r):
        r.run(np.ascontiguousarray(us[:, :250]), time_major=True)
        r.set_models(1, [models[0]])
        r.set_models(2, [models[2]])
        r.run(np.ascontiguousarray(us[:, 250:]), time_major=True)

    def batch():
        return runner(models[0], 3, models=[models[0]] * 3)
    r = batch().set_measurement_bins(coef, start=10, f_den=30, f_num=fn)
    feed(r)
    assert raw(r)[1] == 590
    MT.assert_bin_by_bin(raw(r), kb, MT.shared_by_bin(batch, feed, 30, kb, dict(start=10)))


def test_gpu_exact_moments_and_bins_on_the_pass_through_model(hip_lib):
    """f_den = 2^31 - 1 with tones next to it and at 0; the window 301 ... 8800 is three chunks of 4 096 with a ragged last
    tile; rows [0, 4] and the strided row [3] of a 5-output model; 77 instances in 6 groups: mixed waves"""
    N, T = 77, 9000
    base = np.array([[M31 - 1, 0, 1234567, M31 - 2, 5, 1], [M31 - 2, 0, 7654321, M31 - 1, 5, M31 - 1]])
    f_num = base[:, np.arange(N) % 6]
    coef = np.array([[1, 0], [0, 1], [1, -1], [-3, 2], [32767, -32767], [1, 1]])
    kb = MT.bin_frequencies(coef, f_num, M31)
    u = X.scaled_rows(np.random.default_rng(311), N, T, 5)
    m = X.wire_model(5, FS)
    worst = 0.0
    for rows in ([0, 4], [3]):
        r = runner(m, N).set_measurement_bins(coef, start=301, length=8500, f_den=M31, f_num=f_num, rows=rows)
        assert PI.wave_kinds(r)[1] > 0
        assert np.array_equal(r.run(u, time_major=True), u)
        out, count = raw(r)
        worst = max(worst, MT.check_exact_bins(out, count, u[:, 301:8801][:, :, rows], M31, kb))
    print(f"bins on the GPU: worst |error| / bound {worst:.2e}")


@pytest.mark.parametrize("name", ["rc_ladder", "sallenkey"])
def test_gpu_superposition_on_a_linear_model(hip_lib, name):
    """512 tone pairs, one instance each (F = N: the mixed loop)"""
    m = load(name)
    N = 512
    f1 = np.round(np.logspace(np.log10(30), np.log10(9000), N)).astype(np.int64)
    f2 = f1 + 1000 + 7 * np.arange(N)
    pairs = np.stack([f1, f2])
    kb = MT.bin_frequencies(np.array([[1, 0], [0, 1], [1, 1], [-1, 1], [2, -1], [-1, 2]]), pairs, FS)
    keep = np.ones(N, dtype=bool)
    for j in range(2):                                    # (drop pairs where a product or a mirror falls on a tone)
        for t in (pairs[j], FS - pairs[j]):
            keep &= ~(kb[2:] == t).any(axis=0)
    pairs = pairs[:, keep]
    assert pairs.shape[1] > 400
    rng = np.random.default_rng(5)
    amps = 10.0 ** rng.uniform(-1, 0.5, pairs.shape)
    worst = MT.check_superposition(runner, m, name, FS, pairs, amps)
    print(f"{name}: {pairs.shape[1]} tone pairs, worst error {worst:.3e} of BODE_ATOL x the tones' amplitudes")


# ---- at width -------------------------------------------------------------------------------------------------------------------
def test_gpu_headline_grid_as_a_ccif_run(hip_lib):
    """The headline grid's shape: 8 192 instances of superover (caching solver stack), one second at 44.1 kHz, the CCIF pair
    19 kHz + 20 kHz at levels spread over 40 dB on the signal row, the grid's pots as CONST rows, B = 8 bins, y = NULL,
    device memory.  A contiguous quarter of the grid run through acme_batch_run on its rendered u measures the same, with ==."""
    import torch
    from acme_jl_amd.model import CachingHomotopySolver
    m = load("superover_var", CachingHomotopySolver)
    N, T, Q = 8192, FS, 2048
    idx = np.arange(N)
    pots = np.stack([(idx // 256) / float(N // 256), ((idx // 16) % 16) / 15.0, (idx % 16) / 15.0], axis=1)
    amp = 0.5 * 10.0 ** (-2.0 + 2.0 * ((idx * 2654435761) % N) / (N - 1.0))
    coef = np.array([[1, 0], [0, 1], [-1, 1], [2, -1], [-1, 2], [1, 1], [3, -2], [-2, 3]])
    f_num = np.array([[19000], [20000]])

    def arm(r, lo, hi, sourced=True):
        if sourced:
            r.set_source(0, "multisine", f_den=FS, f_num=[19000, 20000], amp=np.stack([amp[lo:hi]] * 2))
            for c in range(3):
                r.set_source(1 + c, "const", offset=pots[lo:hi, c])
        return r.set_measurement_bins(coef, f_den=FS, f_num=f_num)
    st = torch.cuda.current_stream().cuda_stream
    full = arm(runner(m, N), 0, N)
    full.lib.check(full.lib.L.acme_batch_run_sources(full.h, None, None, T, 1, st))
    torch.cuda.synchronize()
    got, count = raw(full)
    rep = full.report_arrays()
    assert count == T and full.source_clock == T
    lo = 3 * Q
    part = arm(runner(m, Q), lo, lo + Q)
    ud = torch.empty((Q, T, 4), dtype=torch.float64, device="cuda")
    part.lib.check(part.lib.L.acme_batch_render_sources(part.h, None, ud.data_ptr(), T, 1, st))
    twin = arm(runner(m, Q), lo, lo + Q, sourced=False)
    twin.lib.check(twin.lib.L.acme_batch_run(twin.h, ud.data_ptr(), None, T, 1, st))
    torch.cuda.synchronize()
    want, count2 = raw(twin)
    assert count2 == T
    assert np.isfinite(want).all() and np.abs(want[:, 0, 4:6]).max() > 1e-3
    assert np.array_equal(got[lo:lo + Q], want)
    rt = twin.report_arrays()
    assert np.array_equal(rep["n_warn"][lo:lo + Q], rt["n_warn"]) and np.array_equal(rep["iters_total"][lo:lo + Q], rt["iters_total"])
    u0 = ud[:3, :5].cpu().numpy()
    assert np.array_equal(u0[:, :, 1:], np.broadcast_to(pots[lo:lo + 3, None, :], (3, 5, 3)))
    k = dict(f_den=FS, f_num=np.array([19000, 20000]), amp=np.stack([amp[lo:lo + 3]] * 2))
    MT.check_multisine_row(u0[:, :, 0], k, 3, 0, [(i, t) for i in range(3) for t in range(5)])
    imd = full.measurement().imd([0, 1], [2, 3, 4])
    print(f"CCIF IMD over the grid: median {np.median(imd):.4e}, max {imd.max():.4e}")
