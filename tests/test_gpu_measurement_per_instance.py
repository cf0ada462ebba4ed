"""Per-instance measurement fundamentals (acme_batch_set_measurement_per_instance) on the MI355X: the two inner loops of
acme_meas_pi_kernel themselves -- uniform waves broadcast their group's table row (v_readlane), mixed waves load their
lanes' own rows 16 bytes at a time -- which the CPU emulator only walks as plain loops.

Which case runs which loop (the plan says so, and the tests assert it):
  A  every f_num equal                     uniform waves only
  B  F = 1                                 uniform only;   F = 3 (200 / 7 / 1)   3 uniform + 1 mixed
     F = N = 130                           mixed only;     fastest / slowest axis   3 uniform + 1 mixed
  D  6 frequencies over 77 instances       mixed (no group reaches 64 pairs)
  F  2 048 log-spaced frequencies          mixed at width
  G  32 frequencies x 32 cells each        mixed at width (32 pairs a group: no whole wave)"""
from fractions import Fraction

import numpy as np
import pytest

import exact_ref as X
import measure_pi_ref as PI
from helpers import FS, HS, load, sweep_inputs
from test_measurement import birdie_u, clipper, clipper_u, raw, two_output_clipper
from test_measurement_per_instance import M31, _freq_cases

pytestmark = pytest.mark.gpu


def runner(model, n, **kw):
    from acme_jl_amd.runner import ModelRunner
    return ModelRunner(model, n, device=0, **kw)


# ---- A ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [0, 1, 10, 17, 32])
def test_gpu_equal_frequencies_reduce_to_the_shared_measurement(hip_lib, H):
    for m, N, rows in ((clipper(), 131, None), (two_output_clipper(), 99, None), (two_output_clipper(), 99, [1])):
        u = clipper_u(N, 9000)                                  # (three chunks of 4 096 samples, the last tile ragged)
        spec = dict(start=301, length=8500, harmonics=H, rows=rows)
        rs = runner(m, N).set_measurement(f0=(10, 441) if H else None, **spec)
        y = rs.run(u, time_major=True)
        rp = runner(m, N).set_measurement(f_den=441, f_num=np.full(N, 10), **spec)
        assert np.array_equal(rp.run(u, time_major=True), y)
        (a, ca), (b, cb) = raw(rs), raw(rp)
        assert ca == cb == 8500 and (N * a.shape[1]) % 64 != 0
        assert np.array_equal(a, b), (H, N, rows, np.argwhere(a != b)[:8])
        assert PI.wave_kinds(rp)[1] == 0


# ---- B ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(_freq_cases()))
def test_gpu_each_instance_is_the_shared_measurement_at_its_frequency(hip_lib, name):
    f_num, kinds = _freq_cases()[name]
    N, T, f_den = len(f_num), 4300, 441                         # (two chunks; 4 297 = 67 x 64 + 9 samples measured)
    m = clipper()
    u = clipper_u(N, T)
    spec = dict(start=3, harmonics=10)
    r = runner(m, N).set_measurement(f_den=f_den, f_num=f_num, **spec)
    assert PI.wave_kinds(r) == kinds
    r.measure(u, time_major=True)
    ref = PI.shared_by_frequency(lambda: runner(m, N), lambda q: q.measure(u, time_major=True), f_den, f_num, spec)
    PI.assert_instance_by_instance(raw(r), f_num, ref)


def test_gpu_each_instance_two_outputs_h17(hip_lib):
    m = two_output_clipper()
    N, T, f_den = 70, 1000, 441
    f_num = np.array([10] * 33 + [20] * 30 + [30] * 7)[np.random.default_rng(4).permutation(N)]
    u = clipper_u(N, T)
    spec = dict(start=7, harmonics=17)                          # (two unit groups along grid.y, an idle wave)
    r = runner(m, N).set_measurement(f_den=f_den, f_num=f_num, **spec)
    assert PI.wave_kinds(r) == (2, 1)
    r.measure(u, time_major=True)
    ref = PI.shared_by_frequency(lambda: runner(m, N), lambda q: q.measure(u, time_major=True), f_den, f_num, spec)
    PI.assert_instance_by_instance(raw(r), f_num, ref)


# ---- C ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
def test_gpu_memory_paths_slices_split_calls_and_budget_are_bit_identical(hip_lib, monkeypatch, k):
    import torch
    from acme_jl_amd import examples
    from acme_jl_amd.model import DiscreteModel
    if k == 1:
        m = load("birdie_var", HS)
        N, T, t1 = 130, 9000, 4133
        u = birdie_u(N, T)
    else:
        m = DiscreteModel(examples.diodeclipper(), Fraction(1, k * FS), HS)
        N, T, t1 = 130, 9000, 4133
        u = clipper_u(N, T)
    # 26 pairs a group, no whole wave: the 130 remainders make two mixed waves (26 + 26 + 12, 14 + 26 + 24) and the last 2
    # pairs of the fifth group a wave of their own (uniform)
    f_num = np.array([10, 20, 30, 40, 50])[np.arange(N) % 5]
    spec = dict(start=100, length=8000, f_den=441, f_num=f_num, harmonics=12)

    def fresh():
        return runner(m, N).set_oversampling(k).set_measurement(**spec)
    r = fresh()
    assert PI.wave_kinds(r) == (1, 2)
    y = r.run(u, time_major=True)
    ref = raw(r)
    assert ref[1] == 8000 and np.isfinite(y).all()
    results = {"y NULL": raw(fresh().measure(u, time_major=True))}
    r = fresh()
    r.run(np.ascontiguousarray(u[:, :t1]), time_major=True)
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
    if k == 1:
        uv, uc = np.ascontiguousarray(u[:, :, :1]), np.ascontiguousarray(u[:, 0, :])
        r = fresh()
        assert np.array_equal(r.run_const(uv, uc, [1]), y)
        results["run_const"] = raw(r)
        results["run_const, y NULL"] = raw(fresh().measure_const(uv, uc, [1]))
    r = fresh()
    r.run_async(u, None)
    r.wait()
    results["async, y NULL"] = raw(r)
    monkeypatch.setenv("ACME_OS_SLICE", "1000")
    results["slices of 1000"] = raw(fresh().measure(u, time_major=True))
    monkeypatch.delenv("ACME_OS_SLICE")
    monkeypatch.setenv("ACME_MEAS_TABLE_BUDGET", "1")
    r = fresh()
    assert r.measurement_plan()["chunk"] == 64
    r.run(np.ascontiguousarray(u[:, :t1]), time_major=True)
    r.measure(np.ascontiguousarray(u[:, t1:]), time_major=True)
    results["one-tile chunks, split"] = raw(r)
    for name, (out, count) in results.items():
        assert count == ref[1], name
        assert np.array_equal(out, ref[0]), name


def test_gpu_run_sources_reset_and_set_matrices(hip_lib):
    from test_emu_parity import superover_models_with_their_own_diodes
    m = load("birdie_var", HS)
    N, T, f_den = 70, 5000, 441
    f_num = np.array([10, 20, 30, 40, 50, 60, 70])[np.arange(N) % 7]

    def fresh():
        r = runner(m, N)
        r.set_source(0, "sine", amp=np.logspace(-2, 0, N), f_den=f_den, f_num=f_num)
        r.set_source(1, "const", offset=np.linspace(0.1, 0.9, N))
        return r.set_measurement(start=60, harmonics=5, f0_from_source=0)
    r = fresh()
    u = r.render_sources(T)
    y = r.run_sources(T)
    ref = raw(r)
    assert np.array_equal(raw(fresh().measure(T=T))[0], ref[0])
    rr = runner(m, N).set_measurement(start=60, harmonics=5, f_den=f_den, f_num=f_num)
    assert np.array_equal(rr.run(u, time_major=True), y)
    assert np.array_equal(raw(rr)[0], ref[0])
    # reset: the clock restarts, the frequencies stay
    rr.reset_measurement()
    q = runner(m, N)
    q.run(u, time_major=True)
    q.set_measurement(start=60, harmonics=5, f_den=f_den, f_num=f_num)
    u2 = np.ascontiguousarray(u[:, :3000])
    rr.measure(u2, time_major=True)
    q.measure(u2, time_major=True)
    assert raw(rr)[1] == 2940 and np.array_equal(raw(rr)[0], raw(q)[0])
    # set_matrices rebuilds the batch: accumulators, clock and frequencies go with it
    models = superover_models_with_their_own_diodes(3, HS)
    us = np.ascontiguousarray(sweep_inputs("superover_var", 3, 600, seed=2).transpose(0, 2, 1))
    fn = np.array([1, 2, 3])
    spec = dict(start=10, harmonics=3)

    def feed(r):
        r.run(np.ascontiguousarray(us[:, :250]), time_major=True)
        r.set_models(1, [models[0]])
        r.set_models(2, [models[2]])
        r.run(np.ascontiguousarray(us[:, 250:]), time_major=True)

    def batch():
        return runner(models[0], 3, models=[models[0]] * 3)
    r = batch().set_measurement(f_den=30, f_num=fn, **spec)
    feed(r)
    assert raw(r)[1] == 590
    PI.assert_instance_by_instance(raw(r), fn, PI.shared_by_frequency(batch, feed, 30, fn, spec))


# ---- D ------------------------------------------------------------------------------------------------------------------------
def test_gpu_exact_moments_and_harmonics_per_instance(hip_lib):
    """f_den = 2^31 - 1, f_num next to it and 0; the window 301 ... 8800 is three chunks of 4 096 with a ragged last tile;
    rows [0, 4] and the strided row [3] of a 5-output model; P = 154 and 77 pairs, not multiples of 64."""
    N, T, H = 77, 9000, 4
    f_num = np.array([M31 - 1, 0, 1234567, M31 - 2, 1, 3])[np.arange(N) % 6]
    u = X.scaled_rows(np.random.default_rng(311), N, T, 5)
    m = X.wire_model(5, FS)
    worst = 0.0
    for rows in ([0, 4], [3]):
        r = runner(m, N).set_measurement(start=301, length=8500, f_den=M31, f_num=f_num, harmonics=H, rows=rows)
        assert PI.wave_kinds(r)[1] > 0
        assert np.array_equal(r.run(u, time_major=True), u)
        out, count = raw(r)
        worst = max(worst, PI.check_exact_per_instance(out, count, u[:, 301:8801][:, :, rows], M31, f_num, H))
    print(f"per-instance harmonics on the GPU: worst |error| / bound {worst:.2e}")


def test_gpu_window_far_from_the_start(hip_lib):
    """a window that starts beyond 2^20 samples (reached by y = NULL runs of constant input): bit for bit the same window at
    the start of a fresh batch, which is held to the references"""
    N, lead, n, H = 5, 2 ** 20 + 77, 4133, 4
    f_num = np.array([M31 - 1, 0, 1234567, M31 - 2, 1])
    u = X.scaled_rows(np.random.default_rng(8), N, n + 40, 3)
    m = X.wire_model(3, FS)
    const = np.ascontiguousarray(np.broadcast_to(u[:, :1], (N, 2 ** 16, 3)))
    r = runner(m, N).set_measurement(start=lead, length=n, f_den=M31, f_num=f_num, harmonics=H)
    done = 0
    while done < lead - 20:
        step = min(2 ** 16, lead - 20 - done)
        r.measure(np.ascontiguousarray(const[:, :step]), time_major=True)
        done += step
    r.measure(u, time_major=True)
    far = raw(r)
    q = runner(m, N).set_measurement(start=0, length=n, f_den=M31, f_num=f_num, harmonics=H)
    q.measure(np.ascontiguousarray(u[:, 20:]), time_major=True)
    out, count = raw(q)
    assert far[1] == count == n and np.array_equal(far[0], out)
    PI.check_exact_per_instance(out, count, u[:, 20:20 + n], M31, f_num, H)


# ---- F ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rc_ladder", "sallenkey"])
def test_gpu_bode_plot_in_one_batch_against_the_transfer_function(hip_lib, name):
    """2 048 log-spaced integer frequencies 10 Hz ... 22 kHz, one instance each (F ~ N: the mixed loop at width);
    |A_1 - expected| <= 1e-12 absolute, as on the emulator."""
    m = load(name)
    f_den, S, N = FS, PI.BODE_START[name], 2048
    f_num = np.round(np.logspace(1, np.log10(22000), N)).astype(np.int64)
    r = runner(m, N)
    a1 = PI.bode_measured(r, f_den, f_num, S)
    uniform, mixed = PI.wave_kinds(r)
    assert mixed >= 24 and r.measurement_plan()["groups"] == len(np.unique(f_num))
    err = np.abs(a1 - PI.bode_expected(m, f_den, f_num, S))
    print(f"{name}: {len(np.unique(f_num))} distinct frequencies, {uniform} uniform / {mixed} mixed waves, "
          f"max |A_1 - expected| {err.max():.2e} at {f_num[err.argmax()]} Hz")
    assert err.max() <= PI.BODE_ATOL, (err.max(), f_num[err.argmax()])


# ---- G ------------------------------------------------------------------------------------------------------------------------
def test_gpu_frequency_response_grid_at_width_without_outputs(hip_lib):
    """the superover grid of test_gpu_headline_shaped_sweep_without_outputs with the tone axis turned into 32 per-instance
    frequencies: sources on every row, H = 8, y = NULL, one second.  A quarter of the instances -- those of 8 of the 32
    frequencies -- against the shared measurement, one acme_batch_run per frequency on the rendered input."""
    m = load("superover_var")
    N, T, f_den, H = 1024, FS, FS, 8
    pots = sweep_inputs("superover_var", N, 1)[:, 1:, 0]                   # [N, 3]
    tones = np.round(np.logspace(np.log10(50), np.log10(5000), 32)).astype(np.int64)
    f_num = tones[np.arange(N) % 32]                                        # (frequency the fastest axis)

    def sourced(idx):
        r = runner(m, len(idx))
        r.set_source(0, "sine", f_den=f_den, f_num=f_num[idx])
        for k in range(3):
            r.set_source(1 + k, "const", offset=pots[idx, k])
        return r
    everyone = np.arange(N)
    r = sourced(everyone).set_measurement(harmonics=H, f0_from_source=0)
    assert PI.wave_kinds(r) == (0, 16) and r.measurement_plan()["groups"] == 32      # 32 pairs a group: no whole wave
    r.measure(T=T)
    out, count = raw(r)
    assert count == T and np.isfinite(out).all()
    quarter = np.flatnonzero(np.isin(f_num, tones[::4]))
    assert len(quarter) == N // 4
    u = sourced(quarter).render_sources(T)                                  # [N / 4, T, 4]
    for f in tones[::4]:
        q = runner(m, len(quarter)).set_measurement(f0=(int(f), f_den), harmonics=H)
        q.measure(u, time_major=True)
        o, c = raw(q)
        mine = f_num[quarter] == f
        assert c == count and np.array_equal(o[mine], out[quarter[mine]]), int(f)
