"""Shared by the emulator and GPU tests of the measurement weighting (acme_batch_set_measurement_weighting): the reference
every weighted measurement is held to -- a loop over time in numpy, vectorised over the pairs, in exactly the contract's
operation order, on the stored y of an identical run without a weighting -- and the checks, each taking ``mk(model, n)``,
which makes a fresh runner on the library under test (the emulator's or the GPU's).

The weighted samples themselves are read with ``==``: a fold whose period is not shorter than the window puts every window
sample into a slot of its own, so its sums ARE w.  The replay's w then goes through the existing replays (exact_ref's moments,
fold_ref, spectrum_ref, cross_ref, target_ref), every chain compared with ``==``, the harmonics within exact_ref's bound
applied to w."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest

import cross_ref as CR
import exact_ref as X
import fold_ref as FR
import source_ref as sr
import spectrum_ref as SR
import target_ref as TR
from helpers import FS, HS
from test_measurement import clipper, clipper_u, raw, two_output_clipper

MAX_SECTIONS = 8
IDENTITY, DELAY, BINOMIAL, RUNNING_SUM = [1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [1, 2, 1, 0, 0], [1, 0, 0, -1, 0]


def replay(y, sos):
    """the contract on y [N, T, nrows], the rows' samples since arming: w [N, T, nrows], from rest"""
    sos = np.asarray(sos, dtype=np.float64).reshape(-1, 5)
    N, T, nrows = y.shape
    w = np.empty_like(y)
    s1, s2 = np.zeros((len(sos), N, nrows)), np.zeros((len(sos), N, nrows))
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            x = y[:, t]
            for k, (b0, b1, b2, a1, a2) in enumerate(sos):
                v = b0 * x + s1[k]
                s1[k] = (b1 * x - a1 * v) + s2[k]
                s2[k] = b2 * x - a2 * v
                x = v
            w[:, t] = x
    return w


def stable_sos(S, seed=0):
    """S sections with random zeros and poles, the poles of radius <= 0.95 (complex pairs and real ones)"""
    rng = np.random.default_rng(100 * S + seed)
    out = []
    for k in range(S):
        def quad():
            if rng.random() < 0.7:
                rad, th = rng.uniform(0.2, 0.95), rng.uniform(0.0, np.pi)
                return -2.0 * rad * np.cos(th), rad * rad
            p, q = rng.uniform(-0.95, 0.95, 2)
            return -(p + q), p * q
        a1, a2 = quad()
        z1, z2 = quad()
        g = rng.uniform(0.5, 1.5)
        out.append([g, g * z1, g * z2, a1, a2])
    return np.array(out)


def cascades():
    """the cascades of the geometry: S = 1, 2, 3, 8 random stable sections and the A weighting at 44.1 kHz"""
    from acme_jl_amd.runner import weighting_sos
    c = {f"S = {S}": stable_sos(S) for S in (1, 2, 3, 8)}
    c["A"] = weighting_sos("A", 44100)
    return c


def window(a, start, length=0):
    end = a.shape[1] if not length else min(a.shape[1], start + length)
    return a[:, start:end]


def got_w(r):
    """the weighted window sample by sample, [N, count, nrows]: the sums of a fold whose period holds the window"""
    f = r.measurement_fold(raw=True)
    assert f.count <= f.mean.shape[2], (f.count, f.mean.shape)
    return np.ascontiguousarray(f.mean[:, :, :f.count].transpose(0, 2, 1))


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def assert_moments(got, ww, f0=None, H=0, some=None):
    """the base measurement ``got`` (raw) against exact_ref on the weighted window ww [N, count, nrows]: the count, min and max
    of every pair; sum and sq as the header's chains, and the harmonics within exact_ref.harmonic_bound, of the instances
    ``some`` (exact_ref walks them in Python)"""
    out, count = got
    assert count == ww.shape[1]
    with np.errstate(invalid="ignore"):
        nan = np.isnan(ww).any(axis=1)
        assert np.array_equal(out[:, :, 2], np.where(nan, np.nan, ww.min(axis=1)), equal_nan=True)
        assert np.array_equal(out[:, :, 3], np.where(nan, np.nan, ww.max(axis=1)), equal_nan=True)
    some = list(range(ww.shape[0]))[:3] if some is None else some
    s, sq, _, _ = X.exact_moments(ww[some])
    mean, rms = X.reported((s, sq), count)
    assert np.array_equal(out[some][:, :, 0], mean, equal_nan=True) and np.array_equal(out[some][:, :, 1], rms, equal_nan=True)
    if H:
        Cw, Sw, l1 = X.ld_harmonics(ww[some], f0, H)
        Cg, Sg = X.unscale(out[some], count)
        bound = X.harmonic_bound(count, l1)[:, :, None]
        assert (np.abs(Cg - Cw) <= bound).all() and (np.abs(Sg - Sw) <= bound).all()


# ---- 1. exact pins ------------------------------------------------------------------------------------------------------------
def _wire_int(N, T, lim, seed=11):
    ui = np.random.default_rng(seed).integers(-lim, lim + 1, (N, T))
    return ui, np.ascontiguousarray(ui.astype(np.float64)[:, :, None])


def _every_form(r, P, tgt):
    return r.set_measurement_fold(P).set_measurement_spectrum(64, 32).set_measurement_cross(0, 64, 32).set_measurement_target(
        tgt, preemphasis=0.5)


def _read_every_form(r):
    return (raw(r)[0], np.array(raw(r)[1]), *FR.got_fold(r)[:2], *SR.got_spec(r)[:2], *CR.got_cross(r)[:2], TR.got_target(r)[0])


def check_identity(mk, N=5, T=4000, start=37):
    """[1, 0, 0, 0, 0]: every result of every form == the unweighted measurement's, and the series'"""
    ui, u = _wire_int(N, T, 1024)
    m = X.wire_model(1, FS)
    tgt = TR.table(3, 1, 1, 77)
    arm = lambda: _every_form(mk(m, N).set_measurement(start=start, f0=(10, 441), harmonics=3), 441, tgt)
    a, b = arm(), arm().set_measurement_weighting([IDENTITY])
    assert np.array_equal(a.run(u, time_major=True), u) and np.array_equal(b.run(u, time_major=True), u)
    assert same(_read_every_form(a), _read_every_form(b))
    ser = lambda: mk(m, N).set_measurement(start=start, f0=(10, 441), harmonics=3).set_measurement_series(400, 400, 3)
    a, b = ser(), ser().set_measurement_weighting([IDENTITY])
    a.measure(u, time_major=True)
    b.measure(u, time_major=True)
    sa, sb = a.measurement_series(), b.measurement_series()
    assert np.array_equal(sa.counts, sb.counts) and sa.complete == 3 and all(
        np.array_equal(getattr(sa, k), getattr(sb, k)) for k in ("mean", "rms", "min", "max", "harmonics"))


def check_integer_pins(mk, case, N=5, T=4000, start=37):
    """small integers through the pass-through model: w from Python integers, independent of any replay -- a one-sample delay
    (also across a call split), 1 + 2 z^-1 + z^-2, a running sum, eight delays in cascade; and the moments of w"""
    sos, lim, want = {"delay": ([DELAY], 1024, lambda y, m: y[m - 1] if m >= 1 else 0),
                      "delay, split": ([DELAY], 1024, lambda y, m: y[m - 1] if m >= 1 else 0),
                      "1 2 1": ([BINOMIAL], 1024, lambda y, m: y[m] + 2 * (y[m - 1] if m >= 1 else 0) + (y[m - 2] if m >= 2 else 0)),
                      "running sum": ([RUNNING_SUM], 16, None),
                      "8 delays": ([DELAY] * 8, 1024, lambda y, m: y[m - 8] if m >= 8 else 0)}[case]
    ui, u = _wire_int(N, T, lim)
    r = mk(X.wire_model(1, FS), N).set_measurement(start=start).set_measurement_fold(T).set_measurement_weighting(sos)
    if case == "delay, split":
        cut = start + 64
        assert np.array_equal(r.run(np.ascontiguousarray(u[:, :cut]), time_major=True), u[:, :cut])
        r.measure(np.ascontiguousarray(u[:, cut:]), time_major=True)
    else:
        assert np.array_equal(r.run(u, time_major=True), u)           # a stored y stays the raw output
    w, (out, count) = got_w(r), raw(r)
    assert count == T - start and w.shape == (N, T - start, 1)
    for i in range(N):
        y = [int(v) for v in ui[i]]
        if want is None:
            wi, acc = [], 0
            for v in y:
                acc += v
                wi.append(acc)
        else:
            wi = [want(y, m) for m in range(T)]
        wi = wi[start:]
        assert w[i, :, 0].tolist() == [float(v) for v in wi], (case, i)
        s, q = sum(wi), sum(v * v for v in wi)
        assert abs(s) < 2 ** 52 and q < 2 ** 52
        mean, rms = X.reported((np.float64(s), np.float64(q)), count)
        assert out[i, 0].tolist() == [mean, rms, float(min(wi)), float(max(wi))], (case, i)


# ---- 2. geometry --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plain_run(mk, two, N, T):
    """the run without a weighting every case of a shape shares: (model, u, y); never modified"""
    if two:
        m, u = two_output_clipper(), clipper_u(N, T)
    else:
        m, u = TR.wire_data(N, T)
    return m, u, mk(m, N).run(u, time_major=True)


@functools.lru_cache(maxsize=None)
def _weighted(mk, two, N, T, name):
    """the replay on that run's y, all rows, and the package's own host replay (item 7 c): (w [N, T, ny]); never modified"""
    from acme_jl_amd.runner import MeasurementWeighting
    y = _plain_run(mk, two, N, T)[2]
    w = replay(y, cascades()[name])
    assert np.array_equal(MeasurementWeighting(cascades()[name]).apply(y.transpose(0, 2, 1)).transpose(0, 2, 1), w)
    return w


def check_geometry(mk, N, T, start, name, rows=None, two=False, H=2):
    """one weighted run with every form that fits on one measurement: the stored y, w itself, and every form on w"""
    m, u, y = _plain_run(mk, two, N, T)
    sos = cascades()[name]
    cols = list(range(y.shape[2])) if rows is None else rows
    ww = np.ascontiguousarray(window(_weighted(mk, two, N, T, name), start)[:, :, cols])
    tgt = TR.table(7, 2, len(cols), 97)
    which, lag = np.arange(N) % 2, (7 * np.arange(N)) % 97
    r = mk(m, N).set_measurement(start=start, f0=(10, 441), harmonics=H, rows=rows)
    r.set_measurement_fold(T - start).set_measurement_spectrum(128, 96).set_measurement_cross(0, 128, 96)
    r.set_measurement_target(tgt, which=which, lag=lag, preemphasis=TR.C_PATHS).set_measurement_weighting(sos)
    assert np.array_equal(r.measurement_weighting().sos, sos)
    assert np.array_equal(r.run(u, time_major=True), y)                 # a stored y stays the raw output
    assert np.isfinite(ww).all() and np.array_equal(got_w(r), ww), np.argwhere(got_w(r) != ww)[:6]
    assert_moments(raw(r), ww, (10, 441), H)
    FR.assert_fold(FR.got_fold(r), ww, T - start)
    SR.assert_spec(r, SR.got_spec(r), ww)
    CR.assert_cross(r, CR.got_cross(r), window(u, start)[:, :, 0], ww)  # (the input row stays unweighted)
    TR.assert_target(TR.got_target(r), ww, tgt, which, lag, TR.C_PATHS)


# ---- 3. every path ------------------------------------------------------------------------------------------------------------
def check_paths(mk, dev, k, T, monkeypatch, N=70, S0=3, P=97):
    """the pass-through model driven by what a per-instance sine source renders, oversampled by k, S = 3: w, the moments and
    a target's chains after every path == those after a host run with y stored, and w == the replay on that y"""
    m = X.wire_model(1, k * FS)
    src = dict(kind="sine", f_den=441, f_num=1 + np.arange(N) % 40, amp=np.logspace(-2, 0.7, N), phase=np.arange(N) % 441)
    sos = stable_sos(3, seed=k)
    tgt = TR.table(P + k, 2, 1, P)
    which, lag = np.arange(N) % 2, (7 * np.arange(N)) % P

    def fresh(sourced=False, pi=False):
        r = mk(m, N).set_oversampling(k)
        if sourced:
            r = sr.apply_sources(r, [src])
        if pi:      # (the per-instance form: its table's budget sets the chunk length)
            r.set_measurement(start=S0, f_den=441, f_num=1 + np.arange(N), harmonics=2)
        else:
            r.set_measurement(start=S0)
        r.set_measurement_fold(T).set_measurement_target(tgt, which=which, lag=lag, preemphasis=TR.C_PATHS)
        return r.set_measurement_weighting(sos)

    def read(r):
        out, count = raw(r)
        return got_w(r), out[:, :, :4], np.array(count), TR.got_target(r)[0]
    u = sr.apply_sources(mk(m, N).set_oversampling(k), [src]).render_sources(T)
    r = fresh()
    y = r.run(u, time_major=True)
    ref = read(r)
    assert np.isfinite(y).all()
    ww = window(replay(y, sos), S0)
    assert np.array_equal(ref[0], ww)
    TR.assert_target(TR.got_target(r), ww, tgt, which, lag, TR.C_PATHS)
    results = {"y NULL": read(fresh().measure(u, time_major=True))}
    # split calls: before the start, just behind it, inside a tile, on a tile, on a slice of 150 and on a chunk boundary
    for cut in sorted({c for c in (S0 - 1, S0 + 1, S0 + 40, S0 + 64, S0 + 150, S0 + 4096) if 0 < c < T}):
        r = fresh()
        assert np.array_equal(r.run(np.ascontiguousarray(u[:, :cut]), time_major=True), y[:, :cut])
        r.measure(np.ascontiguousarray(u[:, cut:]), time_major=True)
        results[f"split at {cut}"] = read(r)
    t1 = min(S0 + P + 40, T - 1)
    ud = dev.put(u)
    r = fresh()
    assert np.array_equal(dev.run(r, ud, True, T), y)
    results["device"] = read(r)
    r = fresh()
    dev.run(r, ud, False, T)
    results["device, y NULL"] = read(r)
    r = fresh()
    dev.run(r, dev.put(u[:, :t1]), False, t1)
    dev.run(r, dev.put(u[:, t1:]), False, T - t1)
    results["device, y NULL, split"] = read(r)
    r = fresh()
    ya = np.zeros_like(y)
    r.run_async(u, ya)
    r.wait()
    assert np.array_equal(ya, y)
    results["async"] = read(r)
    r = fresh()
    r.run_async(u, None)
    r.wait()
    results["async, y NULL"] = read(r)
    r = fresh(sourced=True)
    assert np.array_equal(r.run_sources(T), y)
    results["sources"] = read(r)
    results["sources, y NULL"] = read(fresh(sourced=True).measure(T=T))
    monkeypatch.setenv("ACME_OS_SLICE", "150")
    results["slices of 150"] = read(fresh().measure(u, time_major=True))
    r = fresh()
    assert np.array_equal(r.run(u, time_major=True), y)
    results["slices of 150, y stored"] = read(r)
    r = fresh()
    assert np.array_equal(dev.run(r, ud, True, T), y)
    results["slices of 150, device"] = read(r)
    # ... with chunks of one tile (the per-instance form under a table budget of one byte), the calls cut again
    monkeypatch.setenv("ACME_MEAS_TABLE_BUDGET", "1")
    b = fresh(pi=True)
    assert b.measurement_plan()["chunk"] == 64
    b.measure(np.ascontiguousarray(u[:, :t1]), time_major=True)
    b.measure(np.ascontiguousarray(u[:, t1:]), time_major=True)
    results["slices of 150, chunks of one tile, split"] = read(b)
    monkeypatch.delenv("ACME_MEAS_TABLE_BUDGET")
    monkeypatch.delenv("ACME_OS_SLICE")
    for name, got in results.items():
        assert same(got, ref), name
    if k > 1:
        return
    # run_const on a constant row against run on the materialised input
    uc = np.logspace(-2, 0.7, N)[:, None]
    r = fresh()
    yc = r.run(np.ascontiguousarray(np.broadcast_to(uc[:, None, :], (N, T, 1))), time_major=True)
    rc = fresh()
    assert np.array_equal(rc.run_const(np.zeros((N, T, 0)), uc, [0]), yc)
    rn = fresh().measure_const(np.zeros((N, T, 0)), uc, [0])
    for q in (rc, rn):
        assert same(read(q), read(r))


# ---- 4. coexistence -----------------------------------------------------------------------------------------------------------
def check_coexistence(mk, N, T, start=5):
    """single window + fold + spectrum + cross + target under one weighting, each against itself alone under it"""
    m, u = TR.wire_data(N, T)
    sos = stable_sos(3)
    tgt = TR.table(9, 2, 1, 77)
    which, lag = np.arange(N) % 2, np.arange(N) % 77
    arm = lambda: mk(m, N).set_measurement(start=start, f0=(10, 441), harmonics=3)
    adds = {"fold": lambda r: r.set_measurement_fold(50), "spectrum": lambda r: r.set_measurement_spectrum(64, 32),
            "cross": lambda r: r.set_measurement_cross(0, 64, 32),
            "target": lambda r: r.set_measurement_target(tgt, which=which, lag=lag, preemphasis=TR.C_PATHS)}
    reads = {"fold": lambda r: FR.got_fold(r)[0], "spectrum": lambda r: SR.got_spec(r)[0], "cross": lambda r: CR.got_cross(r)[0],
             "target": lambda r: TR.got_target(r)[0]}
    base = arm().set_measurement_weighting(sos)
    base.measure(u, time_major=True)
    every = arm()
    for add in adds.values():
        add(every)
    every.set_measurement_weighting(sos).measure(u, time_major=True)
    assert raw(every)[1] == raw(base)[1] and np.array_equal(raw(every)[0], raw(base)[0])
    plain = arm()
    plain.measure(u, time_major=True)
    assert not np.array_equal(raw(plain)[0], raw(base)[0])              # (the weighting is not a no-op here)
    for name, add in adds.items():
        alone = add(arm()).set_measurement_weighting(sos)
        alone.measure(u, time_major=True)
        assert np.array_equal(reads[name](alone), reads[name](every), equal_nan=True), name
        assert np.array_equal(raw(alone)[0], raw(base)[0]), name


def check_series_and_per_instance(mk, N, T, start=5):
    """a series and per-instance harmonics, each with a weighting: on the pass-through model both == the same form without
    a weighting fed the replay's w as its input.  The series: windows of 400 back to back and windows of 100 every 400 (a
    series takes no overlapping windows -- hop < win is refused --, so "win 400, hop 100" cannot be armed; the 400-sample
    blocks every 100 are put together from windows of 100, ``loudness(blocks=4)``)"""
    m, u = TR.wire_data(N, T)
    sos = stable_sos(2)
    w = replay(u, sos)
    for win, hop in ((400, 400), (100, 400), (100, 100)):
        W = (T - start - win) // hop + 2                                # (the last window incomplete)
        ser = lambda: mk(m, N).set_measurement(start=start, f0=(10, 441), harmonics=2).set_measurement_series(win, hop, W)
        a, b = ser().set_measurement_weighting(sos), ser()
        a.measure(u, time_major=True)
        b.measure(w, time_major=True)
        sa, sb = a.measurement_series(), b.measurement_series()
        assert np.array_equal(sa.counts, sb.counts) and 0 < sa.complete < W and sa.counts[-1] < win
        for k in ("mean", "rms", "min", "max", "harmonics"):        # (a window nothing has reached reads NaN in both)
            assert np.array_equal(getattr(sa, k), getattr(sb, k), equal_nan=True), k
        assert not np.array_equal(sa.rms, ser().measure(u, time_major=True).measurement_series().rms)
        assert np.array_equal(sa.loudness(), -0.691 + 10.0 * np.log10(sa.rms * sa.rms), equal_nan=True)
    # ... and four windows of 100 taken together are the window of 400 there (the same samples' mean square, rounded otherwise)
    four, whole = sa.loudness(blocks=4)[:W - 4], mk(m, N).set_measurement(start=start + 100, length=400).set_measurement_weighting(sos)
    whole.measure(u, time_major=True)
    assert four.shape[0] == W - 4 and np.allclose(four[1], whole.measurement().loudness(), rtol=0, atol=1e-9)
    f_num = 1 + np.arange(N) % 7
    pi = lambda: mk(m, N).set_measurement(start=start, f_den=441, f_num=f_num, harmonics=3)
    a, b = pi().set_measurement_weighting(sos), pi()
    a.measure(u, time_major=True)
    b.measure(w, time_major=True)
    assert raw(a)[1] == raw(b)[1] == T - start and np.array_equal(raw(a)[0], raw(b)[0])


# ---- 5. life cycle ------------------------------------------------------------------------------------------------------------
def check_life_cycle(mk, N=5, T=700, start=9):
    from acme_jl_amd.runner import AcmeError
    m, u = TR.wire_data(N, T)
    sos = stable_sos(3)
    fresh = lambda: mk(m, N).set_measurement(start=start).set_measurement_fold(T).set_measurement_weighting(sos)
    r = fresh()
    y = r.run(u, time_major=True)
    ww = window(replay(y, sos), start)
    first = (got_w(r), *raw(r))
    assert np.array_equal(first[0], ww)
    # reset and rerun: the states from 0.0, the coefficients kept -- bit for bit a fresh arming
    r.reset_measurement()
    assert raw(r)[1] == 0 and np.array_equal(r.measurement_weighting().sos, sos)
    r.measure(u, time_major=True)
    assert same((got_w(r), *raw(r)), first)
    # a weighting set again (after a reset: nothing has been fed) replaces the earlier one
    r.reset_measurement().set_measurement_weighting([DELAY])
    r.measure(u, time_major=True)
    assert np.array_equal(got_w(r), y[:, start - 1:T - 1])
    # re-arming and clear remove it
    L = r.lib.L
    r.set_measurement(start=start)
    with pytest.raises(AcmeError, match="no measurement weighting"):
        r.measurement_weighting()
    assert L.acme_batch_get_measurement_weighting(r.h, None, None) == -1 and "no measurement weighting" in L.acme_last_error().decode()
    r.measure(u, time_major=True)
    plain = mk(m, N).set_measurement(start=start)
    plain.measure(u, time_major=True)
    assert np.array_equal(raw(r)[0], raw(plain)[0])
    r.set_measurement(start=start).set_measurement_weighting(sos).clear_measurement()
    assert L.acme_batch_get_measurement_weighting(r.h, None, None) == -1 and "no measurement weighting" in L.acme_last_error().decode()
    with pytest.raises(AcmeError, match="no measurement is armed"):
        r.set_measurement_weighting(sos)


def check_set_matrices_carries_the_weighting(mk):
    from helpers import sweep_inputs
    from test_emu_parity import superover_models_with_their_own_diodes
    models = superover_models_with_their_own_diodes(3, HS)
    u = np.ascontiguousarray(sweep_inputs("superover_var", 3, 60, seed=2).transpose(0, 2, 1))
    sos = stable_sos(3)
    r = mk(models[0], 3, models=[models[0]] * 3).set_measurement(start=10).set_measurement_fold(50).set_measurement_weighting(sos)
    ya = r.run(np.ascontiguousarray(u[:, :25]), time_major=True)
    r.set_models(1, [models[0]])
    r.set_models(2, [models[2]])                            # (the batch moves to the plain shape: a new batch takes the measurement over)
    yb = r.run(np.ascontiguousarray(u[:, 25:]), time_major=True)
    assert np.array_equal(r.measurement_weighting().sos, sos)
    assert np.array_equal(got_w(r), window(replay(np.concatenate([ya, yb], axis=1), sos), 10))


def check_errors(mk):
    """every refusal with its code and the argument's name in the message"""
    from acme_jl_amd.runner import DimensionMismatch, _dp
    m, u = TR.wire_data(3, 10)

    def refused(r, what, sos, S):
        rc = r.lib.L.acme_batch_set_measurement_weighting(r.h, None if sos is None else _dp(sos), S)
        msg = r.lib.L.acme_last_error().decode()
        assert rc == -1 and all(w in msg for w in what), (S, rc, msg)
    one = np.ascontiguousarray(np.tile(np.array(IDENTITY, dtype=np.float64), (MAX_SECTIONS + 1, 1)))
    r = mk(m, 3)
    refused(r, ["no measurement is armed"], one, 1)
    r.set_measurement(start=1)
    refused(r, ["sos is null"], None, 1)
    for S in (0, -1, MAX_SECTIONS + 1):
        refused(r, ["S", str(MAX_SECTIONS)], one, S)
    for bad in (np.nan, np.inf, -np.inf):
        b = one.copy()
        b[1, 3] = bad
        refused(r, ["sos[1][3]", "not finite"], b, 2)
        r.lib.check(r.lib.L.acme_batch_set_measurement_weighting(r.h, _dp(b), 1))       # (beyond S: not read)
        r.set_measurement(start=1)
    assert r.lib.L.acme_batch_get_measurement_weighting(r.h, None, None) == -1      # (a refused weighting leaves none behind)
    r.measure(u, time_major=True)
    refused(r, ["samples have been fed"], one, 1)
    r.reset_measurement()
    # S = 8 is accepted and read back, with the rows beyond S of a shorter one 0.0
    r.set_measurement_weighting(one[:MAX_SECTIONS])
    out, S = np.full((MAX_SECTIONS, 5), 7.0), C.c_int(0)
    assert r.lib.L.acme_batch_get_measurement_weighting(r.h, _dp(out), C.byref(S)) == 0 and S.value == 8 and np.array_equal(out, one[:8])
    r.set_measurement_weighting(one[:2])
    assert r.lib.L.acme_batch_get_measurement_weighting(r.h, _dp(out), C.byref(S)) == 0 and S.value == 2 and not out[2:].any()
    # the Python layer's own refusals; scipy's six columns
    for bad in (np.zeros((MAX_SECTIONS + 1, 5)), np.zeros((2, 4)), np.zeros((0, 5)), np.zeros((1, 2, 5))):
        with pytest.raises(DimensionMismatch):
            r.set_measurement_weighting(bad)
    with pytest.raises(ValueError, match="a0"):
        r.set_measurement_weighting([[1, 0, 0, 2, 0, 0]])
    r.set_measurement_weighting([[3, 2, 1, 1, 0.5, 0.25]])
    assert r.measurement_weighting().sos.tolist() == [[3, 2, 1, 0.5, 0.25]]


def check_no_weighting_invariance(mk, N, T):
    """a batch armed without a weighting, and one armed after a weighting has been set and removed: the results and the run
    kernel's launches of the existing forms"""
    m, u = clipper(), clipper_u(N, T)
    f_num = np.array([10, 20, 30])[np.arange(N) % 3]
    sos = stable_sos(2)
    arms = {"shared": lambda r: r.set_measurement(start=5, f0=(10, 441), harmonics=10),
            "per instance": lambda r: r.set_measurement(start=5, f_den=441, f_num=f_num, harmonics=10),
            "bins": lambda r: r.set_measurement_bins(np.array([[1], [2], [3]]), start=5, f_den=441, f_num=f_num[None])}
    for name, arm in arms.items():
        a = arm(mk(m, N))
        y = a.run(u, time_major=True)
        b = arm(mk(m, N)).set_measurement_weighting(sos)
        arm(b)                                              # (arming removes the weighting)
        assert np.array_equal(b.run(u, time_major=True), y)
        c = arm(mk(m, N)).set_measurement_weighting(sos).clear_measurement()
        arm(c)
        assert np.array_equal(c.run(u, time_major=True), y)
        d = arm(mk(m, N)).set_measurement_weighting(sos)    # ... and with the weighting the run kernel's launches are the same
        assert np.array_equal(d.run(u, time_major=True), y)
        (oa, ca), (ob, cb), (oc, cc), (od, cd) = raw(a), raw(b), raw(c), raw(d)
        assert ca == cb == cc == cd == T - 5, name
        assert np.array_equal(oa, ob) and np.array_equal(oa, oc) and not np.array_equal(oa, od), name
        assert a.kernel_time()[1] == b.kernel_time()[1] == c.kernel_time()[1] == d.kernel_time()[1] > 0, name
        for q in (b, c):
            assert q.lib.L.acme_batch_get_measurement_weighting(q.h, None, None) == -1


# ---- 6. a non-finite instance -------------------------------------------------------------------------------------------------
def check_nan_instance(mk, N=3, T=50):
    """the recipe of test_measurement: a NaN in one instance's input.  Its pair reads NaN from there on, and the other
    instances are unaffected"""
    m, u = clipper(), clipper_u(N, T)
    u[1, 20, 0] = np.nan
    sos = stable_sos(3)
    r = mk(m, N).set_measurement().set_measurement_fold(T).set_measurement_weighting(sos)
    y = r.run(u, time_major=True, check=False)
    assert r.report_arrays()["first_nonfinite"].tolist()[1] >= 0
    w, ww = got_w(r), replay(y, sos)
    assert np.array_equal(w, ww, equal_nan=True)
    first = int(np.flatnonzero(np.isnan(y[1, :, 0]))[0])
    assert np.isnan(w[1, first:]).all() and np.isfinite(w[1, :first]).all() and np.isfinite(w[[0, 2]]).all()
    out, count = raw(r)
    assert count == T and np.isnan(out[1]).all() and np.isfinite(out[[0, 2]]).all()
    q = mk(m, N).set_measurement().set_measurement_fold(T).set_measurement_weighting(sos)   # ... and the same NaN-free run
    u[1, 20, 0] = u[1, 19, 0]
    q.run(u, time_major=True)
    assert np.array_equal(got_w(q)[[0, 2]], w[[0, 2]]) and np.array_equal(raw(q)[0][[0, 2]], out[[0, 2]])


# ---- 7. use level -------------------------------------------------------------------------------------------------------------
# ITU-R BS.1770-4, tables 1 and 2: the two stages of the K pre-filter at 48 kHz (b0 b1 b2 a1 a2)
BS1770_48K = np.array([[1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585],
                       [1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]])
IEC_POLES = (20.598997, 107.65265, 737.86223, 12194.217)


def analog_weighting(kind, f):
    """the analog prototype of IEC 61672 at the frequencies f (Hz), unscaled"""
    s = 2j * np.pi * np.asarray(f, dtype=np.float64)
    w1, w2, w3, w4 = (2.0 * np.pi * p for p in IEC_POLES)
    h = s * s / ((s + w1) ** 2 * (s + w4) ** 2)
    return h * s * s / ((s + w2) * (s + w3)) if kind == "A" else h


def check_loudness(mk, fs=48000, N=2, windows=6):
    """BS.1770: a 997 Hz sine of unit amplitude reads -3.01 LKFS -- the pass-through model, a sine source, the K weighting,
    blocks of 400 ms (19 200 samples) every 100 ms (4 800); every block from the third on (the high-pass has settled) within
    +-0.01.  A series refuses overlapping windows (hop < win), so the blocks are read the two ways the library has: block w
    as the single window armed at w hop (what a series' window is, bit for bit), and a series of back-to-back windows of
    100 ms with four of them taken together per block (``loudness(blocks=4)``)"""
    from acme_jl_amd.runner import weighting_sos
    win, hop = fs * 4 // 10, fs // 10
    T = win + (windows - 1) * hop
    sos = weighting_sos("K", fs)

    def arm():
        r = mk(X.wire_model(1, fs), N)
        r.set_source(0, "sine", f_den=fs, f_num=997, amp=np.ones(N))
        return r
    single = []
    for w in range(2, windows):
        r = arm().set_measurement(start=w * hop, length=win).set_measurement_weighting(sos)
        r.measure(T=T)
        m = r.measurement()
        assert m.count == win
        single.append(m.loudness())
    single = np.array(single)
    print("LKFS per block, single windows:", np.array2string(single[:, 0, 0], precision=4))
    assert single.shape == (windows - 2, N, 1) and (np.abs(single + 3.01) <= 0.01).all(), single[:, 0, 0]
    r = arm().set_measurement().set_measurement_series(hop, hop, T // hop).set_measurement_weighting(sos)
    r.measure(T=T)
    s = r.measurement_series()
    assert s.complete == T // hop
    lk = s.loudness(blocks=4)
    print("LKFS per block, series of 100 ms windows:", np.array2string(lk[:, 0, 0], precision=4))
    assert lk.shape == (windows, N, 1) and (np.abs(lk[2:] + 3.01) <= 0.01).all(), lk[:, 0, 0]
    assert np.allclose(lk[2:], single, rtol=0, atol=1e-9)
    return lk


def check_target_behind_a_weighting(mk, N=16, T=2100, best=7):
    """the diode clipper at N levels against the recording of instance ``best``, weighted on the host with ``.apply``; the
    run carries the same A weighting from rest, no lag: both sides see the same arithmetic from sample 0"""
    from acme_jl_amd.runner import weighting_sos
    m = clipper()
    src = dict(kind="sine", f_den=441, f_num=np.full(N, 10), amp=np.logspace(-1, 0.7, N))
    y = sr.apply_sources(mk(m, N), [src]).run_sources(T)
    r = sr.apply_sources(mk(m, N), [src]).set_measurement().set_measurement_weighting(weighting_sos("A", FS))
    r.set_measurement_target(r.measurement_weighting().apply(y[best, :, 0]))
    r.measure(T=T)
    mt = r.measurement_target()
    others = np.arange(N) != best
    assert mt.count == T and mt.see[best, 0] == 0.0 and (mt.see[others, 0] > 0).all() and int(np.argmin(mt.esr[:, 0])) == best
    return mt


# ---- 8. MultiDeviceRunner -----------------------------------------------------------------------------------------------------
def check_multi_device(mk, mk_md, N=70, T=1000, start=3):
    m, u = TR.wire_data(N, T)
    sos = stable_sos(3)
    one = mk(m, N).set_measurement(start=start).set_measurement_fold(T).set_measurement_weighting(sos)
    one.measure(u, time_major=True)
    md = mk_md(m, N).set_measurement(start=start)
    md.set_measurement_fold(T).set_measurement_weighting(sos).measure(u)
    assert np.array_equal(md.measurement_weighting().sos, sos)
    a, b = one.measurement(), md.measurement()
    assert a.count == b.count == T - start and all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("mean", "rms", "min", "max"))
    assert np.array_equal(one.measurement_fold(raw=True).mean, md.measurement_fold(raw=True).mean, equal_nan=True)
