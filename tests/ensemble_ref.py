"""Shared by the emulator and GPU tests of the measurement ensemble (acme_batch_set_measurement_ensemble): the reference every
ensemble is held to -- numpy on the stored y of an identical run without an ensemble, S and Q sequential float64 accumulations
over the members' axis from 0.0 (np.add.accumulate; the square a separate multiply), the extremes and their indices a plain
loop over the members in ascending instance order -- and the checks, each taking ``mk(model, n)``, which makes a fresh runner
on the library under test (the emulator's or the GPU's).  The four chains are compared bit for bit (the sign of a zero
included), the indices, ``members`` and ``filled`` with ``==``."""
import ctypes as C
import functools

import numpy as np
import pytest

import exact_ref as X
import source_ref as sr
from helpers import FS, HS
from test_measurement import clipper, clipper_u, raw, two_output_clipper

CAP = 16777216              # ACME_MAX_ENSEMBLE
START, LENGTH, T_GEO = 301, 8500, 9000      # the geometry's window: two chunk boundaries inside, a ragged last tile
STRIDES = [1, 3, 64, 4097]                  # recorded samples dense, sparse, one per tile, fewer than one per chunk
NAMES = ("sum", "sumsq", "min", "max")


def slots(length, stride):
    return (length - 1) // stride + 1


def replay(yw, groups, G, stride, E):
    """the contract on the window's samples so far yw [N, count, nrows]: a dict of the six arrays (G, nrows, E), ``members``
    (G,) and ``filled``; slots beyond ``filled`` and empty groups hold the start values"""
    N, count, nrows = yw.shape
    groups = np.zeros(N, dtype=np.int64) if groups is None else np.asarray(groups)
    rec = yw[:, ::stride]                                   # [N, filled, nrows]: window samples 0, stride, 2 stride, ...
    filled = rec.shape[1]
    assert filled <= E
    out = dict(sum=np.zeros((G, nrows, E)), sumsq=np.zeros((G, nrows, E)), min=np.full((G, nrows, E), np.inf),
               max=np.full((G, nrows, E), -np.inf), argmin=np.full((G, nrows, E), -1, dtype=np.int64),
               argmax=np.full((G, nrows, E), -1, dtype=np.int64), members=np.zeros(G, dtype=np.int64), filled=filled)
    for g in range(G):
        idx = np.flatnonzero(groups == g)                   # ascending instance order
        out["members"][g] = len(idx)
        if len(idx) == 0 or filled == 0:
            continue
        v = rec[idx]                                        # [M, filled, nrows]
        zero = np.zeros((1,) + v.shape[1:])
        with np.errstate(invalid="ignore", over="ignore"):
            q = v * v                                       # (a separate multiply, rounded on its own)
            out["sum"][g, :, :filled] = np.add.accumulate(np.concatenate([zero, v]), axis=0)[-1].T      # 0.0 + v0 + v1 ...
            out["sumsq"][g, :, :filled] = np.add.accumulate(np.concatenate([zero, q]), axis=0)[-1].T
            mn, mx = np.full(v.shape[1:], np.inf), np.full(v.shape[1:], -np.inf)
            imin, imax = np.full(v.shape[1:], -1, dtype=np.int64), np.full(v.shape[1:], -1, dtype=np.int64)
            for k, i in enumerate(idx):                     # the rule, member after member
                x = v[k]
                lo, hi = (x < mn) | (x != x), (x > mx) | (x != x)
                mn, imin = np.where(lo, x, mn), np.where(lo, i, imin)
                mx, imax = np.where(hi, x, mx), np.where(hi, i, imax)
        out["min"][g, :, :filled], out["max"][g, :, :filled] = mn.T, mx.T
        out["argmin"][g, :, :filled], out["argmax"][g, :, :filled] = imin.T, imax.T
    return out


def same_bits(a, b):
    """float64 arrays equal bit for bit, every NaN equal to every NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


def got(r):
    e = r.measurement_ensemble()
    return dict(sum=e.sum, sumsq=e.sumsq, min=e.min, max=e.max, argmin=e.argmin, argmax=e.argmax, members=e.members,
                filled=e.filled)


def same(a, b):
    return (all(same_bits(a[k], b[k]) for k in NAMES) and all(np.array_equal(a[k], b[k]) for k in ("argmin", "argmax", "members"))
            and a["filled"] == b["filled"])


def assert_ensemble(g, yw, groups, G, stride, E, what=""):
    want = replay(yw, groups, G, stride, E)
    assert g["filled"] == want["filled"], (what, g["filled"], want["filled"])
    assert np.array_equal(g["members"], want["members"]), (what, g["members"], want["members"])
    for k in NAMES:
        assert g[k].shape == want[k].shape, (what, k, g[k].shape, want[k].shape)
        assert same_bits(g[k], want[k]), (what, k, np.argwhere(~((g[k] == want[k]) | (np.isnan(g[k]) & np.isnan(want[k]))))[:6])
    for k in ("argmin", "argmax"):
        assert np.array_equal(g[k], want[k]), (what, k, np.argwhere(g[k] != want[k])[:6])
    return want


def window(y, start, length, rows=None):
    """the measured samples of the stored y [N, T, ny]: [N, count, nrows]"""
    return y[:, start:min(y.shape[1], start + length)][:, :, list(range(y.shape[2])) if rows is None else rows]


def wire_data(N, T, seed=0):
    return X.wire_model(1, FS), X.scaled_rows(np.random.default_rng(2000 + seed + N), N, T, 1)


def grouping(case, N):
    """(groups or None, G) of the cases' names"""
    if case == "one group":
        return None, 1
    if case == "interleaved":
        return np.arange(N) % 3, 3
    if case == "one member each":
        return np.arange(N), N
    if case == "blocks":        # contiguous blocks of 1, 63, 64 and 65 members (scaled down below N = 200), group 2 EMPTY,
        sizes = [1, 63, 64, 65] if N >= 200 else [1, 2, 1, 1]       # the instances left over in no group
        g, at = np.full(N, -1), 0
        for k, s in zip((0, 1, 3, 4), sizes):
            g[at:at + s] = k
            at += s
        assert at < N
        return g, 5
    raise KeyError(case)


# ---- 1. exact pins: integers, every product and sum exact ---------------------------------------------------------------------
def check_exact_pins(mk, T=300):
    """y = u through the pass-through model: S and Q from Python integers; a constructed tie (the lower index wins); a
    one-member group at -0.0 reads S = +0.0"""
    rng = np.random.default_rng(12)
    N = 6
    ui = rng.integers(-1024, 1025, (N, T))
    ui[1] = ui[0] + 5
    ui[2] = ui[0]                                           # instances 0 and 2 share group 0's minimum at every sample
    ui[4] = np.where(np.arange(T) % 2 == 0, ui[3], ui[3] - 7)       # ... 3 and 4 group 1's maximum at the even ones
    u = ui.astype(np.float64)
    u[5] = -0.0
    groups = [0, 0, 0, 1, 1, 2]
    r = mk(X.wire_model(1, FS), N).set_measurement(length=T).set_measurement_ensemble(groups)
    uu = np.ascontiguousarray(u[:, :, None])
    y = r.run(uu, time_major=True)
    assert np.array_equal(y, uu)
    e = r.measurement_ensemble()
    assert e.filled == T and e.members.tolist() == [3, 2, 1] and e.stride == 1 and e.rows == (0,)
    for g, idx in enumerate(([0, 1, 2], [3, 4])):
        for t in range(T):
            vals = [int(ui[i, t]) for i in idx]
            assert e.sum[g, 0, t] == float(sum(vals)) and e.sumsq[g, 0, t] == float(sum(v * v for v in vals)), (g, t)
            assert e.min[g, 0, t] == float(min(vals)) and e.max[g, 0, t] == float(max(vals)), (g, t)
    assert (e.argmin[0, 0] == 0).all() and (e.argmax[0, 0] == 1).all()          # the tie 0 / 2: the first member keeps it
    assert np.array_equal(e.argmax[1, 0], np.full(T, 3)) and np.array_equal(e.argmin[1, 0], np.where(np.arange(T) % 2 == 0, 3, 4))
    assert not np.signbit(e.sum[2, 0]).any() and not e.sum[2, 0].any() and not e.sumsq[2, 0].any()     # 0.0 + -0.0 = +0.0
    assert same_bits(e.min[2, 0], y[5, :, 0]) and same_bits(e.max[2, 0], y[5, :, 0])     # (min and max carry the stored value itself)
    assert (e.argmin[2, 0] == 5).all() and (e.argmax[2, 0] == 5).all()
    assert same_bits(e.trace(2), np.zeros((1, T)))
    assert_ensemble(got(r), y, groups, 3, 1, T)


# ---- 2. geometry, 3. groups, 4. rows -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plain_run(mk, two, N, T, start, length, rows):
    """the run without an ensemble every case of a shape shares: (model, u, y, raw measurement); never modified"""
    if two:
        m, u = two_output_clipper(), clipper_u(N, T)
    else:
        m, u = wire_data(N, T)
    r = mk(m, N).set_measurement(start=start, length=length, rows=None if rows is None else list(rows))
    y = r.run(u, time_major=True)
    return m, u, y, raw(r)


def check_geometry(mk, N, stride, case, T=T_GEO, start=START, length=LENGTH, rows=None, two=False, cuts=(2000, 6000)):
    """one call over the whole run (the window's chunks follow each other inside it), then three split calls with ``filled``
    after each; ``sum`` of one-member groups == 0.0 + the stored y"""
    m, u, y, plain = _plain_run(mk, two, N, T, start, length, None if rows is None else tuple(rows))
    groups, G = grouping(case, N)
    E = slots(length, stride)
    arm = lambda: mk(m, N).set_measurement(start=start, length=length, rows=rows).set_measurement_ensemble(groups, G, stride)
    r = arm()
    r.measure(u, time_major=True)
    with_ens = raw(r)
    assert with_ens[1] == plain[1] and np.array_equal(with_ens[0], plain[0])    # the measurement's own results
    whole = got(r)
    want = assert_ensemble(whole, window(y, start, length, rows), groups, G, stride, E, "one call")
    assert whole["filled"] == E
    if case == "blocks":
        assert want["members"][2] == 0 and not whole["sum"][2].any() and (whole["min"][2] == np.inf).all() \
            and (whole["max"][2] == -np.inf).all() and (whole["argmin"][2] == -1).all() and (whole["argmax"][2] == -1).all()
    if case == "one member each":
        yw = window(y, start, length, rows)[:, ::stride]                        # [N, E, nrows]
        assert same_bits(whole["sum"], (0.0 + yw).transpose(0, 2, 1))
        assert same_bits(whole["min"], yw.transpose(0, 2, 1)) and same_bits(whole["max"], yw.transpose(0, 2, 1))
        assert np.array_equal(whole["argmin"], np.broadcast_to(np.arange(N)[:, None, None], whole["argmin"].shape))
    r = arm()
    edges = [0, *cuts, T]
    for a, b in zip(edges[:-1], edges[1:]):
        r.measure(np.ascontiguousarray(u[:, a:b]), time_major=True)
        count = max(0, min(b, start + length) - start)
        g = got(r)
        assert g["filled"] == (slots(count, stride) if count else 0), (b, g["filled"])
        assert_ensemble(g, window(y[:, :b], start, length, rows), groups, G, stride, E, f"calls up to {b}")
    assert same(got(r), whole)
    return E


# ---- 5. paths -----------------------------------------------------------------------------------------------------------------
SOS = np.array([[0.5, 0.25, 0.125, -0.3, 0.1], [1.0, -1.0, 0.0, -0.995, 0.0]])


def check_paths(mk, dev, k, T, monkeypatch, stride, weighted=False, N=70, S=3, length=None):
    """the pass-through model driven by what a per-instance sine source renders, oversampled by k: the ensemble read after
    every path == that after a host run with y stored == the replay (``weighted``: of ``MeasurementWeighting.apply`` on the
    stored y).  ``dev``: the device-memory calls (put, run(r, u, keep, T))"""
    from acme_jl_amd.runner import MeasurementWeighting
    m = X.wire_model(1, k * FS)
    src = dict(kind="sine", f_den=441, f_num=1 + np.arange(N) % 40, amp=np.logspace(-2, 0.7, N), phase=np.arange(N) % 441)
    length = T - 100 if length is None else length
    groups, G = np.arange(N) % 3, 4                         # (group 3 is empty)
    groups[[5 % N, 64 % N]] = -1
    E = slots(length, stride)

    def fresh(sourced=False, pi=False):
        r = mk(m, N).set_oversampling(k)
        if sourced:
            r = sr.apply_sources(r, [src])
        if pi:      # (the per-instance form: its table's budget sets the chunk length)
            r.set_measurement(start=S, length=length, f_den=441, f_num=1 + np.arange(N), harmonics=2)
        else:
            r.set_measurement(start=S, length=length)
        if weighted:
            r.set_measurement_weighting(SOS)
        return r.set_measurement_ensemble(groups, G, stride)

    u = sr.apply_sources(mk(m, N).set_oversampling(k), [src]).render_sources(T)
    r = fresh()
    y = r.run(u, time_major=True)
    ref = got(r)
    assert np.isfinite(y).all()
    seen = MeasurementWeighting(SOS).apply(y.transpose(0, 2, 1)).transpose(0, 2, 1) if weighted else y
    assert_ensemble(ref, window(seen, S, length), groups, G, stride, E)
    results = {"y NULL": got(fresh().measure(u, time_major=True))}
    # split calls: before the start, off and on a recorded sample, on a tile and on a chunk boundary, beyond the window's end
    for cut in sorted({c for c in (S - 1, S + 1, S + stride, S + 64, S + 150, S + 4096, S + length + 10) if 0 < c < T}):
        r = fresh()
        assert np.array_equal(r.run(np.ascontiguousarray(u[:, :cut]), time_major=True), y[:, :cut])
        r.measure(np.ascontiguousarray(u[:, cut:]), time_major=True)
        results[f"split at {cut}"] = got(r)
    t1 = min(S + 137, T - 1)
    ud = dev.put(u)
    r = fresh()
    assert np.array_equal(dev.run(r, ud, True, T), y)
    results["device"] = got(r)
    r = fresh()
    dev.run(r, ud, False, T)
    results["device, y NULL"] = got(r)
    r = fresh()
    dev.run(r, dev.put(u[:, :t1]), False, t1)
    dev.run(r, dev.put(u[:, t1:]), False, T - t1)
    results["device, y NULL, split"] = got(r)
    r = fresh()
    ya = np.zeros_like(y)
    r.run_async(u, ya)
    r.wait()
    assert np.array_equal(ya, y)
    results["async"] = got(r)
    r = fresh()
    r.run_async(u, None)
    r.wait()
    results["async, y NULL"] = got(r)
    r = fresh(sourced=True)
    assert np.array_equal(r.run_sources(T), y)
    results["sources"] = got(r)
    results["sources, y NULL"] = got(fresh(sourced=True).measure(T=T))
    monkeypatch.setenv("ACME_OS_SLICE", "150")
    results["slices of 150"] = got(fresh().measure(u, time_major=True))
    r = fresh()
    assert np.array_equal(r.run(u, time_major=True), y)
    results["slices of 150, y stored"] = got(r)
    # ... with chunks of one tile (the per-instance form under a table budget of one byte), the calls cut again
    monkeypatch.setenv("ACME_MEAS_TABLE_BUDGET", "1")
    b = fresh(pi=True)
    assert b.measurement_plan()["chunk"] == 64
    b.measure(np.ascontiguousarray(u[:, :t1]), time_major=True)
    b.measure(np.ascontiguousarray(u[:, t1:]), time_major=True)
    results["slices of 150, chunks of one tile, split"] = got(b)
    monkeypatch.delenv("ACME_MEAS_TABLE_BUDGET")
    monkeypatch.delenv("ACME_OS_SLICE")
    # both shapes of the kernel, whatever the launch would choose
    for split in "01":
        monkeypatch.setenv("ACME_ENS_SPLIT", split)
        results[f"ACME_ENS_SPLIT={split}"] = got(fresh().measure(u, time_major=True))
    monkeypatch.delenv("ACME_ENS_SPLIT")
    for name, g in results.items():
        assert same(g, ref), name
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
        assert same(got(q), got(r))


# ---- 6. coexistence ------------------------------------------------------------------------------------------------------------
def check_coexistence(mk, N, T, start=5):
    m, u = wire_data(N, T)
    tgt = np.random.default_rng(9).standard_normal((2, 1, 77)) * 3.0
    which, lag = np.arange(N) % 2, np.arange(N) % 77
    groups = np.arange(N) % 4
    arm = lambda: mk(m, N).set_measurement(start=start, length=T - 50, f0=(10, 441), harmonics=3)
    adds = {"fold": lambda r: r.set_measurement_fold(50), "spectrum": lambda r: r.set_measurement_spectrum(64, 32),
            "cross": lambda r: r.set_measurement_cross(0, 64, 32),
            "target": lambda r: r.set_measurement_target(tgt, which=which, lag=lag, preemphasis=0.95),
            "ensemble": lambda r: r.set_measurement_ensemble(groups, stride=3)}
    reads = {"fold": lambda r: r.measurement_fold(raw=True).mean, "spectrum": lambda r: r.measurement_spectrum(raw=True).power,
             "cross": lambda r: np.stack([r.measurement_cross(raw=True).sxx, r.measurement_cross(raw=True).syy,
                                          r.measurement_cross(raw=True).sxy.real, r.measurement_cross(raw=True).sxy.imag]),
             "target": lambda r: r.measurement_target(raw=True).sums}
    base = arm()
    base.measure(u, time_major=True)
    every = arm()
    for add in adds.values():
        add(every)
    every.measure(u, time_major=True)
    assert raw(every)[1] == raw(base)[1] and np.array_equal(raw(every)[0], raw(base)[0])
    for name, add in adds.items():
        alone = add(arm())
        alone.measure(u, time_major=True)
        if name == "ensemble":
            assert same(got(alone), got(every)) and got(alone)["filled"] == slots(T - 50, 3)
        else:
            assert np.array_equal(reads[name](alone), reads[name](every), equal_nan=True), name
        assert np.array_equal(raw(alone)[0], raw(base)[0]), name


# ---- 7. a real circuit ----------------------------------------------------------------------------------------------------------
def check_use_level(mk, N=16, T=2100):
    """the diode clipper at N drive levels, a 1 kHz sine source, groups of four neighbouring levels"""
    m = clipper()
    src = dict(kind="sine", f_den=441, f_num=np.full(N, 10), amp=np.logspace(-1, 0.7, N))
    y = sr.apply_sources(mk(m, N), [src]).run_sources(T)
    groups = np.arange(N) // 4
    r = sr.apply_sources(mk(m, N), [src]).set_measurement(length=T).set_measurement_ensemble(groups)
    r.measure(T=T)
    e = r.measurement_ensemble()
    assert_ensemble(got(r), y, groups, N // 4, 1, T)
    assert e.filled == T and e.members.tolist() == [4] * (N // 4)
    mean, (lo, hi) = e.mean(), e.band()
    assert (lo <= mean).all() and (mean <= hi).all()        # (four members: the division is exact, the sums monotonic)
    yg = y[:, :, 0].reshape(N // 4, 4, T)
    assert (lo[:, 0, None, :] <= yg).all() and (yg <= hi[:, 0, None, :]).all()      # the band holds every member's waveform
    # the positive half-wave from the input's crest to its zero crossing (the source's phase: 10 / 441 of a turn per sample):
    # every member sits on its static curve there, a higher drive level a higher output.  (On the rising flank before the
    # crest the stored y of the hardest driven levels cross: the capacitor's charge lags the harder clipped waveform.)
    phase = (10 * np.arange(T) % 441) / 441.0
    rising = (phase > 0.25) & (phase < 0.5)
    assert rising.sum() > 100 and (e.argmax[:, 0][:, rising] == (4 * np.arange(N // 4) + 3)[:, None]).all()
    # std from Q - S^2 / n: the difference carries up to ~4 u Q / n of rounding, so std is off by at most sqrt(4 u Q / n)
    # where the variance vanishes (|y| < 1 V here: 2.1e-8)
    assert np.abs(y).max() < 1.0 and (e.std()[:, 0][:, rising] > 0).all()
    assert np.allclose(e.std()[:, 0], yg.std(axis=1), rtol=0, atol=np.sqrt(4 * X.U))
    return e


# ---- 8. life cycle and refusals ------------------------------------------------------------------------------------------------
def check_life_cycle(mk, N=7, T=300, start=9, length=250):
    from acme_jl_amd.runner import AcmeError
    m, u = wire_data(N, T)
    groups = np.arange(N) % 2
    r = mk(m, N).set_measurement(start=start, length=length).set_measurement_ensemble(groups, stride=3)
    y = r.run(u, time_major=True)                           # (the pass-through model has no state: a rerun repeats y)
    E = slots(length, 3)
    first = got(r)
    assert_ensemble(first, window(y, start, length), groups, 2, 3, E)
    # a reset returns every slot to the start values and keeps group, G and stride
    r.reset_measurement()
    zero = got(r)
    assert zero["filled"] == 0 and same(zero, replay(np.zeros((N, 0, 1)), groups, 2, 3, E))
    r.measure(u, time_major=True)
    assert same(got(r), first)
    # an ensemble set again replaces the earlier one (after a reset: nothing has been fed)
    r.reset_measurement().set_measurement_ensemble(None, 2, 64)
    r.measure(u, time_major=True)
    assert_ensemble(got(r), window(y, start, length), None, 2, 64, slots(length, 64))
    # re-arming and clear remove it
    L = r.lib.L
    r.set_measurement(start=start, length=length)
    with pytest.raises(AcmeError, match="no measurement ensemble"):
        r.measurement_ensemble()
    assert L.acme_batch_get_measurement_ensemble(r.h, None, None, None, None) == -1 and "no measurement ensemble" in L.acme_last_error().decode()
    r.set_measurement_ensemble().clear_measurement()
    assert L.acme_batch_get_measurement_ensemble(r.h, None, None, None, None) == -1 and "no measurement ensemble" in L.acme_last_error().decode()
    with pytest.raises(AcmeError, match="no measurement is armed"):
        r.set_measurement_ensemble()


def check_set_matrices_carries_the_ensemble(mk):
    from helpers import sweep_inputs
    from test_emu_parity import superover_models_with_their_own_diodes
    models = superover_models_with_their_own_diodes(3, HS)
    u = np.ascontiguousarray(sweep_inputs("superover_var", 3, 60, seed=2).transpose(0, 2, 1))
    r = mk(models[0], 3, models=[models[0]] * 3).set_measurement(start=10, length=45)
    groups = [0, 1, 0]
    r.set_measurement_ensemble(groups, stride=2)
    ya = r.run(np.ascontiguousarray(u[:, :25]), time_major=True)
    r.set_models(1, [models[0]])
    r.set_models(2, [models[2]])                            # (the batch moves to the plain shape: a new batch takes the measurement over)
    yb = r.run(np.ascontiguousarray(u[:, 25:]), time_major=True)
    assert_ensemble(got(r), window(np.concatenate([ya, yb], axis=1), 10, 45), groups, 2, 2, slots(45, 2))


def check_errors(mk):
    """every refusal with its code and the argument's name in the message"""
    from acme_jl_amd.runner import AcmeError, DimensionMismatch, _ip
    m, u = wire_data(3, 10)

    def refused(r, code, what, groups, G, stride):
        ga = None if groups is None else np.asarray(groups, dtype=np.int32)
        rc = r.lib.L.acme_batch_set_measurement_ensemble(r.h, None if ga is None else _ip(ga), G, stride)
        msg = r.lib.L.acme_last_error().decode()
        assert rc == code and all(w in msg for w in what), (groups, G, stride, rc, msg)
    r = mk(m, 3)
    refused(r, -1, ["no measurement is armed"], None, 1, 1)
    r.set_measurement(start=1)
    refused(r, -1, ["bounded", "length"], None, 1, 1)        # an unbounded window
    r.set_measurement(start=1, length=8)
    for stride in (0, -3):
        refused(r, -1, ["stride"], None, 1, stride)
    for G in (0, -1):
        refused(r, -1, ["G"], None, G, 1)
    refused(r, -1, ["group", "instance 1"], [0, 2, 1], 2, 1)
    refused(r, -1, ["group", "instance 2"], [0, 1, -2], 2, 1)
    assert r.lib.L.acme_batch_get_measurement_ensemble(r.h, None, None, None, None) == -1     # (a refused ensemble leaves none behind)
    r.measure(u, time_major=True)
    refused(r, -1, ["samples have been fed"], None, 1, 1)
    r.reset_measurement()
    # a series and an ensemble exclude each other, whichever is set first
    r.set_measurement_ensemble([0, -1, 1])
    assert r.lib.L.acme_batch_set_measurement_series(r.h, 4, 4, 2) == -2 and "ensemble" in r.lib.L.acme_last_error().decode()
    with pytest.raises(AcmeError, match="ensemble"):
        r.set_measurement_series(4, 4, 2)
    r.set_measurement(start=1).set_measurement_series(4, 4, 2)
    refused(r, -2, ["series"], None, 1, 1)
    # the cap: G nrows E = ACME_MAX_ENSEMBLE is accepted, one more slot is not -- by the arming call alone, cleared at once
    r.set_measurement(start=1, length=CAP + 1)
    refused(r, -1, ["G nrows E", str(CAP)], None, 1, 1)
    r.set_measurement(start=1, length=CAP // 4096 + 1)
    refused(r, -1, ["G nrows E", str(CAP)], None, 4096, 1)
    r.set_measurement(start=1, length=CAP // 4096)
    r.set_measurement_ensemble(None, 4096, 1)
    filled = C.c_longlong(-1)
    assert r.lib.L.acme_batch_get_measurement_ensemble(r.h, None, None, None, C.byref(filled)) == 0 and filled.value == 0
    r.clear_measurement()
    # the Python layer's own refusals
    r.set_measurement(start=1, length=8)
    with pytest.raises(DimensionMismatch):
        r.set_measurement_ensemble([0, 0])
    with pytest.raises(DimensionMismatch):
        r.set_measurement_ensemble([0.5, 0, 0])


# ---- 9. a non-finite instance ---------------------------------------------------------------------------------------------------
def check_nan_instance(mk, N=4, T=50, bad=20):
    """the recipe of test_measurement: a NaN in one instance's input.  Its group's four chains read NaN from that sample on,
    both indices name the instance; the other group is unaffected"""
    m, u = clipper(), clipper_u(N, T)
    u[1, bad, 0] = np.nan
    groups = [0, 0, 1, 1]
    r = mk(m, N).set_measurement(length=T).set_measurement_ensemble(groups)
    y = r.run(u, time_major=True, check=False)
    assert r.report_arrays()["first_nonfinite"].tolist()[1] >= 0
    assert np.isnan(y[1, bad:]).all() and np.isfinite(y[[0, 2, 3]]).all() and np.isfinite(y[1, :bad]).all()
    e = r.measurement_ensemble()
    assert_ensemble(got(r), y, groups, 2, 1, T)
    for a in (e.sum, e.sumsq, e.min, e.max):
        assert np.isnan(a[0, 0, bad:]).all() and np.isfinite(a[0, 0, :bad]).all() and np.isfinite(a[1]).all()
    assert (e.argmin[0, 0, bad:] == 1).all() and (e.argmax[0, 0, bad:] == 1).all()
    assert np.isin(e.argmin[1], [2, 3]).all() and np.isin(e.argmax[1], [2, 3]).all()


def check_two_nan_members(mk, N=6, T=50, first=20, second=30):
    """two members of one group go non-finite at different samples.  The rule `v < mn || v != v` lets every NaN member take
    the index over, so from the sample at which both are NaN on the indices name the LAST of them in instance order (the
    header's contract), with a finite member between the two changing nothing; while only one is NaN they name that one"""
    m, u = clipper(), clipper_u(N, T)
    u[1, first, 0] = np.nan
    u[3, second, 0] = np.nan
    groups = [0, 0, 0, 0, 1, 1]
    r = mk(m, N).set_measurement(length=T).set_measurement_ensemble(groups)
    y = r.run(u, time_major=True, check=False)
    assert np.isnan(y[1, first:]).all() and np.isnan(y[3, second:]).all() and np.isfinite(y[3, :second]).all()
    assert np.isfinite(y[[0, 2, 4, 5]]).all()
    e = r.measurement_ensemble()
    assert_ensemble(got(r), y, groups, 2, 1, T)
    for a in (e.sum, e.sumsq, e.min, e.max):
        assert np.isnan(a[0, 0, first:]).all() and np.isfinite(a[0, 0, :first]).all() and np.isfinite(a[1]).all()
    for a in (e.argmin, e.argmax):
        assert (a[0, 0, first:second] == 1).all() and (a[0, 0, second:] == 3).all()
        assert np.isin(a[1], [4, 5]).all()

