"""Shared by the emulator and GPU tests of the measurement events (acme_batch_set_measurement_events): the reference every
result is held to -- the contract's rule as a sequential loop over the window's samples of the stored y of an identical run
without events (one step per sample, in time order; numpy only carries the step across the independent triples) -- and the
checks, each taking ``mk(model, n)``, which makes a fresh runner on the library under test (the emulator's or the GPU's).
Every comparison is ``==``: the integer arrays as they are, the copied values ``ab`` through ``view(int64)``.  Every read also
asserts HIGH + LOW + UNKNOWN == count for every triple and that slot E holds the last recorded event."""
import ctypes as C
import functools

import numpy as np
import pytest

import exact_ref as X
import source_ref as sr
from helpers import FS, HS
from test_measurement import clipper, raw, two_output_clipper

CAP = 16777216              # ACME_MAX_EVENTS
MAX_LEVELS, MAX_SLOTS = 8, 16
UNKNOWN, LOW, HIGH = 0, 1, 2
RISE, FALL = 0, 1
START, LENGTH = 3, 4096 + 777               # the geometry's window: a chunk boundary inside, a length that is no multiple of 64
T_GEO = START + LENGTH + 24
SIGNALS = ["constant", "alternating", "sine 64 then 63", "noise", "missed levels"]
LEVELS, SLOTS = [1, 3, 8], [0, 1, 16]


# ---- the reference ------------------------------------------------------------------------------------------------------------
def rule_loop(vs, lo, hi, E):
    """the contract for ONE triple in Python floats, sample after sample: (counters [5], idx [2][E + 1], ab [2][E + 1][2])"""
    state, cnt = UNKNOWN, [0] * 5
    idx = [[-1] * (E + 1) for _ in range(2)]
    ab = [[[0.0, 0.0] for _ in range(E + 1)] for _ in range(2)]
    for m, v in enumerate(vs):
        nxt = HIGH if v >= hi else LOW if v <= lo else state
        for d, (a, b) in enumerate(((LOW, HIGH), (HIGH, LOW))):
            if state == a and nxt == b:
                if cnt[d] < E:
                    idx[d][cnt[d]], ab[d][cnt[d]] = m, [vs[m - 1], v]
                idx[d][E], ab[d][E] = m, [vs[m - 1], v]
                cnt[d] += 1
        cnt[{HIGH: 2, LOW: 3, UNKNOWN: 4}[nxt]] += 1
        state = nxt
    return cnt, idx, ab


def replay(yw, lo, hi, E, at=()):
    """the contract on the window's samples so far yw [N, count, nrows] with the levels lo, hi [C, N]: (counters
    [N, nrows, C, 5], idx [N, nrows, C, 2, E + 1], ab [N, nrows, C, 2, E + 1, 2]); ``at``: also {count: that triple} after
    the first ``count`` samples, for each count named"""
    N, count, nrows = yw.shape
    lo_, hi_ = (np.ascontiguousarray(np.asarray(a, dtype=np.float64).T)[:, None, :] for a in (lo, hi))     # [N, 1, C]
    nC = lo_.shape[-1]
    state = np.zeros((N, nrows, nC), dtype=np.int8)
    cnt = np.zeros((N, nrows, nC, 5), dtype=np.int64)
    idx = np.full((N, nrows, nC, 2, E + 1), -1, dtype=np.int64)
    ab = np.zeros((N, nrows, nC, 2, E + 1, 2))
    snaps = {0: (cnt.copy(), idx.copy(), ab.copy())} if 0 in at else {}
    for m in range(count):
        v = yw[:, m, :, None]
        nxt = np.where(v >= hi_, HIGH, np.where(v <= lo_, LOW, state)).astype(np.int8)
        for d, (a, b) in enumerate(((LOW, HIGH), (HIGH, LOW))):
            ev = (state == a) & (nxt == b)
            if ev.any():
                assert m > 0
                w = np.nonzero(ev)
                va, vb, k = yw[w[0], m - 1, w[1]], yw[w[0], m, w[1]], cnt[..., d][w]
                f = k < E
                wf = tuple(x[f] for x in w)
                idx[wf + (d, k[f])] = m
                ab[wf + (d, k[f], 0)], ab[wf + (d, k[f], 1)] = va[f], vb[f]
                idx[w + (d, E)] = m
                ab[w + (d, E, 0)], ab[w + (d, E, 1)] = va, vb
                cnt[..., d] += ev
        cnt[..., 2] += nxt == HIGH
        cnt[..., 3] += nxt == LOW
        cnt[..., 4] += nxt == UNKNOWN
        state = nxt
        if m + 1 in at:
            snaps[m + 1] = (cnt.copy(), idx.copy(), ab.copy())
    return (cnt, idx, ab, snaps) if at else (cnt, idx, ab)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def got(r):
    """the getter's arrays through ``measurement_events()``: (counters, idx, ab, count); asserts the sum of every triple's
    state counters, the empty slots and that slot E is the last recorded event"""
    e = r.measurement_events()
    cnt, idx, ab = e.counts, e.idx, e.ab
    E = idx.shape[-1] - 1
    assert cnt.dtype == np.int64 and idx.dtype == np.int64 and ab.dtype == np.float64 and (cnt >= 0).all()
    assert (cnt[..., 2] + cnt[..., 3] + cnt[..., 4] == e.count).all(), (cnt[..., 2:].sum(axis=-1), e.count)
    n = cnt[..., :2]                                        # [N, nrows, C, 2]: the events of each direction
    filled = np.arange(E)[None, None, None, None, :] < n[..., None]
    assert (idx[..., :E][~filled] == -1).all() and (bits(ab[..., :E, :])[~filled] == 0).all()
    assert (idx[..., :E][filled] >= 1).all() and (idx[..., :E][filled] < max(e.count, 1)).all()
    if E > 1:
        both = filled[..., 1:]
        assert (np.diff(idx[..., :E], axis=-1)[both] > 0).all()                 # the first E in time order
    none = n == 0
    assert (idx[..., E][none] == -1).all() and (bits(ab[..., E, :])[none] == 0).all()
    assert (idx[..., E][~none] >= 1).all()
    if E:
        within = (n >= 1) & (n <= E)                        # slot E equals slot n - 1
        k = np.clip(n - 1, 0, E - 1)[..., None]
        assert (np.take_along_axis(idx[..., :E], k, axis=-1)[..., 0][within] == idx[..., E][within]).all()
        same = np.take_along_axis(bits(ab[..., :E, :]), k[..., None], axis=-2)[..., 0, :] == bits(ab[..., E, :])
        assert same[within].all()
        assert (idx[..., E][n > E] > idx[..., E - 1][n > E]).all()             # ... and lies beyond the first E after them
    return cnt, idx, ab, e.count


def assert_equal(have, want, what=""):
    for name, a, b in zip(("counters", "idx", "ab"), have, want):
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        if a.dtype == np.float64:
            a, b = bits(a), bits(b)
        assert np.array_equal(a, b), (what, name, np.argwhere(a != b)[:6])


def assert_events(r, yw, lo, hi, E, what="", want=None):
    cnt, idx, ab, count = got(r)
    assert count == yw.shape[1], (what, count, yw.shape)
    want = replay(yw, lo, hi, E) if want is None else want
    assert_equal((cnt, idx, ab), want, what)
    return cnt, idx, ab


def window(y, start, length, rows=None):
    """the measured samples of the stored y [N, T, ny]: [N, count, nrows]"""
    stop = y.shape[1] if not length else min(y.shape[1], start + length)
    return y[:, start:stop][:, :, list(range(y.shape[2])) if rows is None else rows]


def levels2(lo, hi, N):
    """[C] or [C, N] -> [C, N] arrays"""
    f = lambda a: np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64).reshape(len(a), -1), (len(a), N)))
    return f(lo), f(hi)


# ---- 1. hand-listed pins ------------------------------------------------------------------------------------------------------
TINY = 5e-324               # the smallest subnormal
INF, NAN = np.inf, np.nan
# (signal, lo, hi, E) -> (counters RISE FALL HIGH LOW UNKNOWN, rises [(m, a, b)], falls [(m, a, b)]): every event written out by
# hand from the rule; the lists hold ALL events, the first E of them are the slots and the last one is slot E
PINS = [
    # a Schmitt band [-1, 1]: unknown inside the band, a value exactly equal to hi (m = 3) and to lo (m = 6), a wiggle inside
    # the band (m = 4, 5 and 7, 8) that keeps the state
    ([0.0, 0.5, -2.0, 1.0, 0.9, -0.9, -1.0, 0.0, 0.99, 1.5, -1.5], -1.0, 1.0, 2,
     ([2, 2, 4, 5, 2], [(3, -2.0, 1.0), (9, 0.99, 1.5)], [(6, -0.9, -1.0), (10, 1.5, -1.5)])),
    # a comparator lo == hi == 0.5 and v == level: >= wins, the sample is HIGH
    ([0.0, 0.5, 0.5, 0.25, 0.5, 0.75, 0.0], 0.5, 0.5, 4,
     ([2, 2, 4, 3, 0], [(1, 0.0, 0.5), (4, 0.25, 0.5)], [(3, 0.5, 0.25), (6, 0.75, 0.0)])),
    # a signal that never leaves the band: UNKNOWN == count, no slot filled
    ([0.1, -0.1, 0.2, -0.2, 0.0, 0.3], -0.5, 0.5, 3, ([0, 0, 0, 0, 6], [], [])),
    # level 0.0, both zeros are HIGH (-0.0 >= 0.0): the pass-through model hands -0.0 on as +0.0 anyway, and the slots hold
    # what the model handed on; the smallest subnormal on either side of the level
    ([-1.0, 0.0, -TINY, -0.0, -1.0, TINY, -TINY, 0.0], 0.0, 0.0, 8,
     ([4, 3, 4, 4, 0], [(1, -1.0, 0.0), (3, -TINY, 0.0), (5, -1.0, TINY), (7, -TINY, 0.0)],
      [(2, 0.0, -TINY), (4, 0.0, -1.0), (6, TINY, -TINY)])),
    # more events than slots: E = 1 keeps the first and the last
    ([-1.0, 1.0, -1.0, 1.0, -1.0, 1.0], 0.0, 0.0, 1,
     ([3, 2, 3, 3, 0], [(1, -1.0, 1.0), (3, -1.0, 1.0), (5, -1.0, 1.0)], [(2, 1.0, -1.0), (4, 1.0, -1.0)])),
    # E = 0: counters and the last event alone
    ([-1.0, 1.0, -1.0, 1.0], 0.0, 0.0, 0, ([2, 1, 2, 2, 0], [(1, -1.0, 1.0), (3, -1.0, 1.0)], [(2, 1.0, -1.0)])),
    # an infinity: a rise onto +inf.  The pass-through model is NaN from the sample AFTER its first non-finite one on (the
    # histogram's tests pin that), so the state freezes HIGH and HIGH keeps counting
    ([-1.0, -2.0, INF, -1.0, -1.0, 1.0], 0.0, 0.0, 2, ([1, 0, 4, 2, 0], [(2, -2.0, INF)], [])),
    ([1.0, 2.0, -INF, 1.0, 1.0], 0.0, 0.0, 2, ([0, 1, 2, 3, 0], [], [(2, 2.0, -INF)])),
    # an instance that turns NaN at m = 3 while LOW: no event any more, LOW keeps counting (what the input does from there on
    # is lost: the pass-through model stays NaN)
    ([1.0, -1.0, -1.0, NAN, 1.0, -1.0, 1.0], 0.0, 0.0, 2, ([0, 1, 1, 6, 0], [], [(1, 1.0, -1.0)])),
    # NaN from the first sample on: the state never leaves UNKNOWN
    ([NAN, 1.0, -1.0, 1.0], 0.0, 0.0, 2, ([0, 0, 0, 0, 4], [], [])),
]


def expected_from_pin(pin, E):
    cnt, rises, falls = pin
    idx = np.full((2, E + 1), -1, dtype=np.int64)
    ab = np.zeros((2, E + 1, 2))
    for d, evs in enumerate((rises, falls)):
        assert cnt[d] == len(evs)
        for k, (m, a, b) in enumerate(evs[:E]):
            idx[d, k], ab[d, k] = m, (a, b)
        if evs:
            idx[d, E], ab[d, E] = evs[-1][0], evs[-1][1:]
    return np.array(cnt, dtype=np.int64), idx, ab


def model_output(vs):
    """what the pass-through model hands on for the input vs: y = 0.0 + u reads -0.0 as +0.0, and an instance is NaN from the
    sample after its first non-finite one on"""
    out, dead = [], False
    for v in vs:
        out.append(NAN if dead else v + 0.0)
        dead = dead or not np.isfinite(v)
    return out


def check_pins(mk):
    for vs, lo, hi, E, pin in PINS:
        T = len(vs)
        u = np.zeros((3, T, 1))
        u[0, :, 0] = u[2, :, 0] = vs                        # (instance 1 is all zeros: a neighbour the others do not touch)
        r = mk(X.wire_model(1, FS), 3).set_measurement().set_measurement_events(lo=[lo], hi=[hi], slots=E)
        y = r.run(u, time_major=True, check=False)
        seen, out = np.array(model_output(vs)), y[0, :, 0]
        ok = ~np.isnan(seen)                                # (which NaN the model hands on is the model's business)
        assert np.array_equal(np.isnan(out), ~ok) and np.array_equal(bits(out[ok]), bits(seen[ok])), (vs, out)
        want = expected_from_pin(pin, E)
        # the hand-listed events are what the rule gives on the model's output, and what the replay gives
        by_rule = rule_loop(out.tolist(), lo, hi, E)
        assert by_rule[0] == want[0].tolist() and by_rule[1] == want[1].tolist()
        assert np.array_equal(bits(np.array(by_rule[2])), bits(want[2])), (vs, by_rule[2], want[2])
        cnt, idx, ab = assert_events(r, y, *levels2([lo], [hi], 3), E, (vs, lo, hi, E))
        for i in (0, 2):
            assert_equal((cnt[i, 0, 0], idx[i, 0, 0], ab[i, 0, 0]), want, (vs, lo, hi, E, i))
        zero = rule_loop([0.0] * T, lo, hi, E)
        assert cnt[1, 0, 0].tolist() == zero[0] and (idx[1] == -1).all()
    # the sub-sample times the host forms from the first pin: thr = hi for a rise, lo for a fall
    vs, lo, hi, E, _ = PINS[0]
    r = mk(X.wire_model(1, FS), 1).set_measurement().set_measurement_events(lo=[lo], hi=[hi], slots=E)
    r.measure(np.array(vs)[None, :, None], time_major=True)
    e = r.measurement_events()
    t, last = e.times("rise", 0)
    assert t[0, 0].tolist() == [2.0 + (1.0 - -2.0) / (1.0 - -2.0), 8.0 + (1.0 - 0.99) / (1.5 - 0.99)] and last[0, 0] == t[0, 0, 1]
    t, last = e.times("fall", 0)
    assert t[0, 0].tolist() == [5.0 + (-1.0 - -0.9) / (-1.0 - -0.9), 9.0 + (-1.0 - 1.5) / (-1.5 - 1.5)] and last[0, 0] == t[0, 0, 1]
    assert e.last_time(0)[0, 0] == t[0, 0, 1] and e.duty(0)[0, 0] == 4.0 / 9.0


# ---- 2. geometry, 3. rows -----------------------------------------------------------------------------------------------------
def signal(mk, name, N, T):
    """u [N, T, 1] and the amplitude of each instance"""
    t = np.arange(T)
    amp = np.linspace(0.05, 1.3, N)[:, None]
    if name == "constant":
        u = np.broadcast_to(amp * np.where(np.arange(N) % 2 == 0, 1.0, -1.0)[:, None], (N, T))
    elif name == "alternating":             # an event on every sample at the level 0: on every lane, first and last
        u = np.where(t[None] % 2 == 0, amp, -0.37 * amp)
    elif name in ("sine 64 then 63", "missed levels"):      # crossings pinned to one lane, then drifting through all of them
        half = T // 2
        ph = np.where(t < half, t / 64.0, half / 64.0 + (t - half) / 63.0)
        u = amp * np.sin(2 * np.pi * ph + 0.3)[None]
    elif name == "noise":
        r = mk(X.wire_model(1, FS), N)
        r.set_source(0, "noise", amp=amp[:, 0], dist="uniform", hold=1, seed=11)
        u = r.render_sources(T)[:, :, 0]
    else:
        raise KeyError(name)
    return np.ascontiguousarray(np.asarray(u, dtype=np.float64)[:, :, None]), amp[:, 0]


def levels_for(name, amp, nC):
    """lo, hi [C, N]: fractions of each instance's amplitude, level 0 among them; a hysteresis band for the noise; for "missed
    levels" bands the signal never reaches (i mod 3: above it, below it, around it)"""
    N = len(amp)
    frac = np.array([0.0]) if nC == 1 else np.linspace(-0.8, 0.8, nC)
    if nC > 1:
        frac[nC // 2] = 0.0
    mid = frac[:, None] * amp[None, :]
    half = 0.1 * amp[None, :] if name == "noise" else 0.0
    lo, hi = mid - half, mid + half
    if name == "missed levels":
        k = (np.arange(N) % 3)[None, :]
        lo = np.where(k == 0, 10.0 + mid, np.where(k == 1, -11.0 + mid, -10.0 + mid))
        hi = np.where(k == 0, 11.0 + mid, np.where(k == 1, -10.0 + mid, 10.0 + mid))
    return np.ascontiguousarray(lo), np.ascontiguousarray(hi)


@functools.lru_cache(maxsize=None)
def _plain_run(mk, name, two, N, T, start, length, rows):
    """the run without events every case of a shape shares: (model, u, amp, y, raw measurement); never modified"""
    m = two_output_clipper() if two else X.wire_model(1, FS)
    u, amp = signal(mk, name, N, T)
    r = mk(m, N).set_measurement(start=start, length=length, rows=None if rows is None else list(rows))
    y = r.run(u, time_major=True)
    return m, u, amp, y, raw(r)


@functools.lru_cache(maxsize=None)
def _replayed(mk, name, two, N, T, start, length, rows, nC, E, at):
    """the replay of a shape, with its snapshots, computed once; never modified"""
    m, u, amp, y, plain = _plain_run(mk, name, two, N, T, start, length, rows)
    lo, hi = levels_for(name, amp, nC)
    return replay(window(y, start, length, None if rows is None else list(rows)), lo, hi, E, at=at)


def check_geometry(mk, N, nC, E, name, T=T_GEO, start=START, length=LENGTH, rows=None, two=False, cuts=(2000, 4100)):
    """one call over the whole run, then three split calls with the results after each"""
    key = None if rows is None else tuple(rows)
    m, u, amp, y, plain = _plain_run(mk, name, two, N, T, start, length, key)
    lo, hi = levels_for(name, amp, nC)
    edges = [0, *cuts, T]
    counts = tuple(sorted({max(0, min(b, start + length) - start) for b in edges[1:]}))
    *want, snaps = _replayed(mk, name, two, N, T, start, length, key, nC, E, counts)
    arm = lambda: mk(m, N).set_measurement(start=start, length=length, rows=rows).set_measurement_events(lo=lo, hi=hi, slots=E)
    r = arm()
    r.measure(u, time_major=True)
    with_events = raw(r)
    assert with_events[1] == plain[1] and np.array_equal(with_events[0], plain[0])      # the measurement's own results
    yw = window(y, start, length, rows)
    cnt, idx, ab = assert_events(r, yw, lo, hi, E, "one call", want)
    if not two:
        if name == "constant":
            assert not cnt[..., :2].any() and not cnt[..., 4].any()
        if name == "alternating":                           # level 0 (and every level inside the swing): an event per sample
            c0 = nC // 2
            assert (cnt[:, 0, c0, RISE] + cnt[:, 0, c0, FALL] == length - 1).all()
            if E:
                d1, d2 = (FALL, RISE) if start % 2 == 0 else (RISE, FALL)   # (the signal is high at the even samples of the run)
                assert (idx[:, 0, c0, d1, 0] == 1).all() and (idx[:, 0, c0, d2, 0] == 2).all()
            assert (idx[:, 0, c0, :, E].max(axis=-1) == length - 1).all()
        if name == "missed levels":
            k = np.arange(N) % 3
            assert not cnt[..., :2].any()
            assert (cnt[k == 0][..., 3] == length).all() and (cnt[k == 1][..., 2] == length).all() and (cnt[k == 2][..., 4] == length).all()
        if name == "sine 64 then 63":
            c0 = nC // 2
            assert (cnt[:, 0, c0, RISE] >= length // 64 - 1).all()
    r = arm()
    for a, b in zip(edges[:-1], edges[1:]):
        r.measure(np.ascontiguousarray(u[:, a:b]), time_major=True)
        n = max(0, min(b, start + length) - start)
        assert_events(r, yw[:, :n], lo, hi, E, f"calls up to {b}", snaps[n])
    assert_equal(got(r)[:3], want, "split calls")


def check_slot_boundary(mk, E=4):
    """exactly E - 1, E and E + 1 events of a direction: pulses of five samples, instance i has E - 1 + i of them"""
    N, T = 3, 10 * (E + 2) + 7
    u = np.full((N, T, 1), -1.0)
    for i in range(N):
        for k in range(E - 1 + i):
            u[i, 5 + 10 * k:10 + 10 * k] = 1.0
    r = mk(X.wire_model(1, FS), N).set_measurement().set_measurement_events(0.0, slots=E)
    y = r.run(u, time_major=True)
    cnt, idx, ab = assert_events(r, y, *levels2([0.0], [0.0], N), E)
    for i in range(N):
        n = E - 1 + i
        assert cnt[i, 0, 0, :2].tolist() == [n, n]
        first = [5 + 10 * k for k in range(n)]
        assert idx[i, 0, 0, RISE].tolist() == (first + [-1] * E)[:E] + [first[-1] if n else -1]
        assert idx[i, 0, 0, FALL].tolist() == ([f + 5 for f in first] + [-1] * E)[:E] + [first[-1] + 5 if n else -1]
        assert (ab[i, 0, 0, RISE, :min(n, E)] == [-1.0, 1.0]).all() and (ab[i, 0, 0, FALL, E] == ([1.0, -1.0] if n else [0.0, 0.0])).all()


# ---- 4. paths -----------------------------------------------------------------------------------------------------------------
SOS = np.array([[0.5, 0.25, 0.125, -0.3, 0.1], [1.0, -1.0, 0.0, -0.995, 0.0]])


def check_paths(mk, dev, k, T, monkeypatch, nC=3, E=4, weighted=False, N=70, S=3, length=None):
    """the pass-through model driven by what a per-instance sine source renders, oversampled by k: the events read after
    every path == those after a host run with y stored == the replay (``weighted``: of ``MeasurementWeighting.apply`` on the
    stored y).  ``dev``: the device-memory calls (put, run(r, u, keep, T))"""
    from acme_jl_amd.runner import MeasurementWeighting
    m = X.wire_model(1, k * FS)
    amp = np.logspace(-2, 0.7, N)
    src = dict(kind="sine", f_den=441, f_num=1 + np.arange(N) % 40, amp=amp, phase=np.arange(N) % 441)
    length = T - 100 if length is None else length
    frac = np.linspace(-0.5, 0.5, nC) if nC > 1 else np.array([0.1])
    lo, hi = (frac[:, None] - 0.2) * amp[None, :], (frac[:, None] + 0.2) * amp[None, :]        # a Schmitt band per level

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
        return r.set_measurement_events(lo=lo, hi=hi, slots=E)

    u = sr.apply_sources(mk(m, N).set_oversampling(k), [src]).render_sources(T)
    r = fresh()
    y = r.run(u, time_major=True)
    assert np.isfinite(y).all()
    seen = MeasurementWeighting(SOS).apply(y.transpose(0, 2, 1)).transpose(0, 2, 1) if weighted else y
    yw = window(seen, S, length)
    ref = assert_events(r, yw, lo, hi, E)
    assert ref[0][..., :2].sum() > 0
    results = {"y NULL": got(fresh().measure(u, time_major=True))[:3]}
    # split calls: before the start, inside the first round, on a round and on a chunk boundary, beyond the window's end; one
    # sample before, on and after the first rise of the fastest instance that has one; with the last sample of the first call
    # strictly inside a hysteresis band
    cuts = {S - 1, S + 1, S + 64, S + 150, S + 4096, S + length + 10}
    i = int(np.argmax(ref[0][:, 0, 0, RISE] > 0))
    mev = int(ref[1][i, 0, 0, RISE, E])
    cuts |= {S + mev - 1, S + mev, S + mev + 1}
    inside = np.flatnonzero((yw[i, :, 0] > lo[0, i]) & (yw[i, :, 0] < hi[0, i]))
    assert inside.size
    cuts.add(S + int(inside[inside.size // 2]) + 1)
    for cut in sorted(c for c in cuts if 0 < c < T):
        r = fresh()
        assert np.array_equal(r.run(np.ascontiguousarray(u[:, :cut]), time_major=True), y[:, :cut])
        r.measure(np.ascontiguousarray(u[:, cut:]), time_major=True)
        results[f"split at {cut}"] = got(r)[:3]
    t1 = min(S + 137, T - 1)
    ud = dev.put(u)
    r = fresh()
    assert np.array_equal(dev.run(r, ud, True, T), y)
    results["device"] = got(r)[:3]
    r = fresh()
    dev.run(r, ud, False, T)
    results["device, y NULL"] = got(r)[:3]
    r = fresh()
    dev.run(r, dev.put(u[:, :t1]), False, t1)
    dev.run(r, dev.put(u[:, t1:]), False, T - t1)
    results["device, y NULL, split"] = got(r)[:3]
    r = fresh()
    ya = np.zeros_like(y)
    r.run_async(u, ya)
    r.wait()
    assert np.array_equal(ya, y)
    results["async"] = got(r)[:3]
    r = fresh()
    r.run_async(u, None)
    r.wait()
    results["async, y NULL"] = got(r)[:3]
    r = fresh(sourced=True)
    assert np.array_equal(r.run_sources(T), y)
    results["sources"] = got(r)[:3]
    results["sources, y NULL"] = got(fresh(sourced=True).measure(T=T))[:3]
    monkeypatch.setenv("ACME_OS_SLICE", "150")
    results["slices of 150"] = got(fresh().measure(u, time_major=True))[:3]
    r = fresh()
    assert np.array_equal(r.run(u, time_major=True), y)
    results["slices of 150, y stored"] = got(r)[:3]
    # ... with chunks of one round (the per-instance form under a table budget of one byte), the calls cut again
    monkeypatch.setenv("ACME_MEAS_TABLE_BUDGET", "1")
    b = fresh(pi=True)
    assert b.measurement_plan()["chunk"] == 64
    b.measure(np.ascontiguousarray(u[:, :t1]), time_major=True)
    b.measure(np.ascontiguousarray(u[:, t1:]), time_major=True)
    results["slices of 150, chunks of one round, split"] = got(b)[:3]
    monkeypatch.delenv("ACME_MEAS_TABLE_BUDGET")
    monkeypatch.delenv("ACME_OS_SLICE")
    for name, g in results.items():
        assert_equal(g, ref, name)
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
        assert_equal(got(q)[:3], got(r)[:3], "run_const")


# ---- 5. coexistence ------------------------------------------------------------------------------------------------------------
def check_coexistence(mk, N, T, start=5, nC=3, E=5):
    m = X.wire_model(1, FS)
    u = X.scaled_rows(np.random.default_rng(2000 + N), N, T, 1)
    tgt = np.random.default_rng(9).standard_normal((2, 1, 77)) * 3.0
    which, lag = np.arange(N) % 2, np.arange(N) % 77
    groups = np.arange(N) % 4
    scale = np.abs(u[:, :, 0]).max(axis=1)
    lo, hi = np.linspace(-0.5, 0.3, nC)[:, None] * scale[None, :], np.linspace(-0.3, 0.5, nC)[:, None] * scale[None, :]
    arm = lambda: mk(m, N).set_measurement(start=start, length=T - 50, f0=(10, 441), harmonics=3)
    adds = {"fold": lambda r: r.set_measurement_fold(50), "spectrum": lambda r: r.set_measurement_spectrum(64, 32),
            "cross": lambda r: r.set_measurement_cross(0, 64, 32),
            "target": lambda r: r.set_measurement_target(tgt, which=which, lag=lag, preemphasis=0.95),
            "ensemble": lambda r: r.set_measurement_ensemble(groups, stride=3),
            "histogram": lambda r: r.set_measurement_histogram(65, -2.0, 2.0)}
    ens = lambda r: [getattr(r.measurement_ensemble(), k) for k in ("sum", "sumsq", "min", "max", "argmin", "argmax")]
    hist = lambda r: [getattr(r.measurement_histogram(), k) for k in ("counts", "under", "over", "nan")]
    reads = {"fold": lambda r: [r.measurement_fold(raw=True).mean], "spectrum": lambda r: [r.measurement_spectrum(raw=True).power],
             "cross": lambda r: [r.measurement_cross(raw=True).sxx, r.measurement_cross(raw=True).syy,
                                 r.measurement_cross(raw=True).sxy.real, r.measurement_cross(raw=True).sxy.imag],
             "target": lambda r: [r.measurement_target(raw=True).sums], "ensemble": ens, "histogram": hist}
    without = arm()
    for add in adds.values():
        add(without)
    y = without.run(u, time_major=True)
    every = arm()
    for add in adds.values():
        add(every)
    every.set_measurement_events(lo=lo, hi=hi, slots=E)
    every.measure(u, time_major=True)
    assert raw(every)[1] == raw(without)[1] and np.array_equal(raw(every)[0], raw(without)[0])
    for name in adds:       # bit for bit what they are without the events
        for a, b in zip(reads[name](every), reads[name](without)):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64)), name
    want = assert_events(every, window(y, start, T - 50), lo, hi, E)
    alone = arm().set_measurement_events(lo=lo, hi=hi, slots=E)
    alone.measure(u, time_major=True)
    assert_equal(got(alone)[:3], want, "alone")


# ---- 6. life cycle and refusals ------------------------------------------------------------------------------------------------
def check_life_cycle(mk, N=7, T=300, start=9, length=250):
    from acme_jl_amd.runner import AcmeError
    m = X.wire_model(1, FS)
    u = np.random.default_rng(5).uniform(-1.2, 1.2, (N, T, 1))
    lo, hi = levels2([-0.5, 0.2], [-0.1, 0.2], N)
    lo = lo * np.linspace(0.5, 1.0, N)[None, :]
    r = mk(m, N).set_measurement(start=start, length=length).set_measurement_events(lo=lo, hi=hi, slots=3)
    y = r.run(u, time_major=True)                           # (the pass-through model has no state: a rerun repeats y)
    first = assert_events(r, window(y, start, length), lo, hi, 3)
    assert first[0][..., :2].min() > 3                      # (more events than slots everywhere)
    # a reset zeroes the counters, empties the slots, returns the states to UNKNOWN and keeps C, E and the levels
    r.reset_measurement()
    cnt, idx, ab, count = got(r)
    e = r.measurement_events()
    assert count == 0 and not cnt.any() and (idx == -1).all() and not bits(ab).any()
    assert np.array_equal(e.lo, lo) and np.array_equal(e.hi, hi) and e.slots == 3 and e.levels == 2
    r.measure(u, time_major=True)
    assert_equal(got(r)[:3], first, "after a reset")        # (a state or a value left over would show in the first events)
    # events set again replace the earlier ones (after a reset: nothing has been fed)
    r.reset_measurement().set_measurement_events(0.1, hysteresis=0.5, slots=0)
    r.measure(u, time_major=True)
    l1, h1 = levels2([0.1 - 0.25], [0.1 + 0.25], N)
    again = assert_events(r, window(y, start, length), l1, h1, 0)
    assert again[1].shape == (N, 1, 1, 2, 1)
    # re-arming and clear remove them
    L = r.lib.L
    r.set_measurement(start=start, length=length)
    with pytest.raises(AcmeError, match="no measurement events"):
        r.measurement_events()
    assert L.acme_batch_get_measurement_events(r.h, None, None, None, None) == -1 and "no measurement events" in L.acme_last_error().decode()
    r.set_measurement_events(0.0).clear_measurement()
    assert L.acme_batch_get_measurement_events(r.h, None, None, None, None) == -1 and "no measurement events" in L.acme_last_error().decode()
    with pytest.raises(AcmeError, match="no measurement is armed"):
        r.set_measurement_events(0.0)
    # an unbounded window, and a start beyond the run: nothing counted
    r = mk(m, N).set_measurement(start=start).set_measurement_events(0.0, slots=2)
    r.measure(u, time_major=True)
    assert_events(r, window(y, start, 0), *levels2([0.0], [0.0], N), 2)
    r = mk(m, N).set_measurement(start=T + 5).set_measurement_events(0.0, slots=2)
    r.measure(u, time_major=True)
    assert got(r)[3] == 0 and not got(r)[0].any()


def check_set_matrices_carries_the_events(mk):
    from helpers import sweep_inputs
    from test_emu_parity import superover_models_with_their_own_diodes
    models = superover_models_with_their_own_diodes(3, HS)
    u = np.ascontiguousarray(sweep_inputs("superover_var", 3, 60, seed=2).transpose(0, 2, 1))
    r = mk(models[0], 3, models=[models[0]] * 3).set_measurement(start=10, length=45)
    plain = mk(models[0], 3, models=[models[0]] * 3)
    ya = plain.run(np.ascontiguousarray(u[:, :25]), time_major=True)
    scale = np.abs(ya).max(axis=(1, 2))
    lo, hi = np.array([-0.2, 0.0])[:, None] * scale[None, :], np.array([0.2, 0.0])[:, None] * scale[None, :]
    r.set_measurement_events(lo=lo, hi=hi, slots=2)
    ya = r.run(np.ascontiguousarray(u[:, :25]), time_major=True)
    r.set_models(1, [models[0]])
    r.set_models(2, [models[2]])                            # (the batch moves to the plain shape: a new batch takes the measurement over)
    yb = r.run(np.ascontiguousarray(u[:, 25:]), time_major=True)
    assert_events(r, window(np.concatenate([ya, yb], axis=1), 10, 45), lo, hi, 2)
    e = r.measurement_events()
    assert np.array_equal(e.lo, lo) and np.array_equal(e.hi, hi)


def check_errors(mk):
    """every refusal with its code and the argument's name in the message"""
    from acme_jl_amd.runner import AcmeError, DimensionMismatch, _dp
    m = X.wire_model(1, FS)
    u = np.zeros((3, 10, 1))
    ok_lo, ok_hi = np.full((2, 3), -1.0), np.full((2, 3), 1.0)

    def refused(r, code, what, nC, lo, hi, E):
        la = None if lo is None else np.ascontiguousarray(lo, dtype=np.float64)
        ha = None if hi is None else np.ascontiguousarray(hi, dtype=np.float64)
        rc = r.lib.L.acme_batch_set_measurement_events(r.h, nC, None if la is None else _dp(la), None if ha is None else _dp(ha), E)
        msg = r.lib.L.acme_last_error().decode()
        assert rc == code and all(w in msg for w in what), (nC, lo, hi, E, rc, msg)
    r = mk(m, 3)
    refused(r, -1, ["no measurement is armed"], 2, ok_lo, ok_hi, 4)
    r.set_measurement(start=1)
    for nC in (0, -1, MAX_LEVELS + 1):
        refused(r, -1, ["C", str(MAX_LEVELS)], nC, ok_lo, ok_hi, 4)
    for E in (-1, MAX_SLOTS + 1):
        refused(r, -1, ["E", str(MAX_SLOTS)], 2, ok_lo, ok_hi, E)
    refused(r, -1, ["lo", "NULL"], 2, None, ok_hi, 4)
    refused(r, -1, ["hi", "NULL"], 2, ok_lo, None, 4)
    for bad in (np.nan, np.inf, -np.inf):
        lo = ok_lo.copy()
        lo[1, 2] = bad
        refused(r, -1, ["lo", "level 1", "instance 2", "finite"], 2, lo, ok_hi, 4)
        hi = ok_hi.copy()
        hi[0, 1] = bad
        refused(r, -1, ["hi", "level 0", "instance 1", "finite"], 2, ok_lo, hi, 4)
    lo = ok_lo.copy()
    lo[1, 0] = 1.5
    refused(r, -1, ["lo > hi", "level 1", "instance 0"], 2, lo, ok_hi, 4)
    assert r.lib.L.acme_batch_get_measurement_events(r.h, None, None, None, None) == -1     # (refused events leave none behind)
    r.set_measurement_events(lo=ok_lo, hi=ok_lo, slots=0)   # lo == hi and E = 0 are accepted
    r.measure(u, time_major=True)
    refused(r, -1, ["samples have been fed"], 2, ok_lo, ok_hi, 4)
    r.reset_measurement()
    # a series and events exclude each other, whichever is set first
    assert r.lib.L.acme_batch_set_measurement_series(r.h, 4, 4, 2) == -2 and "events" in r.lib.L.acme_last_error().decode()
    with pytest.raises(AcmeError, match="events"):
        r.set_measurement_series(4, 4, 2)
    r.set_measurement(start=1).set_measurement_series(4, 4, 2)
    refused(r, -2, ["series"], 2, ok_lo, ok_hi, 4)
    # the Python layer's own refusals
    r.set_measurement(start=1)
    with pytest.raises(DimensionMismatch):
        r.set_measurement_events(np.zeros((2, 4)))
    with pytest.raises(DimensionMismatch):
        r.set_measurement_events(lo=np.zeros((2, 3)), hi=np.zeros((1, 3)))
    with pytest.raises(ValueError, match="levels"):
        r.set_measurement_events()
    with pytest.raises(ValueError, match="levels"):
        r.set_measurement_events(0.0, lo=[0.0], hi=[0.0])
    with pytest.raises(ValueError, match="hysteresis"):
        r.set_measurement_events(0.0, hysteresis=-1.0)


def check_cap(mk, accept):
    """one record beyond N nrows C (E + 1) = ACME_MAX_EVENTS is refused, by the arming call alone; ``accept``: the cap itself
    is accepted and cleared at once"""
    N, nC, E = CAP // (8 * 16), 8, 15
    assert N * nC * (E + 1) == CAP
    r = mk(X.wire_model(1, FS), N).set_measurement()
    lo = np.zeros((nC, N))
    rc = r.lib.L.acme_batch_set_measurement_events(r.h, nC, lo.ctypes.data_as(C.POINTER(C.c_double)), lo.ctypes.data_as(C.POINTER(C.c_double)), E + 1)
    msg = r.lib.L.acme_last_error().decode()
    assert rc == -1 and "N nrows C (E + 1)" in msg and str(CAP) in msg, (rc, msg)
    if not accept:
        return
    r.set_measurement_events(lo=lo, hi=lo, slots=E)
    count = C.c_longlong(-1)
    assert r.lib.L.acme_batch_get_measurement_events(r.h, None, None, None, C.byref(count)) == 0 and count.value == 0
    r.clear_measurement()


def check_two_shards(mk_multi, mk, N=70, T=1000):
    """``MultiDeviceRunner`` over two shards == the single runner"""
    u, amp = signal(mk, "sine 64 then 63", N, T)
    m = X.wire_model(1, FS)
    lo, hi = levels_for("noise", amp, 3)
    one = mk(m, N).set_measurement(start=3, length=900).set_measurement_events(lo=lo, hi=hi, slots=5)
    one.measure(u, time_major=True)
    md = mk_multi(m, N)
    md.set_measurement(start=3, length=900).set_measurement_events(lo=lo, hi=hi, slots=5).measure(u)
    a, b = one.measurement_events(), md.measurement_events()
    assert a.count == b.count == 900 and a.rows == b.rows
    for k in ("counts", "idx", "lo", "hi"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert np.array_equal(bits(a.ab), bits(b.ab)) and a.counts[..., :2].sum() > 0
    # levels as a scalar and as [C] on every shard
    for lv in (0.0, [-0.01, 0.02]):
        md.set_measurement(start=3, length=900).set_measurement_events(lv, hysteresis=0.01, slots=2).measure(u)
        one.set_measurement(start=3, length=900).set_measurement_events(lv, hysteresis=0.01, slots=2).measure(u, time_major=True)
        assert np.array_equal(md.measurement_events().idx, one.measurement_events().idx)


# ---- 7. a circuit ---------------------------------------------------------------------------------------------------------------
def check_circuit(mk, N=16, periods=104, P=45):
    """the diode clipper over a level sweep behind a sine source of ``P`` samples a period (f_num / f_den = 1 / P), levels at 0
    and at +- a quarter of each instance's drive: events == the replay on the stored y; ``frequency()`` is f_num / f_den fs to
    1e-9 relative (the output is periodic to the solver's tolerance, and the first and the last rise lie whole periods apart,
    so the interpolation's error at the two ends cancels to that); the duty at the level 0 lies in (0.45, 0.55) -- the clipper is
    asymmetric, a plausibility band and no precision claim.

    The window's length follows from that tolerance.  At the drives where one Newton step meets the solver's tolerance (0.2 to
    0.3 V here) consecutive periods of the stored y differ by up to 5e-8 V and do not converge further -- the harder driven
    instances iterate to the last bit and repeat exactly.  At a zero crossing of slope 2 pi A / P per sample (A about 0.28 V)
    that moves a crossing by up to 1.3e-6 samples at either end, so over K whole periods the frequency is off by up to
    2.6e-6 / (K P) relative: 6.4e-9 over the 9 periods a short window would hold (3.9e-9 was measured over 8), 5.7e-10 over
    the K = 100 periods measured here."""
    m = clipper()
    T = P * periods
    amp = np.logspace(-1, 0.7, N)
    src = dict(kind="sine", f_den=P, f_num=np.full(N, 1), amp=amp)
    start, length = 4 * P, T - 4 * P                        # whole periods behind four periods of settling
    lo, hi = levels2([0.0], [0.0], N)
    lo = np.concatenate([lo, -0.25 * amp[None], 0.25 * amp[None]])
    hi = lo.copy()
    y = sr.apply_sources(mk(m, N), [src]).run_sources(T)
    r = sr.apply_sources(mk(m, N), [src]).set_measurement(start=start, length=length).set_measurement_events(lo=lo, hi=hi, slots=4)
    r.measure(T=T)
    cnt, idx, ab = assert_events(r, window(y, start, length), lo, hi, 4)
    e = r.measurement_events()
    crosses = cnt[:, 0, 0, RISE] >= 2
    assert crosses.all()                                    # (every instance's output swings through 0)
    f = e.frequency(FS, 0)[:, 0]
    assert (np.abs(f[crosses] - FS / P) <= 1e-9 * FS / P).all(), (f - FS / P) / (FS / P)
    duty = e.duty(0)[:, 0]
    assert ((duty > 0.45) & (duty < 0.55)).all(), duty
    # the rise time between the lower and the upper level is positive and below a quarter period where both are crossed
    both = (cnt[:, 0, 1, RISE] > 0) & (cnt[:, 0, 2, RISE] > 0)
    tt = e.transition_time(1, 2, "rise")[:, 0]
    assert both.any() and np.isnan(tt[~both]).all()
    return e, f, duty


# ---- the result object ----------------------------------------------------------------------------------------------------------
def check_object(mk):
    from acme_jl_amd.runner import MeasurementEvents
    u = np.array([[-1.0, 1.0, -1.0, 3.0, -1.0, 1.0, 1.0, -3.0], [0.5] * 8, [-1.0] * 8])[:, :, None]
    r = mk(X.wire_model(1, FS), 3).set_measurement().set_measurement_events([0.0, 2.0], slots=2)
    r.measure(np.ascontiguousarray(u), time_major=True)
    e = r.measurement_events()
    assert e.count == 8 and e.levels == 2 and e.slots == 2 and e.rows == (0,)
    assert e.counts.shape == (3, 1, 2, 5) and e.idx.shape == (3, 1, 2, 2, 3) and e.ab.shape == (3, 1, 2, 2, 3, 2)
    assert e.rises[:, 0].tolist() == [[3, 1], [0, 0], [0, 0]] and e.falls[:, 0].tolist() == [[3, 1], [0, 0], [0, 0]]
    assert e.high[:, 0].tolist() == [[4, 1], [8, 0], [0, 0]] and e.low[:, 0].tolist() == [[4, 7], [0, 8], [8, 8]]
    assert e.unknown[:, 0].tolist() == [[0, 0]] * 3
    t, last = e.times("rise", 0)
    assert t.shape == (3, 1, 2) and t[0, 0].tolist() == [0.5, 2.25] and last[0, 0] == 4.5 and np.isnan(t[1:]).all() and np.isnan(last[1:]).all()
    t, last = e.times("fall", 1)
    assert t[0, 0, 0] == 3.0 + (2.0 - 3.0) / (-1.0 - 3.0) and np.isnan(t[0, 0, 1]) and last[0, 0] == t[0, 0, 0]
    assert e.frequency(8.0, 0)[0, 0] == 8.0 * 2 / (4.5 - 0.5) and np.isnan(e.frequency(8.0, 1)).all()
    assert e.duty(0)[:, 0].tolist() == [0.5, 1.0, 0.0] and e.duty(1)[0, 0] == 0.125
    assert e.transition_time(0, 1, "rise")[0, 0] == (2.0 + 3.0 / 4.0) - 0.5 and np.isnan(e.transition_time(0, 1, "rise")[1:]).all()
    assert e.last_time(0)[0, 0] == 6.0 + 1.0 / 4.0 and np.isnan(e.last_time(0)[1:]).all()
    j = MeasurementEvents.concatenate([e, e])
    assert j.counts.shape == (6, 1, 2, 5) and j.count == 8 and j.lo.shape == (2, 6) and np.array_equal(j.idx[3:], e.idx)
    other = MeasurementEvents(e.counts, e.idx, e.ab, 9, e.lo, e.hi, e.rows)
    with pytest.raises(ValueError, match="differ"):
        MeasurementEvents.concatenate([e, other])
