"""Shared by the emulator and GPU tests of the multisine source (acme_batch_set_source_multisine) and of measurement bins
(acme_batch_set_measurement_bins): the tone chain against mpmath at phases reduced in unbounded integers, the bins' reduced
frequencies in unbounded integers, and the two identities the bins are held to -- bin b of instance i is harmonic 1 of the
shared measurement at k[b][i], and one tone with coefficients 1 ... B is the per-instance form."""
import numpy as np

import exact_ref as X
import measure_pi_ref as PI
import source_ref as sr
from test_measurement import raw


# ---- the source ---------------------------------------------------------------------------------------------------------------
def tone_par(a, tones, N, default):
    """a per-tone parameter as [tones, N]: None, (tones,) or (tones, N)"""
    if a is None:
        return np.full((tones, N), default)
    a = np.asarray(a)
    return np.broadcast_to(a[:, None] if a.ndim == 1 else a, (tones, N))


def multisine_bound(amps, offset):
    """Bound on |rendered - (offset + sum_k amp_k sin th_k) evaluated exactly| for one MULTISINE element, derived as
    source_ref.sine_bound is: (12 sum_k |amp_k| + sum_k (|offset| + sum_{j <= k} |amp_j|)) 2^-53.  Per tone 12 units of
    |amp_k| for the angle's two roundings, the constant 2 pi and the device's sin (source_ref.sine_bound), plus one rounding
    of each partial sum of the fma chain, which |offset| + sum_{j <= k} |amp_j| bounds.  One tone: sine_bound."""
    a = np.abs(np.asarray(amps, dtype=np.float64))
    return float(12.0 * a.sum() + sum(abs(offset) + a[:k + 1].sum() for k in range(len(a)))) * X.U


def multisine_error(got, amps, offset, f_nums, phases, f_den, n):
    """|got - (offset + sum_k amp_k sin(2 pi kappa_k / f_den))| with the right-hand side at 120 bits"""
    import mpmath
    with mpmath.workprec(120):
        want = mpmath.mpf(float(offset))
        for a, f, p in zip(amps, f_nums, phases):
            want += mpmath.mpf(float(a)) * sr.exact_sine(int(f), int(p), f_den, n)
        return float(abs(mpmath.mpf(float(got)) - want))


def check_multisine_row(got, k, N, n0, samples):
    """got [N, T] of the row described by k (dict: f_den, f_num, phase, amp [tones, N] or [tones], offset [N]) against mpmath
    at the (instance, sample) pairs of ``samples``; returns the worst error in units of its bound (asserts it is at most 1)"""
    f_num = np.asarray(k["f_num"])
    tones = f_num.shape[0]
    fn, ph = tone_par(f_num, tones, N, 0), tone_par(k.get("phase"), tones, N, 0)
    amp, off = tone_par(k.get("amp"), tones, N, 1.0), sr.par(k.get("offset"), N, 0.0)
    worst = 0.0
    for i, t in samples:
        err = multisine_error(got[i, t], amp[:, i], off[i], fn[:, i], ph[:, i], k["f_den"], n0 + t)
        bound = multisine_bound(amp[:, i], off[i])
        worst = max(worst, err / bound)
        assert err <= bound, (i, t, n0, float(got[i, t]), err / X.U, bound / X.U)
    return worst


def awkward_tones(tones, N, rng, f_den=sr.PRIME_DEN):
    """``tones`` tones of prime f_den near 2^31 with f_num near f_den, phases all over, amplitudes over six decades"""
    f_num = np.stack([f_den - 1 - (3 + 1000003 * k) * (1 + np.arange(N)) for k in range(tones)]) % f_den
    phase = np.stack([(np.arange(N) * 715827881 + 97 * k) % f_den for k in range(tones)])
    amp = rng.standard_normal((tones, N)) * 10.0 ** rng.integers(-3, 4, (tones, N))
    return dict(kind="multisine", f_den=f_den, f_num=f_num, phase=phase, amp=amp, offset=rng.standard_normal(N))


def two_tone(N, f_den, f1=19000, f2=20000, level=None):
    """a CCIF-like pair at per-instance level (both tones the same amplitude), tone 1 a quarter turn ahead"""
    level = np.logspace(-1, 0.3, N) if level is None else level
    return dict(kind="multisine", f_den=f_den, f_num=np.array([f1, f2]), phase=np.array([0, f_den // 4]),
                amp=np.stack([level, level]))


# ---- the bins -------------------------------------------------------------------------------------------------------------------
def bin_frequencies(coef, f_num, f_den):
    """k [B, N] = (sum_j coef[b][j] f_num[j][i]) mod f_den, the non-negative residue, in unbounded integers"""
    coef, f_num = np.asarray(coef), np.asarray(f_num)
    B, N = coef.shape[0], f_num.shape[1]
    k = np.zeros((B, N), dtype=np.int64)
    for b in range(B):
        for i in range(N):
            k[b, i] = sum(int(c) * int(f) for c, f in zip(coef[b], f_num[:, i])) % int(f_den)
    return k


def shared_by_bin(fresh, feed, f_den, kb, spec):
    """{k: (out, count)}: acme_batch_set_measurement(f_num = k, f_den, harmonics = 1) on an identical run, once per distinct
    reduced bin frequency"""
    return PI.shared_by_frequency(fresh, feed, f_den, np.unique(kb), dict(spec, harmonics=1))


def assert_bin_by_bin(got, kb, ref):
    """bin b of instance i == harmonic 1 of the shared run at k[b][i]; the four moments == the shared run's, bit for bit"""
    out, count = got
    B, N = kb.shape
    assert out.shape[2] == 4 + 2 * B
    for k, (o, c) in ref.items():
        assert c == count, k
        assert np.array_equal(out[:, :, :4], o[:, :, :4], equal_nan=True), ("moments", k)
        for b in range(B):
            idx = kb[b] == k
            if idx.any():
                g, w = out[idx][:, :, 4 + 2 * b:6 + 2 * b], o[idx][:, :, 4:6]
                assert np.array_equal(g, w, equal_nan=True), (k, b, np.argwhere(g != w)[:8])
    assert set(np.unique(kb).tolist()) == set(ref)


# two tones, six bins: both fundamentals, the difference either way round (the second wraps below zero where f2 > f1), a
# third-order product and a bin at 0
COEF6 = np.array([[1, 0], [0, 1], [-1, 1], [1, -1], [2, -1], [0, 0]])


def tone_cases(f_den=441):
    """name -> (f_num [2, N], (uniform, mixed) waves of a one-row measurement): the grouping of measure_pi_ref's cases by
    tone PAIR.  F = N keeps f2 - f1 = 7 for every instance: 130 groups, few distinct bin frequencies."""
    rng = np.random.default_rng(3)
    pairs = np.array([[40, 47]] * 200 + [[47, 40]] * 7 + [[40, 40]])[rng.permutation(208)].T
    n = np.arange(130)
    return {"F1": (np.stack([np.full(130, 19), np.full(130, 20)]), (3, 0)),
            "F3-200-7-1": (pairs, (3, 1)),
            "F=N": (np.stack([1 + n, 8 + n]), (0, 3))}


def check_bins_against_shared(mk, m, f_num, kinds_want, f_den, T, spec, coef=COEF6):
    """the diode clipper driven by a MULTISINE row at f_num, measured in bins; then the shared measurement once per distinct
    k on the rendered input"""
    N = f_num.shape[1]
    kb = bin_frequencies(coef, f_num, f_den)
    src = dict(kind="multisine", f_den=f_den, f_num=f_num, amp=np.stack([np.logspace(-1, 0.4, N)] * 2))
    r = sr.apply_sources(mk(m, N), [src])
    u = r.render_sources(T)
    r.set_measurement_bins(coef, tones_from_source=0, **spec)
    assert PI.wave_kinds(r) == kinds_want, PI.wave_kinds(r)
    assert r.measurement_plan()["groups"] == len(set(map(tuple, f_num.T.tolist())))
    r.measure(T=T)
    got = raw(r)
    ref = shared_by_bin(lambda: mk(m, N), lambda q: q.measure(u, time_major=True), f_den, kb, spec)
    assert_bin_by_bin(got, kb, ref)
    zero = np.argwhere(kb == 0)
    assert len(zero)
    for b, i in zero:               # k = 0: C = the sum, S = 0 exactly
        assert np.array_equal(got[0][i, :, 4 + 2 * b], 2.0 * got[0][i, :, 0]) and not got[0][i, :, 5 + 2 * b].any()
    return got, kb


def check_exact_bins(out, count, seg, f_den, kb):
    """the pass-through model: moments bit for bit, C_b / S_b within exact_ref.harmonic_bound of sums with mpmath twiddles at
    k[b][i] (measure_pi_ref.check_exact_per_instance, bin by bin as a one-harmonic result)"""
    worst = 0.0
    for b in range(kb.shape[0]):
        one = np.concatenate([out[:, :, :4], out[:, :, 4 + 2 * b:6 + 2 * b]], axis=2)
        worst = max(worst, PI.check_exact_per_instance(one, count, seg, f_den, kb[b], 1))
    return worst


def check_superposition(mk, m, name, f_den, pairs, amps):
    """a linear fixture, one instance per tone pair, a window of f_den samples after BODE_START: the bins (1, 0) and (0, 1)
    are the transfer function at their tone times the tone's amplitude, every product bin is 0 -- each within BODE_ATOL x
    the sum of the tone amplitudes.  Returns the worst error over that."""
    S = PI.BODE_START[name]
    coef = np.array([[1, 0], [0, 1], [1, 1], [-1, 1], [2, -1], [-1, 2]])
    N = pairs.shape[1]
    r = mk(m, N)
    r.set_source(0, "multisine", f_den=f_den, f_num=pairs, amp=amps)
    r.set_measurement_bins(coef, start=S, length=f_den, tones_from_source=0)
    r.measure(T=S + f_den)
    mm = r.measurement()
    assert mm.count == f_den
    A = mm.bins[:, 0, :]
    tol = PI.BODE_ATOL * amps.sum(axis=0)
    kb = bin_frequencies(coef, pairs, f_den)
    worst = 0.0
    for j in range(2):
        assert not (kb[2:] == kb[j]).any() and (kb[j] != 0).all()       # (no product falls on a tone)
        err = np.abs(A[:, j] - amps[j] * PI.bode_expected(m, f_den, pairs[j], S))
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), (name, j, err.max())
    err = np.abs(A[:, 2:])
    worst = max(worst, float((err / tol[:, None]).max()))
    assert (err <= tol[:, None]).all(), (name, err.max())
    assert np.allclose(mm.imd([0, 1], [2, 3, 4, 5]), np.sqrt((np.abs(A[:, 2:]) ** 2).sum(1) / (np.abs(A[:, :2]) ** 2).sum(1))[:, None])
    return worst
