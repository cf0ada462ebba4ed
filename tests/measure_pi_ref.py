"""Shared by the emulator and GPU tests of per-instance measurement fundamentals
(acme_batch_set_measurement_per_instance): the shared-frequency measurement as the reference instance by instance, the
exact pins of exact_ref per instance, and the analytic transfer function of a linear fixture."""
import numpy as np

import exact_ref as X
from test_measurement import raw


def shared_by_frequency(fresh, feed, f_den, f_num, spec):
    """{f: (out, count)}: the shared measurement (acme_batch_set_measurement at f / f_den) on an identical run, once per
    distinct frequency.  ``fresh()`` makes the runner, ``feed(r)`` runs it."""
    ref = {}
    for f in sorted(set(int(v) for v in f_num)):
        r = fresh().set_measurement(f0=(f, f_den) if spec.get("harmonics") else None, **spec)
        feed(r)
        ref[f] = raw(r)
    return ref


def assert_instance_by_instance(got, f_num, ref):
    """instance i of the per-instance batch == instance i of the shared run at f_num[i], bit for bit"""
    out, count = got
    f_num = np.asarray(f_num)
    for f, (o, c) in ref.items():
        idx = f_num == f
        assert idx.any() and c == count, f
        assert np.array_equal(out[idx], o[idx], equal_nan=True), (f, np.argwhere(out[idx] != o[idx])[:8])


def wave_kinds(r):
    """(uniform waves, mixed waves) of the armed plan; the permutation is one"""
    plan = r.measurement_plan()
    assert sorted(plan["perm"].tolist()) == list(range(len(plan["perm"])))
    wg = plan["wave_group"]
    return int((wg >= 0).sum()), int((wg < 0).sum())


def check_exact_per_instance(out, count, seg, f_den, f_num, H):
    """out [N, rows, 4 + 2H] of the window's samples seg [N, n, rows]: moments bit for bit, C_h / S_h of instance i within
    exact_ref.harmonic_bound of sums with mpmath twiddles at f_num[i].  Returns the worst |error| / bound."""
    N, n, rows = seg.shape
    assert count == n and out.shape == (N, rows, 4 + 2 * H)
    s, sq, mn, mx = X.exact_moments(seg)
    mean, rms = X.reported((s, sq), n)
    for name, got, want in (("mean", out[:, :, 0], mean), ("rms", out[:, :, 1], rms), ("min", out[:, :, 2], mn), ("max", out[:, :, 3], mx)):
        assert np.array_equal(got, want, equal_nan=True), (name, np.argwhere(got != want)[:8])
    gc, gs = X.unscale(out, n)
    worst = 0.0
    for f in sorted(set(int(v) for v in f_num)):
        idx = np.flatnonzero(np.asarray(f_num) == f)
        C_, S_, l1 = X.ld_harmonics(seg[idx], (f, f_den), H)
        bound = X.harmonic_bound(n, l1)[:, :, None]
        ec, es = np.abs(gc[idx] - C_) / bound, np.abs(gs[idx] - S_) / bound
        w = float(max(ec.max(), es.max()))
        print(f"harmonics: f_num {f} / {f_den} H {H} n {n}: max |error| / bound {w:.2e}")
        assert w <= 1.0, (f, w)
        if f == 0:          # th = 0 at every sample: C_h is the sum, S_h a sum of zeros
            inv = 1.0 / n
            for h in range(1, H + 1):
                assert np.array_equal(out[idx][:, :, 2 + 2 * h], 2.0 * s[idx] * inv) and not out[idx][:, :, 3 + 2 * h].any()
        worst = max(worst, w)
    return worst


# ---- a Bode plot in one batch ------------------------------------------------------------------------------------------------
BODE_START = {"rc_ladder": 2942, "sallenkey": 172}      # S >= ln(1e-17) / ln rho(a): rho = 0.98678, 0.79633
BODE_ATOL = 1e-12                                        # absolute, x the source's amplitude (1)


def bode_expected(m, f_den, f_num, start):
    """A_1 of the steady-state response to sin(2 pi f_num n / f_den) measured from sample ``start`` over whole periods:
    H(e^{jw}) (-j) e^{j 2 pi ((f_num start) mod f_den) / f_den}, H(z) = dy (zI - a)^-1 b + ey"""
    a, b, dy, ey = (np.asarray(v, dtype=np.float64) for v in (m.a, m.b, m.dy, m.ey))
    assert not np.asarray(m.x0, dtype=np.float64).any() and not np.asarray(m.y0, dtype=np.float64).any()
    out = np.empty(len(f_num), dtype=np.complex128)
    for i, f in enumerate(int(v) for v in f_num):
        z = np.exp(2j * np.pi * f / f_den)
        h = (dy @ np.linalg.solve(z * np.eye(a.shape[0]) - a, b) + ey)[0, 0]
        out[i] = h * -1j * np.exp(2j * np.pi * ((f * start) % f_den) / f_den)
    return out


def bode_measured(r, f_den, f_num, start):
    """one instance per frequency: a unit sine source on input row 0, the measurement's fundamentals taken from it, a window
    of f_den samples after ``start``, y = NULL.  Returns A_1 [N]."""
    r.set_source(0, "sine", f_den=f_den, f_num=f_num)
    r.set_measurement(start=start, length=f_den, harmonics=1, f0_from_source=0)
    r.measure(T=start + f_den)
    mm = r.measurement()
    assert mm.count == f_den
    return mm.harmonics[:, 0, 0]
