"""The condensed Newton loop's two bookkeeping paths (csrc/acme_kernel.h, base_solve_c): the usual pass -- every active
instance's pivots hold, no instance off the linear rows' subspace, no lane re-learnt -- takes a lean glue, anything else
the general one, and the choice is made per WAVE.  The cases here put both kinds of instance into the same wave and
check what must not depend on the choice.  Shared by test_emu_lean_pass.py (CPU wave emulator) and
test_gpu_lean_pass.py (-m gpu): same inputs, same oracle runs (computed once per process), same bars."""
import functools

import numpy as np

from helpers import HS, RTOL, load, moving_pot_inputs, sine

CACHING = "HomotopySolver{CachingSolver{SimpleSolver}}"
STACKS = ((HS, None), (CACHING, 16))        # (solver stack, the oracle's store bound: what the kernel implements)
MOVING = 1                                  # the instance of each wave of four whose potentiometers move every sample


def fixed_rows(n, T):
    """n instances spread over the interior of bench.py's drive x tone x level grid, pots fixed (the headline's inputs).
    Without the grid's two end cells: in the last one (the hardest) a rounding-level flip of a nearest-entry decision of
    the solution cache sends kernel and oracle through different, equally valid solves (6e-8 between them within 400
    samples, the kernel before the lean path existed included: test_gpu_headline.py bounds that regime at 8e-6)."""
    import bench
    N = 8192
    _, pots, amp = bench.grid_inputs("superover_grid", 0, 1, N, T)
    idx = np.linspace(0, N - 1, n + 2)[1:-1].astype(int)
    u = np.zeros((n, 4, T))
    u[:, 0] = amp * sine(T)
    u[:, 1:] = pots[idx][:, :, None]
    return u


def mixed_inputs(n, T, moving=True):
    """[n, 4, T]: fixed pots from the bench grid; with ``moving`` instance 1 of every wave of four takes rows whose
    pots move every sample (every one of its solves starts off the linear rows' subspace: the general path)"""
    u = fixed_rows(n, T)
    if moving:
        mv = moving_pot_inputs(n, T)
        for i in range(MOVING, n, 4):
            u[i] = mv[i]
    return u


@functools.lru_cache(maxsize=None)
def oracle(solver, lim, n, T, moving=True, maxiter=None):
    """(y [n, ny, T], iteration totals, warning counts) of the oracle, one fresh runner per instance"""
    from oracle.refpy import RefRunner
    m = load("superover_var", solver)
    u = mixed_inputs(n, T, moving)
    ys, its, warn = [], [], []
    for i in range(n):
        r = RefRunner(m)
        if lim is not None:
            r.set_cache_limit(lim)
        if maxiter is not None:
            r.set_maxiter(maxiter)
        ys.append(r.run(u[i]))
        its.append(r.report.iters_total)
        warn.append(r.report.n_warn)
    out = np.stack(ys), np.array(its), np.array(warn)
    for a in out:
        a.setflags(write=False)
    return out


def kernel_run(lib, solver, u, cuts=None, maxiter=None):
    from acme_jl_amd.runner import ModelRunner
    r = ModelRunner(load("superover_var", solver), u.shape[0], lib=lib, maxiter=maxiter)
    cuts = cuts or [0, u.shape[2]]
    y = np.concatenate([r.run(u[:, :, a:b], check=False) for a, b in zip(cuts[:-1], cuts[1:])], axis=2)
    return y, r.report_arrays()


def rel_err(y, yref):
    return float(np.abs(y - yref).max() / max(1.0, np.abs(yref).max()))


def check_mixed_waves(lib, n=8, T=400):
    """Both paths in every wave, both stacks: outputs at RTOL of the oracle; iteration totals per instance equal to the
    oracle's without the solution cache, within 10 % per instance and 1 % of the sum with it (the bars of
    test_gpu_headline.py's moving-pots test)."""
    u = mixed_inputs(n, T)
    for solver, lim in STACKS:
        yref, its, warn = oracle(solver, lim, n, T)
        y, ra = kernel_run(lib, solver, u)
        err = rel_err(y, yref)
        dev = np.abs(ra["iters_total"] - its) / its
        print(f"mixed waves, {solver}: rel err {err:.2e}, iteration totals {ra['iters_total'].tolist()} vs {its.tolist()}, "
              f"warnings {ra['n_warn'].sum()} vs {warn.sum()}")
        assert err <= RTOL
        assert (ra["first_nonfinite"] < 0).all()
        if lim is None:
            assert np.array_equal(ra["iters_total"], its)
        else:
            assert dev.max() <= 0.10
            assert abs(float(ra["iters_total"].sum()) - its.sum()) <= 0.01 * its.sum()


def check_wave_mates(lib, n=8, T=400):
    """What the three fixed instances of a wave compute does not depend on which path their wave-mate sends the wave
    down: the same batch with the moving instance replaced by a fixed one, bit for bit."""
    fixed = np.array([i for i in range(n) if i % 4 != MOVING])
    for solver, _ in STACKS:
        y1, r1 = kernel_run(lib, solver, mixed_inputs(n, T))
        y2, r2 = kernel_run(lib, solver, mixed_inputs(n, T, moving=False))
        assert np.array_equal(y1[fixed], y2[fixed]), solver
        assert np.array_equal(r1["iters_total"][fixed], r2["iters_total"][fixed]), solver
        assert not np.array_equal(y1[MOVING], y2[MOVING])       # (the two batches do differ)


def check_maxiter(lib, n=5, T=200):
    """Base solves cut short at three iterations (the loop's other exit; a partial second wave): warning counts and
    iteration totals as the oracle's, outputs at RTOL."""
    u = mixed_inputs(n, T)
    yref, its, warn = oracle(HS, None, n, T, maxiter=3)
    y, ra = kernel_run(lib, HS, u, maxiter=3)
    print(f"maxiter 3: rel err {rel_err(y, yref):.2e}, iteration totals {ra['iters_total'].tolist()} vs {its.tolist()}, "
          f"warnings {ra['n_warn'].tolist()} vs {warn.tolist()}")
    assert np.array_equal(ra["n_warn"], warn)
    assert np.array_equal(ra["iters_total"], its)
    assert rel_err(y, yref) <= RTOL


def check_split_launches(lib, n=8, T=400):
    """The mixed-wave run cut at samples 1 and 133: bit-identical to the uncut run, counters included."""
    u = mixed_inputs(n, T)
    for solver, _ in STACKS:
        y1, r1 = kernel_run(lib, solver, u)
        y2, r2 = kernel_run(lib, solver, u, cuts=[0, 1, 133, T])
        assert np.array_equal(y1, y2), solver
        for key in ("iters_total", "n_warn"):
            assert np.array_equal(r1[key], r2[key]), (solver, key)
