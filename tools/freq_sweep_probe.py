"""Per-instance measurement fundamentals at the headline shape: the superover grid (bench.py's superover_grid), 8 192
instances, the caching solver stack, one second of a 1 kHz sine at 44.1 kHz per step, H = 10, the one output row, device
arrays, y stored (leg (b) of tools/measurement_probe.py).  Seconds per second of audio for
  a   nothing armed;
  b   acme_batch_set_measurement at one shared frequency;
  1   the per-instance form, F = 1;
  2   F = 32, frequency the slowest axis (256 consecutive instances a frequency: every wave uniform);
  3   F = 32, frequency the fastest axis (instance i: frequency i mod 32 -- the grouping has to earn it);
  4   F = N: every instance its own frequency (mixed waves throughout).
Steady state as measurement_probe.py defines it: 4 untimed seconds, then the median of 4 timed ones; every leg runs twice, in
alternation (pass 0 of every leg, then pass 1).  One process; every leg runs under its own time limit (SIGALRM) and the
first failure ends the run.  With a library that lacks the per-instance entry point (ACME_HIP_LIB = an older build: the
yardstick) run --legs a,b.  The measurement kernels' own time: run one leg under `rocprofv3 --kernel-trace --stats`
(acme_meas_pi_kernel, acme_meas_pi_tw_kernel), in a run of its own.

    python tools/freq_sweep_probe.py [--instances N] [--steps S] [--warmup W] [--legs a,b,1,2,3,4] [--passes 2] [--limit SECONDS]
"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frequencies(leg, N, f_den):
    """f_num [N] of a leg (all of them within 20 Hz ... 20 kHz at f_den = 44 100)"""
    tones = np.round(np.logspace(np.log10(100), np.log10(10000), 32)).astype(np.int64)
    if leg == "1":
        return np.full(N, 1000, dtype=np.int64)
    if leg == "2":
        return tones[np.arange(N) * 32 // N]
    if leg == "3":
        return tones[np.arange(N) % 32]
    return (20 + np.arange(N, dtype=np.int64)) % f_den


def main():
    import torch
    from acme_jl_amd.model import CachingHomotopySolver, DiscreteModel
    from acme_jl_amd.runner import ModelRunner
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=4, help="untimed seconds first (the first seconds of the signal cost more)")
    ap.add_argument("--legs", default="a,b,1,2,3,4")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120, help="seconds a leg may take")
    args = ap.parse_args()
    legs = args.legs.split(",")
    N, fs, H = args.instances, 44100, 10
    T = fs
    if N % 256:
        raise SystemExit("the superover grid needs a multiple of 256 instances")

    def too_long(*_):
        raise SystemExit("a leg ran into its time limit: nothing more is started")
    signal.signal(signal.SIGALRM, too_long)

    m = DiscreteModel.load(os.path.join(ROOT, "tests", "golden", "superover_var.json"), CachingHomotopySolver)
    idx = np.arange(N)           # (bench.py superover_grid: level fastest, then tone, then drive)
    pots = np.stack([(idx // 256) / float(N // 256), ((idx // 16) % 16) / 15.0, (idx % 16) / 15.0], axis=1)
    signal.alarm(args.limit)
    ud = torch.empty((N, T, 4), dtype=torch.float64, device="cuda")
    ud[:, :, 0] = torch.from_numpy(np.sin(2 * np.pi * 1000.0 / fs * np.arange(T))).cuda()[None]
    ud[:, :, 1:] = torch.from_numpy(pots).cuda()[:, None, :]
    yd = torch.empty((N, T, m.ny), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    signal.alarm(0)

    results = []
    for p in range(args.passes):
        for leg in legs:
            signal.alarm(args.limit)
            r = ModelRunner(m, N, device=0)
            line = dict(leg=leg, **{"pass": p}, instances=N, samples=T, harmonics=H)
            if leg == "b":
                r.set_measurement(f0=(10, 441), harmonics=H)
            elif leg != "a":
                r.set_measurement(f_den=fs, f_num=frequencies(leg, N, fs), harmonics=H)
                plan = r.measurement_plan()
                line.update(groups=plan["groups"], chunk=plan["chunk"], table_mb=plan["groups"] * H * plan["chunk"] * 16 / 2 ** 20,
                            uniform_waves=int((plan["wave_group"] >= 0).sum()), mixed_waves=int((plan["wave_group"] < 0).sum()))

            def step():
                r.run_device(ud.data_ptr(), yd.data_ptr(), T, torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
            for _ in range(args.warmup):
                step()
            r.kernel_time(reset=True)
            times = []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                step()
                times.append(time.perf_counter() - t0)
            r.check()
            run_ms, launches = r.kernel_time()
            line.update(s_per_audio_s=float(np.median(times)) * fs / T, times=times, run_kernel_ms_per_step=run_ms / args.steps,
                        run_launches_per_step=launches / args.steps)
            if leg != "a":
                mm = r.measurement()
                line.update(count=mm.count, a1_median=float(np.median(np.abs(mm.harmonics[:, 0, 0]))))
            signal.alarm(0)
            print(json.dumps(line), flush=True)
            results.append(line)
            del r
    best = {}
    for x in results:
        best[x["leg"]] = min(best.get(x["leg"], np.inf), x["s_per_audio_s"])
    if "a" in best:
        print(json.dumps({f"{k}_over_a": v / best["a"] for k, v in best.items() if k != "a"}))


if __name__ == "__main__":
    main()
