"""The measurement spectrum at the headline shape: the superover grid (bench.py's superover_grid), 8 192 instances, the caching
solver stack, a 1 kHz sine at 44.1 kHz, H = 10, the one output row, device arrays, y stored (leg (b) of
tools/measurement_probe.py).  Seconds per second of audio for
  1   nothing armed;
  2   acme_batch_set_measurement at one shared frequency;
  3   leg 2 with a spectrum, L = 1024, hop 512, Hann;
  4   leg 2 with a spectrum, L = 4096, hop 2048, Hann;
  5   leg 2 with a spectrum, L = 64, hop 32, Hann;
  6   a GAUSSIAN source on the signal row (the pots as CONST sources), y = NULL, leg 2's measurement and leg 3's spectrum.
Steady state as measurement_probe.py defines it: 4 untimed steps, then the median of 4 timed ones; every leg runs twice, in
alternation.  One process; every leg runs under its own time limit (SIGALRM) and the first failure ends the run.  The
yardstick is the parent commit: --package-root names a checkout of it with its library built, and legs 1 and 2 run there
(--legs 1,2) as they do here.  Raw lines go to
--out (profiles/spectrum_probe.jsonl).  The spectrum kernel's own time: one leg under `rocprofv3 --kernel-trace --stats`
(acme_meas_spectrum_kernel), in a run of its own.

    python tools/spectrum_probe.py [--instances N] [--steps S] [--warmup W] [--legs 1,2,3,4,5,6] [--passes 2] [--limit SECONDS]
                                   [--package-root DIR] [--out FILE]
"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC = {"3": (1024, 512), "4": (4096, 2048), "5": (64, 32), "6": (1024, 512)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=4, help="untimed steps first (the first seconds of the signal cost more)")
    ap.add_argument("--legs", default="1,2,3,4,5,6")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120, help="seconds a leg may take")
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose package and library run (the parent's: legs 1,2)")
    ap.add_argument("--out", default=None, help="append the raw lines to this file")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    from acme_jl_amd.model import CachingHomotopySolver, DiscreteModel
    from acme_jl_amd.runner import ModelRunner
    legs = args.legs.split(",")
    N, fs, H = args.instances, 44100, 10
    if N % 256:
        raise SystemExit("the superover grid needs a multiple of 256 instances")

    def too_long(*_):
        raise SystemExit("a leg ran into its time limit: nothing more is started")
    signal.signal(signal.SIGALRM, too_long)

    m = DiscreteModel.load(os.path.join(ROOT, "tests", "golden", "superover_var.json"), CachingHomotopySolver)
    idx = np.arange(N)           # (bench.py superover_grid: level fastest, then tone, then drive)
    pots = np.stack([(idx // 256) / float(N // 256), ((idx // 16) % 16) / 15.0, (idx % 16) / 15.0], axis=1)
    signal.alarm(args.limit)
    ud = torch.empty((N, fs, 4), dtype=torch.float64, device="cuda")
    ud[:, :, 0] = torch.from_numpy(np.sin(2 * np.pi * 1000.0 / fs * np.arange(fs))).cuda()[None]
    ud[:, :, 1:] = torch.from_numpy(pots).cuda()[:, None, :]
    yd = torch.empty((N, fs, m.ny), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    signal.alarm(0)

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")

    results = []
    for p in range(args.passes):
        for leg in legs:
            signal.alarm(args.limit)
            T = fs
            r = ModelRunner(m, N, device=0)
            line = dict(leg=leg, **{"pass": p}, instances=N, samples=T, harmonics=H, package=os.path.basename(os.path.abspath(args.package_root)))
            if leg == "6":
                r.set_source(0, "noise", dist="gaussian", amp=np.full(N, 0.01), seed=1)
                for row in (1, 2, 3):
                    r.set_source(row, "const", offset=pots[:, row - 1])
            if leg != "1":
                r.set_measurement(f0=(10, 441), harmonics=H)
            if leg in SPEC:
                r.set_measurement_spectrum(*SPEC[leg])
                line.update(nfft=SPEC[leg][0], hop=SPEC[leg][1], spectrum_gb=(SPEC[leg][0] + SPEC[leg][0] // 2 + 1) * N * 8 / 1e9)

            def step():
                if leg == "6":
                    r.measure(T=T)
                else:
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
            if leg in SPEC:
                sp = r.measurement_spectrum()
                line.update(segments=sp.segments, spectrum_count=sp.count, spectrum_finite=bool(np.isfinite(sp.power).all()),
                            line_1khz=float(np.median(sp.amplitude()[:, 0, round(1000 * SPEC[leg][0] / fs)])))
            if leg != "1":
                mm = r.measurement()
                line.update(count=mm.count, a1_median=float(np.median(np.abs(mm.harmonics[:, 0, 0]))))
            signal.alarm(0)
            emit(line)
            results.append(line)
            del r
    best = {}
    for x in results:
        best[x["leg"]] = min(best.get(x["leg"], np.inf), x["s_per_audio_s"])
    emit({"best_s_per_audio_s": best})


if __name__ == "__main__":
    main()
