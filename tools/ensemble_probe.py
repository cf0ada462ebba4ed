"""The measurement ensemble in use and under the clock: a Monte-Carlo-sized batch of the diode clipper -- N instances, one drive
level each, a 1 kHz sine source at 44.1 kHz generated on the device -- whose band over the instances is read with neither u
nor y stored; N = 8 192, T = 44 100 per step, the one output row, H = 0 (the moments unit of acme_meas_kernel alone walks the
same y with four chains).  Seconds per second of audio for
  1   the measurement alone, the window the whole step (runs on the parent commit too: --package-root);
  2   leg 1 with an ensemble of ONE group, stride 1 (E = 44 100 slots; per chunk 64 tiles: the chains split over the waves);
  3   leg 1 with G = 64 groups of 128 members, stride 1;
  4   G = N one-member groups at stride 1 over a window of 2 048 samples -- the waveforms of all instances kept, the longest
      window the cap G nrows E <= 2^24 admits at N = 8 192;
  5   the measurement alone over leg 4's window (runs on the parent commit too).
`--split 0 / 1` forces the kernel's shape (ACME_ENS_SPLIT) for an A/B of leg 2.  Steady state: `--warmup` untimed steps, then
the median of `--steps` timed ones; every leg runs `--passes` times, in alternation.  One process; every leg runs under its own
time limit (SIGALRM) and the first failure ends the run.  Raw lines go to --out.  The kernels' own times: one leg under
`rocprofv3 --kernel-trace --stats` in a run of its own (acme_meas_ensemble_kernel beside acme_meas_kernel, per chunk of 4 096
samples).

    python tools/ensemble_probe.py [--instances N] [--steps S] [--warmup W] [--legs 1,2,3,4,5] [--passes 2] [--split auto]
                                   [--limit SECONDS] [--package-root DIR] [--out FILE]
"""
import argparse
import json
import os
import signal
import sys
import time
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="1,2,3,4,5")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--split", default="auto", choices=["auto", "0", "1"], help="the ensemble kernel's shape (ACME_ENS_SPLIT)")
    ap.add_argument("--limit", type=int, default=120, help="seconds a leg may take")
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose package and library run (the parent's: legs 1, 5)")
    ap.add_argument("--out", default=None, help="append the raw lines to this file")
    args = ap.parse_args()
    if args.split != "auto":
        os.environ["ACME_ENS_SPLIT"] = args.split
    sys.path.insert(0, os.path.abspath(args.package_root))
    from acme_jl_amd import examples
    from acme_jl_amd.model import DiscreteModel
    from acme_jl_amd.runner import ModelRunner
    N, fs, T = args.instances, 44100, 44100
    short = max(1, min(T, (1 << 24) // N))       # leg 4's window: G nrows E at the cap

    def too_long(*_):
        raise SystemExit("a leg ran into its time limit: nothing more is started")
    signal.signal(signal.SIGALRM, too_long)

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")

    m = DiscreteModel(examples.diodeclipper(), Fraction(1, fs), "HomotopySolver{CachingSolver{SimpleSolver}}")
    amp = np.logspace(-1, 0.7, N)
    results = []
    for p in range(args.passes):
        for leg in args.legs.split(","):
            signal.alarm(args.limit)
            r = ModelRunner(m, N, device=0)
            r.set_source(0, "sine", f_den=441, f_num=10, amp=amp)
            length = short if leg in ("4", "5") else T
            r.set_measurement(length=length)
            line = dict(leg=leg, **{"pass": p}, instances=N, samples=T, window=length, split=args.split,
                        package=os.path.basename(os.path.abspath(args.package_root)))
            if leg == "2":
                r.set_measurement_ensemble()
            elif leg == "3":
                r.set_measurement_ensemble(np.arange(N) // max(1, N // 64), 64)
            elif leg == "4":
                r.set_measurement_ensemble(np.arange(N), N)

            def step():
                r.reset_measurement()
                r.source_clock = 0
                r.measure(T=T)
                r.measurement()                 # (the getter synchronises)
            for _ in range(args.warmup):
                step()
            r.kernel_time(reset=True)
            times = []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                step()
                times.append(time.perf_counter() - t0)
            run_ms, launches = r.kernel_time()
            line.update(s_per_audio_s=float(np.median(times)) * fs / T, times=times, run_kernel_ms_per_step=run_ms / args.steps,
                        run_launches_per_step=launches / args.steps, count=r.measurement().count)
            if leg in ("2", "3", "4"):
                e = r.measurement_ensemble()
                lo, hi = e.band()
                line.update(filled=e.filled, groups=len(e.members), members=int(e.members[0]),
                            band_peak=float(hi.max()), band_trough=float(lo.min()), mean_rms=float(np.sqrt(np.mean(e.mean()[0, 0] ** 2))),
                            std_max=float(e.std().max()), worst_case_instances=int(len(np.unique(e.argmax[0, 0]))))
            signal.alarm(0)
            emit(line)
            results.append(line)
            del r
    fastest = {}
    for x in results:
        fastest[x["leg"]] = min(fastest.get(x["leg"], np.inf), x["s_per_audio_s"])
    emit({"best_s_per_audio_s": fastest})


if __name__ == "__main__":
    main()
