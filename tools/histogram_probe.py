"""The measurement histogram under the clock: N pairs of the pass-through model (a voltage source into a probe, y = u, one
output row) driven by a source generated on the device, so that the signal the histogram sees is the one named -- N = 8 192,
T = 44 100 per step (eleven chunks of 4 096 samples, one after another), H = 0 (the moments unit of acme_meas_kernel alone walks
the same y with four chains).  A leg is
  plain            the measurement alone (runs on the parent commit too: --package-root);
  fold             the measurement with a fold of period 441 (acme_meas_fold_kernel on the same y, the second yardstick);
  SIGNAL:B         the measurement with a histogram of B bins over (-1, 1): SIGNAL is `constant` (every lane of a wave in ONE
                   counter: a DC operating point, a hard-clipped rail), `sine` (1 kHz, amplitude 0.9: neighbouring lanes in
                   neighbouring counters) or `noise` (white, uniform in (-0.9, 0.9): every lane somewhere else).
`--agg 0 / 1` forces the kernel's shape (ACME_HIST_AGG: the runs of equal counters among neighbouring lanes aggregated ahead of
the LDS atomic, or one atomic per lane).  Seconds per second of audio, steady state: `--warmup` untimed steps, then the median
of `--steps` timed ones; every leg runs `--passes` times, in alternation.  One process; every leg runs under its own time
limit (SIGALRM) and the first failure ends the run.  Raw lines go to --out.  The kernels' own times: ONE leg under
`rocprofv3 --kernel-trace --stats` in a run of its own (acme_meas_hist_kernel beside acme_meas_kernel and, in the fold leg,
acme_meas_fold_kernel, per chunk of 4 096 samples).

    python tools/histogram_probe.py [--instances N] [--steps S] [--warmup W] [--legs plain,fold,constant:64,...] [--passes 2]
                                    [--agg auto] [--limit SECONDS] [--package-root DIR] [--out FILE]
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
LEGS = "plain,fold," + ",".join(f"{s}:{b}" for b in (64, 1024, 4096) for s in ("constant", "sine", "noise"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default=LEGS)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--agg", default="auto", choices=["auto", "0", "1"], help="the histogram kernel's shape (ACME_HIST_AGG)")
    ap.add_argument("--limit", type=int, default=120, help="seconds a leg may take")
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose package and library run (the parent's: plain, fold)")
    ap.add_argument("--out", default=None, help="append the raw lines to this file")
    args = ap.parse_args()
    if args.agg != "auto":
        os.environ["ACME_HIST_AGG"] = args.agg
    sys.path.insert(0, os.path.abspath(args.package_root))
    from acme_jl_amd.circuit import voltageprobe, voltagesource
    from acme_jl_amd.examples import build
    from acme_jl_amd.model import DiscreteModel
    from acme_jl_amd.runner import ModelRunner
    N, fs, T = args.instances, 44100, 44100

    def too_long(*_):
        raise SystemExit("a leg ran into its time limit: nothing more is started")
    signal.signal(signal.SIGALRM, too_long)

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")

    wire = build([("in", voltagesource(), {"-": "gnd"}), ("out", voltageprobe(), {"+": ("in", "+"), "-": "gnd"})])
    m = DiscreteModel(wire, Fraction(1, fs), "HomotopySolver{SimpleSolver}")
    results = []
    for p in range(args.passes):
        for leg in args.legs.split(","):
            signal.alarm(args.limit)
            sig, _, bins = leg.partition(":")
            r = ModelRunner(m, N, device=0)
            if sig == "constant":
                r.set_source(0, "const", offset=np.linspace(-0.9, 0.9, N))
            elif sig == "noise":
                r.set_source(0, "noise", amp=0.9, dist="uniform", seed=3)
            else:
                r.set_source(0, "sine", f_den=441, f_num=10, amp=0.9)
            r.set_measurement(length=T)
            line = dict(leg=leg, **{"pass": p}, instances=N, samples=T, agg=args.agg,
                        package=os.path.basename(os.path.abspath(args.package_root)))
            if sig == "fold":
                r.set_measurement_fold(441)
            elif bins:
                r.set_measurement_histogram(int(bins), -1.0, 1.0)

            def step():
                r.reset_measurement()
                r.source_clock = 0
                r.measure(T=T)
                r.measurement()                 # (the getter synchronises)
            for _ in range(args.warmup):
                step()
            times = []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                step()
                times.append(time.perf_counter() - t0)
            line.update(s_per_audio_s=float(np.median(times)) * fs / T, times=times, count=r.measurement().count)
            if bins:
                h = r.measurement_histogram()
                used = (h.counts[:, 0] > 0).sum(axis=-1)
                line.update(bins=h.bins, count=h.count, outside=int(h.under.sum() + h.over.sum() + h.nan.sum()),
                            counters_used_min=int(used.min()), counters_used_max=int(used.max()),
                            median_of_instance_0=float(h.percentile(50)[0, 0]))
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
