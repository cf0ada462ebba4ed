"""The measurement events under the clock: N pairs of the pass-through model (a voltage source into a probe, y = u, one output
row) driven by a source generated on the device, so that the signal the events see is the one named -- N = 8 192, T = 44 100 per
step (eleven chunks of 4 096 samples, one after another), H = 0 (the moments unit of acme_meas_kernel alone walks the same y
with four chains).  A leg is
  plain            the measurement alone (runs on the parent commit too: --package-root);
  hist             the measurement with a histogram of 64 bins over (-1, 1) (acme_meas_hist_kernel on the same y, the yardstick;
                   runs on the parent commit too);
  SIGNAL:C:E       the measurement with events at C levels spread over (-0.6, 0.6), E slots: SIGNAL is `constant` (no event, every
                   lane on one side of every level), `sine` (1 kHz, amplitude 0.9: two events per level and period, 2 000 a
                   second) or `noise` (white, uniform in (-0.9, 0.9): events in every round, every slot filled at once).
Seconds per second of audio, steady state: `--warmup` untimed steps, then the median of `--steps` timed ones; every leg runs
`--passes` times, in alternation.  One process; every leg runs under its own time limit (SIGALRM) and the first failure ends the
run.  Raw lines go to --out.  The kernels' own times: ONE leg under `rocprofv3 --kernel-trace --stats` in a run of its own
(acme_meas_events_kernel beside acme_meas_kernel and, in the hist leg, acme_meas_hist_kernel, per chunk of 4 096 samples).

    python tools/events_probe.py [--instances N] [--steps S] [--warmup W] [--legs plain,hist,constant:1:8,...] [--passes 2]
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
LEGS = "plain,hist," + ",".join(f"{s}:{c}:{e}" for c, e in ((1, 8), (4, 8), (8, 16)) for s in ("constant", "sine", "noise"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default=LEGS)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120, help="seconds a leg may take")
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose package and library run (the parent's: plain, hist)")
    ap.add_argument("--out", default=None, help="append the raw lines to this file")
    args = ap.parse_args()
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
            sig, levels, slots = (leg.split(":") + ["", ""])[:3]
            r = ModelRunner(m, N, device=0)
            if sig == "constant":
                r.set_source(0, "const", offset=np.linspace(-0.9, 0.9, N))
            elif sig == "noise":
                r.set_source(0, "noise", amp=0.9, dist="uniform", seed=3)
            else:
                r.set_source(0, "sine", f_den=441, f_num=10, amp=0.9)
            r.set_measurement(length=T)
            line = dict(leg=leg, **{"pass": p}, instances=N, samples=T, package=os.path.basename(os.path.abspath(args.package_root)))
            if sig == "hist":
                r.set_measurement_histogram(64, -1.0, 1.0)
            elif levels:
                nC = int(levels)
                r.set_measurement_events(np.linspace(-0.6, 0.6, nC) if nC > 1 else 0.0, slots=int(slots))

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
            if levels:
                e = r.measurement_events()
                line.update(levels=e.levels, slots=e.slots, count=e.count, rises_min=int(e.rises.min()), rises_max=int(e.rises.max()),
                            falls_max=int(e.falls.max()), unknown=int(e.unknown.sum()),
                            frequency_of_instance_0=float(e.frequency(fs, 0)[0, 0]))
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
