"""The measurement weighting under the clock: N instances of the diode clipper -- one drive level each, a 1 kHz sine source at
44.1 kHz generated on the device --, measured with neither u nor y stored; N = 8 192, T = 44 100, the one output row, H = 0
(the moments unit of acme_meas_kernel alone).  Seconds per second of audio for
  1   the measurement alone (runs on the parent commit too: --package-root);
  2   leg 1 behind the K weighting of BS.1770 (S = 2);
  3   leg 1 behind eight sections (S = 8: the A weighting's three, the K filter's two, a DC blocker and two random stable ones).
Steady state: `--warmup` untimed steps, then the median of `--steps` timed ones; every leg runs `--passes` times, in
alternation.  One process; every leg runs under its own time limit (SIGALRM) and the first failure ends the run.  Raw lines go
to --out.  The kernels' own times: one leg under `rocprofv3 --kernel-trace --stats` in a run of its own
(acme_meas_weight_kernel per slice of 4 096 samples beside acme_meas_kernel per chunk of as many; --target adds the
measurement target to every leg, so that acme_meas_target_kernel is timed on the same y in the same trace).

    python tools/weighting_probe.py [--instances N] [--steps S] [--warmup W] [--legs 1,2,3] [--passes 2] [--limit SECONDS]
                                    [--target] [--package-root DIR] [--out FILE]
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
    ap.add_argument("--legs", default="1,2,3")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120, help="seconds a leg may take")
    ap.add_argument("--target", action="store_true", help="every leg also carries a measurement target (its kernel in the trace)")
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose package and library run (the parent's: leg 1)")
    ap.add_argument("--out", default=None, help="append the raw lines to this file")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    from acme_jl_amd import examples
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

    def cascade(leg):
        from acme_jl_amd.runner import weighting_sos
        if leg == "2":
            return weighting_sos("K", fs)
        rng = np.random.default_rng(8)
        rnd = [[1.0, 0.3, 0.1, -2 * r * np.cos(t), r * r] for r, t in zip(rng.uniform(0.3, 0.9, 2), rng.uniform(0.2, 2.8, 2))]
        return np.concatenate([weighting_sos("A", fs), weighting_sos("K", fs), weighting_sos("dc", fs), np.array(rnd)])

    m = DiscreteModel(examples.diodeclipper(), Fraction(1, fs), "HomotopySolver{CachingSolver{SimpleSolver}}")
    amp = np.logspace(-1, 0.7, N)
    recording = np.sin(2 * np.pi * 1000.0 * np.arange(T) / fs)
    results = []
    for p in range(args.passes):
        for leg in args.legs.split(","):
            signal.alarm(args.limit)
            r = ModelRunner(m, N, device=0)
            r.set_source(0, "sine", f_den=441, f_num=10, amp=amp)
            r.set_measurement()
            line = dict(leg=leg, **{"pass": p}, instances=N, samples=T, target=args.target,
                        package=os.path.basename(os.path.abspath(args.package_root)))
            if args.target:
                r.set_measurement_target(recording, preemphasis=0.95)
            if leg in ("2", "3"):
                sos = cascade(leg)
                r.set_measurement_weighting(sos)
                line.update(sections=len(sos))

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
            ms = r.measurement()
            line.update(s_per_audio_s=float(np.median(times)) * fs / T, times=times, run_kernel_ms_per_step=run_ms / args.steps,
                        run_launches_per_step=launches / args.steps, count=ms.count, rms_median=float(np.median(ms.rms)),
                        loudness_median=float(np.median(ms.loudness())) if hasattr(ms, "loudness") else None)
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
