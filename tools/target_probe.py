"""The measurement target in use and under the clock: N candidates of the diode clipper -- one drive level each, a 1 kHz sine
source at 44.1 kHz generated on the device -- against the recorded output of the "real device" (one more instance, run on its
own with y stored), ESR per instance with neither u nor y stored; N = 8 192, T = 44 100, the one output row, K = 1, H = 0
(the moments unit of acme_meas_kernel alone walks the same y with four chains).  Seconds per second of audio for
  1   the measurement alone (runs on the parent commit too: --package-root);
  2   leg 1 with the target, every instance at lag 0 (uniform waves: the target tile broadcast);
  3   leg 1 with the target, a lag per instance (mixed waves: a gather per lane).
Steady state: `--warmup` untimed steps, then the median of `--steps` timed ones; every leg runs `--passes` times, in
alternation.  One process; every leg runs under its own time limit (SIGALRM) and the first failure ends the run.  Raw lines go
to --out.  The kernels' own times: one leg under `rocprofv3 --kernel-trace --stats` in a run of its own
(acme_meas_target_kernel beside acme_meas_kernel, per chunk of 4 096 samples).

    python tools/target_probe.py [--instances N] [--steps S] [--warmup W] [--legs 1,2,3] [--passes 2] [--limit SECONDS]
                                 [--package-root DIR] [--out FILE]
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

    m = DiscreteModel(examples.diodeclipper(), Fraction(1, fs), "HomotopySolver{CachingSolver{SimpleSolver}}")
    amp = np.logspace(-1, 0.7, N)
    best = N // 3
    signal.alarm(args.limit)
    rec = ModelRunner(m, 1, device=0)            # the recording: the device at the level of candidate `best`
    rec.set_source(0, "sine", f_den=441, f_num=10, amp=amp[best:best + 1])
    recording = rec.run_sources(T)[0, :, 0].copy()
    del rec
    signal.alarm(0)
    results = []
    for p in range(args.passes):
        for leg in args.legs.split(","):
            signal.alarm(args.limit)
            r = ModelRunner(m, N, device=0)
            r.set_source(0, "sine", f_den=441, f_num=10, amp=amp)
            r.set_measurement()
            line = dict(leg=leg, **{"pass": p}, instances=N, samples=T, package=os.path.basename(os.path.abspath(args.package_root)))
            if leg in ("2", "3"):
                r.set_measurement_target(recording, lag=None if leg == "2" else (441 * (np.arange(N) % 7)) % T, preemphasis=0.95)

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
            if leg in ("2", "3"):               # (lags of whole periods: the steady state lines up again, the start does not)
                mt = r.measurement_target()
                esr = mt.esr[:, 0]
                line.update(target_count=mt.count, esr_argmin=int(np.argmin(esr)), esr_min=float(esr.min()), esr_max=float(esr.max()),
                            esr_preemphasis_min=float(mt.esr_preemphasis[:, 0].min()), recorded=best,
                            gain_at_recorded=float(mt.gain[best, 0]), null_db_median=float(np.median(mt.null_db[:, 0])))
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
