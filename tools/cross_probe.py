"""The measurement cross-spectrum at the headline shape: the superover grid (bench.py's superover_grid), 8 192 instances, the
caching solver stack, a 1 kHz sine at 44.1 kHz, H = 10, the one output row, device arrays, y stored (leg (b) of
tools/measurement_probe.py).  Seconds per second of audio for
  1   nothing armed;
  2   acme_batch_set_measurement at one shared frequency;
  3   leg 2 with a cross-spectrum of the signal row, L = 1024, hop 512, Hann;
  4   leg 2 with a cross-spectrum, L = 4096, hop 2048, Hann;
  5   leg 2 with a cross-spectrum, L = 64, hop 32, Hann;
  6   leg 3 with a spectrum of the same geometry as well;
  7, 8, 9   leg 2 with a SPECTRUM alone at the geometries of legs 3, 4, 5 (tools/spectrum_probe.py's legs 3, 4, 5, for the
      comparison in one session).
Steady state as measurement_probe.py defines it: 4 untimed steps, then the median of 4 timed ones.  ONE PROCESS PER LEG: the
driver starts `timeout -k 10 LIMIT python tools/cross_probe.py --leg K ...` for each leg of each pass in turn and stops at the
first one that does not exit with 0 -- after a fault, an abort or a time limit nothing more is started on the device.  The
yardstick is the parent commit: --package-root names a checkout of it with its library built, and legs 1 and 2 run there
(--legs 1,2) as they do here.  Raw lines go to --out (profiles/cross_probe.jsonl).  The kernel's own time: one leg under
`rocprofv3 --kernel-trace --stats` (acme_meas_cross_kernel), in a run of its own (--leg 3 directly).

    python tools/cross_probe.py [--instances N] [--steps S] [--warmup W] [--legs 1,2,...,9] [--passes 1] [--limit SECONDS]
                                [--package-root DIR] [--out FILE]
    python tools/cross_probe.py --leg K [...]         one leg in this process
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CROSS = {"3": (1024, 512), "4": (4096, 2048), "5": (64, 32), "6": (1024, 512)}
SPEC = {"6": (1024, 512), "7": (1024, 512), "8": (4096, 2048), "9": (64, 32)}


def one_leg(args, leg):
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    from acme_jl_amd.model import CachingHomotopySolver, DiscreteModel
    from acme_jl_amd.runner import ModelRunner
    N, fs, H = args.instances, 44100, 10
    if N % 256:
        raise SystemExit("the superover grid needs a multiple of 256 instances")
    m = DiscreteModel.load(os.path.join(ROOT, "tests", "golden", "superover_var.json"), CachingHomotopySolver)
    idx = np.arange(N)           # (bench.py superover_grid: level fastest, then tone, then drive)
    pots = np.stack([(idx // 256) / float(N // 256), ((idx // 16) % 16) / 15.0, (idx % 16) / 15.0], axis=1)
    ud = torch.empty((N, fs, 4), dtype=torch.float64, device="cuda")
    ud[:, :, 0] = torch.from_numpy(np.sin(2 * np.pi * 1000.0 / fs * np.arange(fs))).cuda()[None]
    ud[:, :, 1:] = torch.from_numpy(pots).cuda()[:, None, :]
    yd = torch.empty((N, fs, m.ny), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    T = fs
    r = ModelRunner(m, N, device=0)
    line = dict(leg=leg, **{"pass": args.pass_number}, instances=N, samples=T, harmonics=H,
                package=os.path.basename(os.path.abspath(args.package_root)))
    if leg != "1":
        r.set_measurement(f0=(10, 441), harmonics=H)
    if leg in SPEC:
        r.set_measurement_spectrum(*SPEC[leg])
        line.update(spectrum_nfft=SPEC[leg][0], spectrum_hop=SPEC[leg][1])
    if leg in CROSS:
        L, hop = CROSS[leg]
        r.set_measurement_cross(0, L, hop)
        line.update(nfft=L, hop=hop, cross_gb=(2 * L + 4 * (L // 2 + 1)) * N * 8 / 1e9)

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
    if leg in CROSS:
        c = r.measurement_cross()
        k = round(1000 * CROSS[leg][0] / fs)
        line.update(segments=c.segments, cross_count=c.count, cross_finite=bool(np.isfinite(c.sxx).all() and np.isfinite(c.sxy).all()),
                    gain_1khz_median=float(np.median(np.abs(c.transfer()[:, 0, k]))),
                    coherence_1khz_median=float(np.median(c.coherence()[:, 0, k])))
    if leg in SPEC:
        sp = r.measurement_spectrum()
        line.update(spectrum_segments=sp.segments, spectrum_finite=bool(np.isfinite(sp.power).all()))
    if leg != "1":
        mm = r.measurement()
        line.update(count=mm.count, a1_median=float(np.median(np.abs(mm.harmonics[:, 0, 0]))))
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=4, help="untimed steps first (the first seconds of the signal cost more)")
    ap.add_argument("--legs", default="1,2,3,4,5,6,7,8,9")
    ap.add_argument("--leg", default=None, help="run this one leg in this process")
    ap.add_argument("--pass-number", type=int, default=0)
    ap.add_argument("--passes", type=int, default=1)
    ap.add_argument("--limit", type=int, default=150, help="seconds a leg's process may take")
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose package and library run (the parent's: legs 1,2)")
    ap.add_argument("--out", default=None, help="append the raw lines to this file")
    args = ap.parse_args()
    if args.leg is not None:
        return one_leg(args, args.leg)
    for p in range(args.passes):
        for leg in args.legs.split(","):
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--pass-number", str(args.pass_number + p),
                   "--instances", str(args.instances), "--steps", str(args.steps), "--warmup", str(args.warmup),
                   "--package-root", args.package_root] + (["--out", args.out] if args.out else [])
            rc = subprocess.call(cmd)
            if rc != 0:
                raise SystemExit(f"leg {leg} ended with status {rc}: nothing more is started")


if __name__ == "__main__":
    main()
