"""What a NOISE row costs (acme_batch_set_source_noise, csrc/acme_source.h), by the protocol of tools/source_probe.py: untimed
steps first, the median of the timed ones, the legs in alternation, each leg --repeat times (the spread between a leg's
repetitions is the yardstick for every comparison between legs).

Kernel legs: the source kernel alone on ONE row of --instances instances, one slice (4 096 samples) rendered to device
memory, milliseconds per slice from device events
  gauss1   a GAUSSIAN row                      unif1    a UNIFORM row
  hold1    a UNIFORM row with hold = 64        sine1    a SINE row with per-instance frequencies (source_probe's leg)
  table1   a TABLE row of 44 100 entries (source_probe's leg)
--tree DIR: the checkout whose package and library run; the parent commit's knows sine1 and table1 only.  To compare two
trees, give both the same legs, each in a process of its own, in alternation.

    python tools/noise_probe.py [--instances N] [--steps S] [--warmup W] [--repeat R] [--legs gauss1,unif1,...] [--tree DIR]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_LEGS = ("gauss1", "unif1", "hold1", "sine1", "table1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--legs", default="gauss1,unif1,hold1,sine1,table1")
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    from acme_jl_amd.model import DiscreteModel
    from acme_jl_amd.runner import ModelRunner
    N, fs = args.instances, 44100
    idx = np.arange(N)
    st = torch.cuda.current_stream().cuda_stream

    def kernel_leg(leg):
        from fractions import Fraction
        from acme_jl_amd import examples
        from acme_jl_amd.circuit import voltageprobe, voltagesource
        wire = DiscreteModel(examples.build([("in", voltagesource(), {"-": "gnd"}), ("out", voltageprobe(), {"+": ("in", "+"), "-": "gnd"})]),
                             Fraction(1, fs), "HomotopySolver{SimpleSolver}")
        r = ModelRunner(wire, N, device=0)
        amp = np.linspace(0.01, 1.0, N)
        if leg == "sine1":
            r.set_source(0, "sine", f_den=fs, f_num=20 + idx % 20000, amp=amp)
        elif leg == "table1":
            r.set_source(0, "table", table=np.sin(2 * np.pi * 1000.0 / fs * np.arange(fs)), amp=amp)
        else:
            r.set_source(0, "noise", amp=amp, dist="gaussian" if leg == "gauss1" else "uniform", hold=64 if leg == "hold1" else 1)
        TS = 4096
        ud = torch.empty((N, TS, 1), dtype=torch.float64, device="cuda")
        ms = []
        for k in range(args.warmup + args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r.lib.check(r.lib.L.acme_batch_render_sources(r.h, None, ud.data_ptr(), TS, 1, st))
            e1.record()
            torch.cuda.synchronize()
            if k >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        return dict(leg=leg, instances=N, samples=TS, kernel_ms_per_slice=float(np.median(ms)), ms_min=min(ms), ms_max=max(ms))

    for rep in range(args.repeat):
        for leg in args.legs.split(","):
            if leg not in KERNEL_LEGS:
                raise SystemExit(f"unknown leg {leg}")
            out = kernel_leg(leg)
            print(json.dumps(dict(out, repetition=rep, tree=os.path.abspath(args.tree))), flush=True)


if __name__ == "__main__":
    main()
