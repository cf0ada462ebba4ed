"""What a source run costs, at the headline shape: the superover grid (drive x tone x level, bench.py's superover_grid),
8 192 instances, the caching solver stack, one second at 44.1 kHz per step, H = 8 harmonics of f0 = 10/441 fs measured,
y = NULL.  Milliseconds per second of audio (median over the steps) for
  yard    run_const on a device-resident u_var (the signal row; the three pots constant): the sliced pipeline with the
          expand kernel where the source kernel sits -- the yardstick; runs on any checkout (--tree: the parent commit's)
  src     the same grid as a source run from device memory: a SINE source on the signal row, three CONST rows
  host    the source run as a one-shot host-memory call (there is no u to copy)
  sine1   the source kernel alone: one slice (4 096 samples) of ONE row, a SINE with per-instance frequencies, rendered
          to device memory; milliseconds per slice from device events
  table1  the same for a TABLE row of 44 100 entries
  pulse1  the same for a PULSE row: per-instance periods (100 ... 20 099 samples), edges (rise and fall a tenth of the period
          each) and widths
  burst1  the same for a BURST row: pulse1's envelopes on sine1's tones
The source and expand kernels' own times per slice inside a run: `rocprofv3 --kernel-trace --stats -- python
tools/source_probe.py --legs src` (acme_source_kernel) and `--legs yard` (acme_expand_kernel), in runs of their own.

    python tools/source_probe.py [--instances N] [--steps S] [--warmup W] [--legs yard,src,host,sine1,table1,pulse1,burst1] [--tree DIR]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5, help="untimed seconds first (the first seconds of the signal cost more)")
    ap.add_argument("--legs", default="yard,src,host,sine1,table1")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package and library run (the yardstick: the parent commit's)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    from acme_jl_amd.model import CachingHomotopySolver, DiscreteModel
    from acme_jl_amd.runner import ModelRunner
    legs = args.legs.split(",")
    N, fs = args.instances, 44100
    T = fs
    if N % 256:
        raise SystemExit("the superover grid needs a multiple of 256 instances")
    m = DiscreteModel.load(os.path.join(ROOT, "tests", "golden", "superover_var.json"), CachingHomotopySolver)
    idx = np.arange(N)           # (bench.py superover_grid: level fastest, then tone, then drive)
    pots = np.stack([(idx // 256) / float(N // 256), ((idx // 16) % 16) / 15.0, (idx % 16) / 15.0], axis=1)
    spec = dict(f0=(10, 441), harmonics=8)
    st = torch.cuda.current_stream().cuda_stream

    for leg in legs:
        if leg in ("sine1", "table1", "pulse1", "burst1"):
            from fractions import Fraction
            from acme_jl_amd import examples
            from acme_jl_amd.circuit import voltageprobe, voltagesource
            wire = DiscreteModel(examples.build([("in", voltagesource(), {"-": "gnd"}), ("out", voltageprobe(), {"+": ("in", "+"), "-": "gnd"})]),
                                 Fraction(1, fs), "HomotopySolver{SimpleSolver}")
            r = ModelRunner(wire, N, device=0)
            if leg == "sine1":
                r.set_source(0, "sine", f_den=fs, f_num=20 + idx % 20000, amp=np.linspace(0.01, 1.0, N))
            elif leg == "table1":
                r.set_source(0, "table", table=np.sin(2 * np.pi * 1000.0 / fs * np.arange(fs)), amp=np.linspace(0.01, 1.0, N))
            else:
                period = 100 + idx % 20000
                env = dict(period=period, delay=idx % 97, rise=period // 10, on=period // 2, fall=period // 10, amp=np.linspace(0.01, 1.0, N))
                if leg == "pulse1":
                    r.set_source(0, "pulse", **env)
                else:
                    r.set_source(0, "burst", f_den=fs, f_num=20 + idx % 20000, **env)
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
            print(json.dumps(dict(leg=leg, instances=N, samples=TS, kernel_ms_per_slice=float(np.median(ms)), gb_written=N * TS * 8 / 1e9)), flush=True)
            del r, ud
            continue
        r = ModelRunner(m, N, device=0)
        r.set_measurement(**spec)
        if leg == "yard":
            sig = np.sin(2 * np.pi * 1000.0 / fs * np.arange(T))
            uv = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(sig[None, :, None], (N, T, 1)))).cuda()
            ucn = np.zeros((N, 4))
            ucn[:, 1:] = pots
            uc = torch.from_numpy(ucn).cuda()

            def step():
                r.lib.check(r.lib.L.acme_batch_run_const(r.h, uv.data_ptr(), uc.data_ptr(), 0b1110, None, T, 1, st))
                torch.cuda.synchronize()
        else:
            r.set_source(0, "sine", f_den=441, f_num=10)
            for c in range(3):
                r.set_source(1 + c, "const", offset=pots[:, c])
            mem = 1 if leg == "src" else 0

            def step():
                r.lib.check(r.lib.L.acme_batch_run_sources(r.h, None, None, T, mem, st if mem else None))
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
        mm = r.measurement()
        print(json.dumps(dict(leg=leg, tree=os.path.abspath(args.tree), instances=N, samples=T, ms_per_audio_s=1e3 * float(np.median(times)),
                              ms_min=1e3 * min(times), ms_max=1e3 * max(times), run_kernel_ms_per_step=run_ms / args.steps,
                              run_launches_per_step=launches / args.steps, thd_median=float(np.median(mm.thd())), count=mm.count)), flush=True)
        del r


if __name__ == "__main__":
    main()
