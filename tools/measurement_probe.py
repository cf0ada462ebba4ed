"""Output measurements at the headline shape: the superover grid (drive x tone x level, bench.py's superover_grid), 8 192
instances, the caching solver stack, one second of a 1 kHz sine at 44.1 kHz per step, H = 10 harmonics of f0 = 10/441 fs, the one output row.  Seconds per
second of audio and device memory in use for
  (a) device arrays, y stored;
  (b) (a) with the measurement armed;
  (c) device arrays, y = NULL, the measurement armed;
  (d) run_const from host arrays (pageable numpy; the three pots constant) with y;
  (e) (d) with y = NULL and the measurement armed.
Device memory: what the device has in use after the run (the batch keeps its staging and scratch buffers until it goes)
less what it had in use before the batch and the arrays were made.  The measurement kernels' own time: run this under
`rocprofv3 --kernel-trace --stats` (acme_meas_kernel, acme_meas_tw_kernel), in a run of its own.

    python tools/measurement_probe.py [--instances N] [--steps S] [--warmup W] [--legs a,b,c,d,e]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def used_gb(torch):
    free, total = torch.cuda.mem_get_info(0)
    return (total - free) / 1e9


def main():
    import torch
    from acme_jl_amd.model import CachingHomotopySolver, DiscreteModel
    from acme_jl_amd.runner import ModelRunner
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3, help="untimed seconds first (the first seconds of the signal cost more)")
    ap.add_argument("--legs", default="a,b,c,d,e", help="which of a ... e to run")
    args = ap.parse_args()
    legs = args.legs.split(",")
    N, fs = args.instances, 44100
    T = fs
    if N % 256:
        raise SystemExit("the superover grid needs a multiple of 256 instances")
    # (the bench's solver stack: HomotopySolver{CachingSolver{SimpleSolver}})
    m = DiscreteModel.load(os.path.join(ROOT, "tests", "golden", "superover_var.json"), CachingHomotopySolver)
    idx = np.arange(N)           # (bench.py superover_grid: level fastest, then tone, then drive)
    pots = np.stack([(idx // 256) / float(N // 256), ((idx // 16) % 16) / 15.0, (idx % 16) / 15.0], axis=1)
    sig = np.sin(2 * np.pi * 1000.0 / fs * np.arange(T))
    spec = dict(f0=(10, 441), harmonics=10)

    results = []
    for leg in ("a", "b", "c", "d", "e"):
        if leg not in legs:
            continue
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = used_gb(torch)
        r = ModelRunner(m, N, device=0)
        if leg in ("b", "c", "e"):
            r.set_measurement(**spec)
        if leg in ("a", "b", "c"):
            u = np.empty((N, T, 4))
            u[:, :, 0] = sig[None]
            u[:, :, 1:] = pots[:, None, :]
            ud = torch.from_numpy(u).cuda()
            del u
            yd = torch.empty((N, T, m.ny), dtype=torch.float64, device="cuda") if leg != "c" else None

            def step():
                r.run_device(ud.data_ptr(), yd.data_ptr() if yd is not None else 0, T, torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
        else:
            uv = np.ascontiguousarray(np.broadcast_to(sig[None, :, None], (N, T, 1)))
            uc = np.zeros((N, 4))
            uc[:, 1:] = pots
            y = np.empty((N, T, m.ny)) if leg == "d" else None

            def step():
                if y is None:
                    r.measure_const(uv, uc, [1, 2, 3], check=False)
                else:
                    r.run_const(uv, uc, [1, 2, 3], y=y, check=False)
        for _ in range(args.warmup):                   # (allocations, the first seconds of the signal)
            step()
        r.kernel_time(reset=True)
        times = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            step()
            times.append(time.perf_counter() - t0)
        r.check()
        mem_gb = used_gb(torch) - base
        run_ms, launches = r.kernel_time()
        t = float(np.median(times))
        line = dict(leg=leg, instances=N, samples=T, s_per_audio_s=t * fs / T, times=times, device_gb=mem_gb,
                    run_kernel_ms_per_step=run_ms / args.steps, run_launches_per_step=launches / args.steps)
        if leg in ("b", "c", "e"):
            mm = r.measurement()
            line["thd_median"] = float(np.median(mm.thd()))
            line["count"] = mm.count
        print(json.dumps(line), flush=True)
        results.append(line)
        del r
        if leg in ("a", "b", "c"):
            del ud, yd
    by = {x["leg"]: x for x in results}
    ratios = {}
    if "a" in by and "b" in by:
        ratios["b_over_a"] = by["b"]["s_per_audio_s"] / by["a"]["s_per_audio_s"]
    if "a" in by and "c" in by:
        ratios["c_over_a"] = by["c"]["s_per_audio_s"] / by["a"]["s_per_audio_s"]
    if "d" in by and "e" in by:
        ratios["e_over_d"] = by["e"]["s_per_audio_s"] / by["d"]["s_per_audio_s"]
    if ratios:
        print(json.dumps(ratios))


if __name__ == "__main__":
    main()
