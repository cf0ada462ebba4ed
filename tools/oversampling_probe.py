"""Oversampled runs at BASELINE config 5's shape: birdie_var_176k, 2 048 instances, one second of 44.1 kHz audio at k = 4,
vol held.  Model-rate instance-samples per second and device memory in use for
  (a) base-rate device arrays with set_oversampling(4),
  (b) today's way: pre-upsampled 176.4 kHz device arrays at k = 1,
  (c) both through host buffers (numpy arrays; nothing page-locked).
Device memory: what the device has in use after the run (the batch keeps its staging and scratch buffers until it goes)
less what it had in use before the batch and the arrays were made.

    python tools/oversampling_probe.py [--instances N] [--steps S]
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
    from acme_jl_amd.model import DiscreteModel
    from acme_jl_amd.runner import ModelRunner
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--factor", type=int, default=4)
    ap.add_argument("--legs", default="a,b,c/a,c/b", help="which of a, b, c/a, c/b to run")
    args = ap.parse_args()
    legs = args.legs.split(",")
    N, k, fs = args.instances, args.factor, 44100
    T = fs
    m = DiscreteModel.load(os.path.join(ROOT, "tests", "golden", "birdie_var_176k.json"))
    amp = np.logspace(-2, 0.5, N)
    vol = np.linspace(0.01, 1.0, N)

    def inputs(rate, samples):
        u = np.empty((N, samples, 2))
        u[:, :, 0] = amp[:, None] * np.sin(2 * np.pi * 1000.0 / rate * np.arange(samples))[None]
        u[:, :, 1] = vol[:, None]
        return u

    results = []
    for leg, factor, mem in (("a", k, "device"), ("b", 1, "device"), ("c/a", k, "host"), ("c/b", 1, "host")):
        if leg not in legs:
            continue
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = used_gb(torch)
        samples = T if factor > 1 else k * T
        u = inputs(fs * (k if factor == 1 else 1), samples)
        r = ModelRunner(m, N, device=0)
        if factor > 1:
            r.set_oversampling(factor, held_rows=[1])
        if mem == "device":
            ud = torch.from_numpy(u).cuda()
            yd = torch.empty((N, samples, m.ny), dtype=torch.float64, device="cuda")
            del u

            def step():
                r.run_device(ud.data_ptr(), yd.data_ptr(), samples, torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
        else:
            y = np.empty((N, samples, m.ny))

            def step():
                r.lib.check(r.lib.L.acme_batch_run(r.h, u.ctypes.data, y.ctypes.data, samples, 0, None))
        step()                                         # (warm-up: allocations, the first second of the signal)
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
        rate = N * k * T / t
        line = dict(leg=leg, factor=factor, memory=mem, base_samples=T, model_samples=k * T, s_per_step=t,
                    model_rate_inst_samples_per_s=rate, device_gb=mem_gb, os_slice=os.environ.get("ACME_OS_SLICE"),
                    run_kernel_ms_per_step=run_ms / args.steps, run_launches_per_step=launches / args.steps)
        print(json.dumps(line), flush=True)
        results.append(line)
        del r
        if mem == "device":
            del ud, yd
    by = {x["leg"]: x for x in results}
    if len(by) < 4:
        return
    print(json.dumps(dict(
        a_over_b_rate=by["a"]["model_rate_inst_samples_per_s"] / by["b"]["model_rate_inst_samples_per_s"],
        a_over_b_memory=by["a"]["device_gb"] / by["b"]["device_gb"],
        host_a_over_b_rate=by["c/a"]["model_rate_inst_samples_per_s"] / by["c/b"]["model_rate_inst_samples_per_s"])))


if __name__ == "__main__":
    main()
