"""A two-tone intermodulation sweep at the headline shape: the superover grid (bench.py's superover_grid), 8 192 instances,
the caching solver stack, one second at 44.1 kHz per step, one output row measured, sources on every input row, y = NULL.
Seconds per second of audio for
  Y   the PARENT commit (--parent-tree: a checkout of it with its library built): a SINE source at 1 kHz plus
      acme_batch_set_measurement_per_instance, H = 10, every f_num equal;
  1   this tree, the same calls as Y;
  2   a MULTISINE source 19 kHz + 20 kHz at f_den = 44 100 with per-instance level, plus 10 bins
      (acme_batch_set_measurement_bins), one tone pair (F = 1);
  3   as leg 2 with 32 distinct tone pairs (the pair's centre swept, the fastest axis).
Steady state as tools/measurement_probe.py defines it: 4 untimed seconds, then the median of 4 timed ones; every leg runs
twice, in alternation (pass 0 of every leg, then pass 1).  Every leg-pass is a child process of its own (leg Y imports
another package and loads another library) under its own time limit; one runs at a time, and the first failure ends the run.
--check N: one more child that stores y for N instances of leg 2 and compares the bins with a numpy DFT of the stored y.
The source kernel's own time: run `--child 2` under `rocprofv3 --kernel-trace --stats` in a run of its own.

    python tools/imd_probe.py [--parent-tree DIR] [--legs Y,1,2,3] [--passes 2] [--limit SECONDS] [--out profiles/imd_probe.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, H = 44100, 10
# both fundamentals, then the products: f2 - f1, 2 f1 - f2, 2 f2 - f1 (CCIF / DFD), f1 + f2, 3 f1 - 2 f2, 3 f2 - 2 f1, 2 f1, 2 f2
COEF = [[1, 0], [0, 1], [-1, 1], [2, -1], [-1, 2], [1, 1], [3, -2], [-2, 3], [2, 0], [0, 2]]


def grid(N):
    idx = np.arange(N)           # (bench.py superover_grid: level fastest, then tone, then drive)
    pots = np.stack([(idx // 256) / float(N // 256), ((idx // 16) % 16) / 15.0, (idx % 16) / 15.0], axis=1)
    level = 0.5 * 10.0 ** (-2.0 + 2.0 * ((idx * 2654435761) % N) / (N - 1.0))      # 40 dB, spread over the cells
    return pots, level


def pairs(leg, N):
    """f_num [2, N]: 19 kHz + 20 kHz, or 32 pairs 1 kHz apart with the centre between 4.5 and 20 kHz"""
    if leg != "3":
        return np.stack([np.full(N, 19000, dtype=np.int64), np.full(N, 20000, dtype=np.int64)])
    f1 = (4000 + 500 * (np.arange(N) % 32)).astype(np.int64)
    return np.stack([f1, f1 + 1000])


def arm(r, leg, N, lo=0, hi=None):
    hi = N if hi is None else hi
    pots, level = grid(N)
    if leg in ("Y", "1"):
        r.set_source(0, "sine", f_den=FS, f_num=1000, amp=level[lo:hi])
    else:
        r.set_source(0, "multisine", f_den=FS, f_num=pairs(leg, N)[:, lo:hi], amp=np.stack([level[lo:hi]] * 2))
    for c in range(3):
        r.set_source(1 + c, "const", offset=pots[lo:hi, c])
    if leg in ("Y", "1"):
        r.set_measurement(f_den=FS, f_num=np.full(hi - lo, 1000, dtype=np.int64), harmonics=H)
    else:
        r.set_measurement_bins(COEF, tones_from_source=0)
    return r


def child(args):
    import torch
    from acme_jl_amd.model import CachingHomotopySolver, DiscreteModel
    from acme_jl_amd.runner import ModelRunner
    leg, N, T = args.child, args.instances, FS
    m = DiscreteModel.load(os.path.join(ROOT, "tests", "golden", "superover_var.json"), CachingHomotopySolver)
    st = torch.cuda.current_stream().cuda_stream
    if args.check:
        n = args.check
        lo = N - n                   # (the cells with the highest drive)
        r = arm(ModelRunner(m, n, device=0), "2", N, lo, N)
        y = r.run_sources(T)
        A = r.measurement().bins[:, 0, :]
        kb = [(c[0] * 19000 + c[1] * 20000) % FS for c in COEF]
        dft = 2.0 / T * np.fft.fft(y[:, :, 0], axis=1)[:, kb]
        imd_lib = r.measurement().imd([0, 1], [2, 3, 4])[:, 0]
        a = np.abs(dft)
        imd_np = np.sqrt((a[:, 2:5] ** 2).sum(1) / (a[:, :2] ** 2).sum(1))
        print(json.dumps(dict(check=n, max_abs_bin_difference=float(np.abs(A - dft).max()), imd_library=imd_lib.tolist(), imd_numpy_dft=imd_np.tolist())), flush=True)
        return
    r = arm(ModelRunner(m, N, device=0), leg, N)
    line = dict(leg=leg, **{"pass": args.pass_no}, instances=N, samples=T, bins=H, library=r.lib.path)
    plan = r.measurement_plan()
    line.update(groups=plan["groups"], chunk=plan["chunk"], uniform_waves=int((plan["wave_group"] >= 0).sum()), mixed_waves=int((plan["wave_group"] < 0).sum()))

    def step():
        r.lib.check(r.lib.L.acme_batch_run_sources(r.h, None, None, T, 1, st))
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
    line.update(s_per_audio_s=float(np.median(times)), times=times, run_kernel_ms_per_step=run_ms / args.steps, count=mm.count)
    if leg in ("2", "3"):
        line.update(imd_median=float(np.median(mm.imd([0, 1], [2, 3, 4]))), a_f1_median=float(np.median(np.abs(mm.bins[:, 0, 0]))))
    else:
        line.update(thd_median=float(np.median(mm.thd())), a1_median=float(np.median(np.abs(mm.harmonics[:, 0, 0]))))
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=4, help="untimed seconds first (the first seconds of the signal cost more)")
    ap.add_argument("--legs", default="Y,1,2,3")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--limit", type=int, default=150, help="seconds a leg-pass may take")
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built (leg Y)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imd_probe.jsonl"))
    ap.add_argument("--check", type=int, default=0, help="instances of the stored-y check against a numpy DFT (0: none)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--pass-no", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.instances % 256:
        raise SystemExit("the superover grid needs a multiple of 256 instances")
    if args.child:
        sys.path.insert(0, os.environ.get("IMD_PROBE_TREE", ROOT))
        return child(args)
    legs = args.legs.split(",")
    if "Y" in legs and not args.parent_tree:
        raise SystemExit("leg Y needs --parent-tree")
    jobs = [(leg, p, 0) for p in range(args.passes) for leg in legs] + ([("2", 0, args.check)] if args.check else [])
    lines = []
    for leg, p, chk in jobs:
        env = dict(os.environ)
        if leg == "Y":
            tree = os.path.abspath(args.parent_tree)
            env.update(IMD_PROBE_TREE=tree, ACME_HIP_LIB=os.path.join(tree, "acme_jl_amd", "csrc", "libacme_hip.so"))
        cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--pass-no", str(p), "--instances", str(args.instances),
               "--steps", str(args.steps), "--warmup", str(args.warmup), "--check", str(chk)]
        try:
            out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"leg {leg} pass {p} ran into its time limit: nothing more is started")
        if out.returncode != 0:
            sys.stderr.write(out.stdout + out.stderr)
            raise SystemExit(f"leg {leg} pass {p} failed (exit status {out.returncode}): nothing more is started")
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        lines.append(line)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    best = {}
    for x in map(json.loads, lines):
        if "leg" in x:
            best[x["leg"]] = min(best.get(x["leg"], np.inf), x["s_per_audio_s"])
    if "Y" in best:
        print(json.dumps({f"{k}_over_Y": v / best["Y"] for k, v in best.items() if k != "Y"}))


if __name__ == "__main__":
    main()
