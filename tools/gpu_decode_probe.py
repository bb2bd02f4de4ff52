"""Decodes per second of jss_decode_keys (include/jss_decode.h) on the device, and for context the env's own decoder,
rollout("keys"), on a batch of the same size -- another decoder (non-delay-like dynamics with NOPE, stepping live envs), so the two
figures stand next to each other and no ratio is asked of them.
usage: python tools/gpu_decode_probe.py [--out FILE.txt] [--windows N] [--cases ta01,ta41] [--sizes 4096,65536] [--limit SECONDS]

Every step -- one instance at one size -- runs in a child process of its own under a time limit of its own; the first step that
fails, is killed or runs out of time ends the probe, and nothing more is started on the device.  A step: ONE env of the instance,
`size` random key tables (int32, drawn on the device), candidate c on env 0; two warm-up calls, then --windows calls at each
delta 0, 0.5 and 1, HIP events around one call; reported are the median and the spread (min .. max) of a call and, from the
median, decodes per second.  Then a batch of `size` envs, reset and decoded by one rollout("keys") with the same tables, timed
the same way (the reset is outside the events)."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DELTAS = (0.0, 0.5, 1.0)


def step(name, size, windows):
    import torch
    from jssenv_amd import BatchedJssEnv
    from jssenv_amd.env import HipBackend

    def timed_us(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1000.0

    be = HipBackend("cuda:0")
    env = BatchedJssEnv(name, batch=1, _backend=be, seed=7)
    env.reset()
    J, M = env.jmax, env.mmax
    keys, _ = env.evolve_keys((size, J, M), None, 1, 0, 1, seed=7)
    parents = torch.zeros(size, dtype=torch.int32, device=be.device)
    lines = [f"case {name}: {J} x {M}, {size} candidates of one env"]
    for delta in DELTAS:
        for _ in range(2):
            mk = env.decode_keys(keys, parents, delta)
        torch.cuda.synchronize()
        times = [timed_us(lambda: env.decode_keys(keys, parents, delta)) for _ in range(windows)]
        mk, info = env.decode_keys(keys, parents, delta, info=True)
        torch.cuda.synchronize()
        assert (mk > 0).all()
        us = float(np.median(times))
        lines.append(f"  decode_keys delta {delta:3.1f} {us:12.1f} us ({min(times):.1f} .. {max(times):.1f})   {size / us * 1e6:14.0f} decodes/s   "
                     f"mean makespan {mk.float().mean().item():.1f}, operations delayed per decode {info[:, 2].float().mean().item():.1f}")
    batch = BatchedJssEnv(name, batch=size, _backend=be, seed=7)
    n_iter = 3 * J * M
    times = []
    for w in range(2 + windows):
        batch.reset()
        torch.cuda.synchronize()
        t = timed_us(lambda: batch.rollout("keys", n_iter=n_iter, autoreset=False, keys=keys))
        if w >= 2:
            times.append(t)
    assert bool(batch.done.all())
    us = float(np.median(times))
    lines.append(f"  rollout(\"keys\")      {us:12.1f} us ({min(times):.1f} .. {max(times):.1f})   {size / us * 1e6:14.0f} episodes/s   "
                 f"mean makespan {batch.makespan.float().mean().item():.1f}   (the env's own decoder, for context)")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--cases", default="ta01,ta41")
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--limit", type=int, default=120, help="seconds per step")
    ap.add_argument("--step", default=None, help="(internal) case,size: run that step in this process")
    args = ap.parse_args()
    if args.step:
        name, size = args.step.split(",")
        print("\n".join(step(name, int(size), args.windows)), flush=True)
        return 0
    import torch
    lines = [f"# device {torch.cuda.get_device_name(0)}; HIP events around one call, median (min .. max) of {args.windows} calls; random int32 "
             f"key tables; every step a process of its own under a limit of {args.limit} s"]
    print(lines[0], flush=True)
    status = 0
    for name in args.cases.split(","):
        for size in args.sizes.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", f"{name},{size}", "--windows", str(args.windows)]
            try:
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                lines.append(f"case {name}, {size}: no answer within {args.limit} s; nothing more is started")
                status = 124
                break
            if out.returncode:
                lines.append(f"case {name}, {size}: exit status {out.returncode}; nothing more is started\n{out.stderr[-2000:]}")
                status = out.returncode
                break
            lines.append(out.stdout.rstrip())
            print(lines[-1], flush=True)
        if status:
            print(lines[-1], flush=True)
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
