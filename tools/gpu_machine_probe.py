"""Builds and relaxations per second of jss_bottleneck_build and jss_machine_relax (include/jss_machine.h) on the device, and for
context the one-thread host twin's time for a share of the same work, scaled to the whole -- a figure to read the device's number
by, not a baseline it replaced, so the two stand next to each other and no ratio is asked of them.
usage: python tools/gpu_machine_probe.py [--out FILE.txt] [--windows N] [--cases ta01,ta41] [--builds 4096] [--relaxations 65536]
                                         [--limit SECONDS]

Every step -- one instance -- runs in a child process of its own under a time limit of its own; the first step that fails, is
killed or runs out of time ends the probe, and nothing more is started on the device.  A step: ONE env of the instance; `builds`
candidates on env 0 with seeded integer biases in [0, 50] (candidate 0 unbiased) at reopt 0 and 1, then `relaxations` candidates
of the empty selection with every output that has one row per candidate or per machine; two warm-up calls, then --windows calls,
HIP events around one call; reported are the median and the spread (min .. max) of a call and, from the median, calls' candidates
per second.  The twin (CpuBackend(threads=1)) runs the first `--twin` candidates once, wall clock, scaled to the whole."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step(name, builds, relaxations, windows, twin_share):
    import torch
    from jssenv_amd import BatchedJssEnv
    from jssenv_amd.env import CpuBackend, HipBackend

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
    host = BatchedJssEnv(name, batch=1, _backend=CpuBackend(threads=1), seed=7)
    host.reset()
    J, M = env.jmax, env.mmax
    bias_host = np.random.default_rng(7).integers(0, 51, (builds, M)).astype(np.int32)
    bias_host[0] = 0
    bias = torch.from_numpy(bias_host).to(be.device)
    parents = torch.zeros(builds, dtype=torch.int32, device=be.device)
    lines = [f"case {name}: {J} x {M}, candidates of one env"]
    for reopt in (0, 1):
        for _ in range(2):
            mk, _, info = env.bottleneck(parents, bias, reopt)
        torch.cuda.synchronize()
        times = [timed_us(lambda: env.bottleneck(parents, bias, reopt)) for _ in range(windows)]
        assert (mk > 0).all()
        us = float(np.median(times))
        share = min(twin_share, builds)
        t0 = time.perf_counter()
        twin_mk = host.bottleneck(np.zeros(share, np.int32), bias_host[:share], reopt)[0]
        twin_us = (time.perf_counter() - t0) * 1e6 * builds / share
        assert np.array_equal(twin_mk, mk[:share].cpu().numpy())
        lines.append(f"  bottleneck reopt {reopt} x {builds:6d} {us:12.1f} us ({min(times):.1f} .. {max(times):.1f})   {builds / us * 1e6:12.0f} builds/s   "
                     f"makespan unbiased {int(mk[0])}, best {int(mk.min())}, mean {mk.float().mean().item():.1f}; re-sequencings per build "
                     f"{info[:, 1].float().mean().item():.0f}   [one-thread twin, {share} builds scaled: {twin_us:.0f} us]")
    parents = torch.zeros(relaxations, dtype=torch.int32, device=be.device)
    for _ in range(2):
        out = env.relax_machines(None, 0, parents, jps=True, schrage=True)
    torch.cuda.synchronize()
    times = [timed_us(lambda: env.relax_machines(None, 0, parents, jps=True, schrage=True)) for _ in range(windows)]
    us = float(np.median(times))
    share = min(twin_share * 8, relaxations)
    t0 = time.perf_counter()
    twin_out = host.relax_machines(None, 0, np.zeros(share, np.int32), jps=True, schrage=True)
    twin_us = (time.perf_counter() - t0) * 1e6 * relaxations / share
    assert np.array_equal(twin_out[0], out[0][:share].cpu().numpy()) and np.array_equal(twin_out[3], out[3][:share].cpu().numpy())
    lines.append(f"  relax_machines    x {relaxations:6d} {us:12.1f} us ({min(times):.1f} .. {max(times):.1f})   {relaxations / us * 1e6:12.0f} relaxations/s   "
                 f"lower bound {int(out[0][0])}, length {int(out[1][0])}, bottleneck {int(out[2][0])}   [one-thread twin, {share} scaled: {twin_us:.0f} us]")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--cases", default="ta01,ta41")
    ap.add_argument("--builds", type=int, default=4096)
    ap.add_argument("--relaxations", type=int, default=65536)
    ap.add_argument("--twin", type=int, default=64, help="builds the one-thread twin runs (8 times as many relaxations)")
    ap.add_argument("--limit", type=int, default=150, help="seconds per step")
    ap.add_argument("--step", default=None, help="(internal) case: run that step in this process")
    args = ap.parse_args()
    if args.step:
        print("\n".join(step(args.step, args.builds, args.relaxations, args.windows, args.twin)), flush=True)
        return 0
    import torch
    lines = [f"# device {torch.cuda.get_device_name(0)}; HIP events around one call, median (min .. max) of {args.windows} calls; seeded biases in "
             f"[0, 50]; every step a process of its own under a limit of {args.limit} s"]
    print(lines[0], flush=True)
    status = 0
    for name in args.cases.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--windows", str(args.windows), "--builds", str(args.builds),
               "--relaxations", str(args.relaxations), "--twin", str(args.twin)]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            lines.append(f"case {name}: no answer within {args.limit} s; nothing more is started")
            status = 124
        else:
            if out.returncode:
                lines.append(f"case {name}: exit status {out.returncode}; nothing more is started\n{out.stderr[-2000:]}")
                status = out.returncode
            else:
                lines.append(out.stdout.rstrip())
        print(lines[-1], flush=True)
        if status:
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
