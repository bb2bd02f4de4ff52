"""Propagations per second of jss_propagate (include/jss_propagate.h) on the device, and what search.destructive_bound reaches
with them: one launch of 64 trial makespans of ta01, one shaving round of ta01 and one of ta41 at the scan's bound, and a whole
destructive_bound("ta01", upper=1231, rounds=8).  For context the host-core twin on one thread for the same candidates, timed on a
subset and scaled.  No ratio is asked of anything.
usage: python tools/gpu_propagate_probe.py [--out FILE.txt] [--windows N] [--twin N] [--limit SECONDS]

Every step runs in a child process of its own under a time limit of its own; the first step that fails, is killed or runs out of
time ends the probe, and nothing more is started on the device.  A launch is timed by HIP events around one call: two warm-up
calls, then --windows calls; reported are the median and the spread (min .. max).  The statuses of the first `--twin` candidates of
every launch are compared with the one-thread twin's, whose time for them is scaled to the launch's candidates."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("scan:ta01", "round:ta01", "round:ta41", "bound:ta01")


def step(what, windows, twin_share):
    import torch
    from jssenv_amd import BatchedJssEnv, search
    from jssenv_amd.env import CpuBackend, HipBackend
    kind, name = what.split(":")

    def timed_us(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1000.0

    def measure(fn):
        for _ in range(2):
            out = fn()
        torch.cuda.synchronize()
        times = [timed_us(fn) for _ in range(windows)]
        return out, float(np.median(times)), f"({min(times):.1f} .. {max(times):.1f})"

    be = HipBackend("cuda:0")
    if kind == "bound":
        search.destructive_bound(name, upper=1231, rounds=8, _backend=be)          # (warm-up: the libraries, the allocator)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = search.destructive_bound(name, upper=1231, rounds=8, _backend=be)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        return [f"case {name}: destructive_bound(upper=1231, rounds=8)   {wall * 1e3:10.1f} ms wall   one machine {int(res.one_machine[0])}, "
                f"scan {int(res.first_bound[0])}, bound {int(res.lower_bound[0])}, launches {int(res.launches[0])}, propagations "
                f"{int(res.propagations[0])}, proved optimal {bool(res.proved_optimal[0])}"]
    env = BatchedJssEnv(name, batch=1, _backend=be, seed=7)
    env.reset()
    host = BatchedJssEnv(name, batch=1, _backend=CpuBackend(threads=1), seed=7)
    host.reset()
    start = int(env.solve_machines()[0][0])

    def twin_check(status, ubs, est=None, lct=None, hyp=None):
        share = min(twin_share, len(ubs))
        t0 = time.perf_counter()
        ref = host.propagate(ubs[:share], parents=np.zeros(share, np.int32), est=est, lct=lct, hyp=None if hyp is None else tuple(x[:share] for x in hyp))
        seconds = time.perf_counter() - t0
        assert np.array_equal(ref[0], status[0][:share].cpu().numpy()) and np.array_equal(ref[1], status[1][:share].cpu().numpy())
        return seconds / share * len(ubs) * 1e6

    zeros = torch.zeros(64, dtype=torch.int32, device=be.device)
    while True:                                                        # (the span of 64 makespans that holds the first open one)
        ubs = (start + np.arange(64)).astype(np.int32)
        dev_ubs = torch.from_numpy(ubs).to(be.device)
        out, us, spread = measure(lambda: env.propagate(dev_ubs, parents=zeros, windows=True))
        status = out[0].cpu().numpy()
        if (status != 1).any():
            break
        start += 64
    first = int(ubs[np.flatnonzero(status != 1)[0]])
    lines = []
    if kind == "scan":
        twin_us = twin_check(out, ubs)
        lines.append(f"case {name}: scan, 64 makespans from {start}        x {64:6d} {us:12.1f} us {spread}   {64 / us * 1e6:10.0f} propagations/s   "
                     f"first open {first}, passes at most {int(out[1].max())}; one-thread twin {twin_us:.0f} us ({twin_us / us:.1f} x)")
        return lines
    at = int(first - start)
    est, lct = out[2][at].cpu().numpy(), out[3][at].cpu().numpy()
    dur = (np.asarray(env.packed.ops).reshape(-1, env.jmax, env.mmax)[0] & 0xFFFF).astype(np.int64)
    ops, mid, d, hyp = search.shaving_hypotheses(est, lct, dur)
    n = 2 * ops.size
    round_ubs = np.full(n, first, np.int32)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(be.device)   # noqa: E731
    args = dict(parents=torch.zeros(n, dtype=torch.int32, device=be.device), est=dev(est), lct=dev(lct), hyp=tuple(dev(x) for x in hyp))
    dev_round = dev(round_ubs)
    out, us, spread = measure(lambda: env.propagate(dev_round, **args))
    twin_us = twin_check(out, round_ubs, est, lct, hyp)
    gone = (out[0].cpu().numpy() == 1).reshape(-1, 2)
    lines.append(f"case {name}: shaving round at {first}             x {n:6d} {us:12.1f} us {spread}   {n / us * 1e6:10.0f} propagations/s   "
                 f"halves refuted {int(gone.sum())}, operations with both {int(gone.all(axis=1).sum())}, passes at most {int(out[1].max())}; "
                 f"one-thread twin {twin_us:.0f} us ({twin_us / us:.1f} x)")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--twin", type=int, default=16, help="candidates of every launch the one-thread twin checks and is timed on")
    ap.add_argument("--limit", type=int, default=150, help="seconds per step")
    ap.add_argument("--steps", default=",".join(STEPS))
    ap.add_argument("--step", default=None, help="(internal) run that step in this process")
    args = ap.parse_args()
    if args.step:
        print("\n".join(step(args.step, args.windows, args.twin)), flush=True)
        return 0
    import torch
    lines = [f"# device {torch.cuda.get_device_name(0)}; HIP events around one call, median (min .. max) of {args.windows} calls; every step a "
             f"process of its own under a limit of {args.limit} s"]
    print(lines[0], flush=True)
    status = 0
    for what in args.steps.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", what, "--windows", str(args.windows), "--twin", str(args.twin)]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            lines.append(f"step {what}: no answer within {args.limit} s; nothing more is started")
            status = 124
        else:
            if out.returncode:
                lines.append(f"step {what}: exit status {out.returncode}; nothing more is started\n{out.stderr[-2000:]}")
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
