"""Builds and solves per second of jss_bottleneck_exact and jss_machine_solve (include/jss_carlier.h) on the device, next to
jss_bottleneck_build and jss_machine_relax (include/jss_machine.h) on the same batch in the same run: what sequencing the machines
exactly costs over Schrage's schedule, and what it builds.  No ratio is asked of anything.
usage: python tools/gpu_carlier_probe.py [--out FILE.txt] [--windows N] [--cases ta01,ta41] [--builds 4096] [--solves 65536]
                                         [--budgets 1,256] [--limit SECONDS]

Every step -- one instance -- runs in a child process of its own under a time limit of its own; the first step that fails, is
killed or runs out of time ends the probe, and nothing more is started on the device.  A step: ONE env of the instance; `builds`
candidates on env 0 with seeded integer biases in [0, 50] (candidate 0 unbiased) at reopt 0 and 1 -- first the existing
`bottleneck`, then `bottleneck_exact` at every budget -- then `solves` candidates of the empty selection through `relax_machines`
(jps, schrage) and through `solve_machines` (opt, low) at every budget; two warm-up calls, then --windows calls, HIP events around
one call; reported are the median and the spread (min .. max) of a call and, from the median, candidates per second.  The builds
at a budget of one node are compared with the existing kernel's bit for bit, the first `--twin` builds of every budget with the
one-thread host twin's."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step(name, builds, solves, windows, budgets, twin_share):
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

    def measure(fn):
        for _ in range(2):
            out = fn()
        torch.cuda.synchronize()
        times = [timed_us(fn) for _ in range(windows)]
        return out, float(np.median(times)), f"({min(times):.1f} .. {max(times):.1f})"

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
    share = min(twin_share, builds)
    lines = [f"case {name}: {J} x {M}, candidates of one env"]
    for reopt in (0, 1):
        (mk0, rank0, info0), us0, spread = measure(lambda: env.bottleneck(parents, bias, reopt))
        lines.append(f"  bottleneck       reopt {reopt}            x {builds:6d} {us0:12.1f} us {spread}   {builds / us0 * 1e6:10.0f} builds/s   "
                     f"makespan unbiased {int(mk0[0])}, best {int(mk0.min())}, mean {mk0.float().mean().item():.1f}")
        for nodes in budgets:
            (mk, rank, info), us, spread = measure(lambda: env.bottleneck_exact(parents, bias, reopt, nodes))
            assert (mk > 0).all()
            if nodes == 1:
                assert torch.equal(mk, mk0) and torch.equal(rank, rank0) and torch.equal(info[:, :4], info0)
            twin_mk, _, twin_info = host.bottleneck_exact(np.zeros(share, np.int32), bias_host[:share], reopt, nodes)
            assert np.array_equal(twin_mk, mk[:share].cpu().numpy()) and np.array_equal(twin_info, info[:share].cpu().numpy())
            f = info.float()
            lines.append(f"  bottleneck_exact reopt {reopt} nodes {nodes:4d} x {builds:6d} {us:12.1f} us {spread}   {builds / us * 1e6:10.0f} builds/s   "
                         f"makespan unbiased {int(mk[0])}, best {int(mk.min())}, mean {mk.float().mean().item():.1f}; per build: nodes "
                         f"{f[:, 4].mean().item():.0f}, most of one problem {int(info[:, 5].max())}, left open {f[:, 6].mean().item():.2f}, "
                         f"replaced {int(info[:, 7].sum())}; {us / us0:.2f} x bottleneck's time")
    parents = torch.zeros(solves, dtype=torch.int32, device=be.device)
    old, us0, spread = measure(lambda: env.relax_machines(None, 0, parents, jps=True, schrage=True))
    lines.append(f"  relax_machines                      x {solves:6d} {us0:12.1f} us {spread}   {solves / us0 * 1e6:10.0f} relaxations/s   "
                 f"lower bound {int(old[0][0])}, length {int(old[1][0])}")
    for nodes in budgets:
        out, us, spread = measure(lambda: env.solve_machines(None, 0, parents, nodes, opt=True, low=True, nodes_used=True))
        if nodes == 1:
            assert torch.equal(out[3], old[4]) and torch.equal(out[4], old[3]) and torch.equal(out[0], old[0])
        twin_out = host.solve_machines(None, 0, np.zeros(share, np.int32), nodes, opt=True, low=True, nodes_used=True)
        assert all(np.array_equal(a, b[:share].cpu().numpy()) for a, b in zip(twin_out, out))
        lines.append(f"  solve_machines           nodes {nodes:4d} x {solves:6d} {us:12.1f} us {spread}   {solves / us * 1e6:10.0f} solves/s   "
                     f"lower bound {int(out[0][0])}, nodes per solve {int(out[5][0].clamp(min=0).sum())}, most of one machine {int(out[5][0].max())}; "
                     f"{us / us0:.2f} x relax_machines' time")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--cases", default="ta01,ta41")
    ap.add_argument("--builds", type=int, default=4096)
    ap.add_argument("--solves", type=int, default=65536)
    ap.add_argument("--budgets", default="1,256")
    ap.add_argument("--twin", type=int, default=64, help="candidates the one-thread twin checks")
    ap.add_argument("--limit", type=int, default=200, help="seconds per step")
    ap.add_argument("--step", default=None, help="(internal) case: run that step in this process")
    args = ap.parse_args()
    budgets = [int(x) for x in args.budgets.split(",")]
    if args.step:
        print("\n".join(step(args.step, args.builds, args.solves, args.windows, budgets, args.twin)), flush=True)
        return 0
    import torch
    lines = [f"# device {torch.cuda.get_device_name(0)}; HIP events around one call, median (min .. max) of {args.windows} calls; seeded biases in "
             f"[0, 50]; every step a process of its own under a limit of {args.limit} s"]
    print(lines[0], flush=True)
    status = 0
    for name in args.cases.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--windows", str(args.windows), "--builds", str(args.builds),
               "--solves", str(args.solves), "--budgets", args.budgets, "--twin", str(args.twin)]
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
