"""Timings of jss_bound (include/jss_bound.h) on the device, against jss_lookahead("SPT") on the same candidate list and against
the bytes the case must read over the memory's peak rate.
usage: python tools/gpu_bound_probe.py [--out FILE.txt] [--windows N] [--reps N] [--cases a,b,c] [--steps K]

Cases: (a) ta01 x 65 536 states, their own bounds; (b) 4 096 ta01 parents x 16 columns; (c) 8 192 per-env 50 x 20 parents x 21
columns (a column past J is refused at once; it is part of what a caller passes).  The states are --steps random steps into
their episodes, so that scheduled and unscheduled operations both occur.  HIP events around --reps back-to-back calls, warmed
up, the median of --windows such windows.

Bytes a case must read: per DISTINCT parent its solution rows and, per distinct table, the op and work tables (J x M x 4 bytes
each, counted once: candidates of one parent share them), per candidate 8 bytes of parent / action and a mask byte, plus 4
bytes written.  The floor is those bytes over 8 TB/s; it says how far the kernel is from a pure stream, not what a latency-
bound walk can reach."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ctypes as C  # noqa: E402

from jssenv_amd import BatchedJssEnv, _abi, search  # noqa: E402
from jssenv_amd import instances as I  # noqa: E402
from jssenv_amd.env import HipBackend  # noqa: E402

PEAK_BYTES_PER_S = 8e12


def median_us(fn, windows, reps):
    """median over `windows` of the time of one call, from HIP events around `reps` calls"""
    for _ in range(3):
        fn()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / reps)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def make_case(be, tag):
    if tag == "a":
        env, columns = BatchedJssEnv("ta01", batch=65536, _backend=be, seed=1), None
    elif tag == "b":
        env, columns = BatchedJssEnv("ta01", batch=4096, _backend=be, seed=2), 16
    else:
        env, columns = BatchedJssEnv(I.synthetic_packed(8192, 50, 20), batch=8192, _backend=be, seed=3), 21
    return env, columns


def probe(be, tag, steps, windows, reps):
    t = torch
    env, columns = make_case(be, tag)
    env.reset()
    env.rollout("random", n_iter=steps, autoreset=False)
    B, J, M = env.batch, env.jmax, env.mmax
    dev = be.device
    if columns is None:
        par = t.arange(B, dtype=t.int32, device=dev)
        act = t.full((B,), _abi.ACTION_SKIP, dtype=t.int32, device=dev)
    else:
        par = t.arange(B, dtype=t.int32, device=dev).repeat_interleave(columns)
        act = t.arange(columns, dtype=t.int32, device=dev).repeat(B)
    n = int(par.shape[0])
    lower = t.zeros(n, dtype=t.int32, device=dev)
    est = t.zeros((n, J, M), dtype=t.int32, device=dev) if n * J * M * 4 <= 2 ** 30 else None
    mk, st, rn = t.zeros(n, dtype=t.int32, device=dev), t.zeros(n, dtype=t.int32, device=dev), t.zeros(n, dtype=t.int64, device=dev)
    lib = search.bound_library(be)
    p = be.ptr
    mask = p(env.action_mask) if columns is not None else None
    arg = _abi.JssBound(n, p(par), p(act), mask, p(lower), None, None)
    arg_est = _abi.JssBound(n, p(par), p(act), mask, p(lower), None, p(est))
    sel = env._selector("SPT", "probe")
    n_iter = 3 * J * M

    def bound(a=arg):
        rc = lib.jss_bound(C.byref(env._desc), C.byref(env._state), C.byref(a), be.stream())
        assert rc == 0, rc

    def lookahead():
        search.lookahead_into(env, sel, par, act, mk, st, rn, env.seed, 0, n_iter)

    bound()
    lookahead()
    t.cuda.synchronize()
    lb, up = lower.cpu().numpy(), mk.cpu().numpy()
    both = (lb >= 0) & (up >= 0)
    assert both.any() and (lb[both] <= up[both]).all(), "a bound above a rollout's makespan"
    tables = 1 if env.n_tables == 1 else B
    need = B * J * M * 4 + tables * 2 * J * M * 4 + n * (8 + (1 if columns is not None else 0) + 4)
    floor_us = need / PEAK_BYTES_PER_S * 1e6
    row = {"case": tag, "parents": B, "columns": columns or 1, "candidates": n, "J": J, "M": M, "evaluated": int((lb >= 0).sum()),
           "bytes_needed": need, "floor_us": floor_us}
    row["bound_us"], row["bound_min_us"], row["bound_max_us"] = median_us(bound, windows, reps)
    if est is not None:
        row["bound_est_start_us"] = median_us(lambda: bound(arg_est), windows, reps)[0]
    row["lookahead_us"] = median_us(lookahead, windows, max(1, reps // 4))[0]
    row["lookahead_over_bound"] = row["lookahead_us"] / row["bound_us"]
    row["bound_over_floor"] = row["bound_us"] / floor_us
    row["mean_gap"] = float((up[both] - lb[both]).mean() / up[both].mean())
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=11)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--cases", default="a,b,c")
    args = ap.parse_args()
    be = HipBackend("cuda:0")
    lines = [f"# device {torch.cuda.get_device_name(0)}; HIP events, median (min .. max) of {args.windows} windows of {args.reps} calls; "
             f"states {args.steps} random steps into their episodes; floor = bytes needed / 8 TB/s"]
    for tag in args.cases.split(","):
        r = probe(be, tag, args.steps, args.windows, args.reps)
        lines.append(f"case {r['case']}: {r['parents']} parents x {r['columns']} columns = {r['candidates']} candidates ({r['evaluated']} "
                     f"evaluated), {r['J']} x {r['M']}")
        lines.append(f"  jss_bound          {r['bound_us']:10.1f} us ({r['bound_min_us']:.1f} .. {r['bound_max_us']:.1f})"
                     + (f"   with est_start {r['bound_est_start_us']:.1f} us" if "bound_est_start_us" in r else ""))
        lines.append(f"  jss_lookahead SPT  {r['lookahead_us']:10.1f} us   = {r['lookahead_over_bound']:.1f} x jss_bound")
        lines.append(f"  bytes needed       {r['bytes_needed']:10d}      floor {r['floor_us']:.2f} us   jss_bound = {r['bound_over_floor']:.1f} x floor")
        lines.append(f"  mean (rollout makespan - bound) / makespan over the evaluated candidates: {r['mean_gap']:.3f}")
        print("\n".join(lines[-5:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
