"""Timings of jss_order_eval (include/jss_order.h) and of a whole search.improve on the device, next to the host-core twin on 16
threads, jss_lookahead("SPT") over the same number of candidates, and the bytes the case must read over the memory's peak rate.
usage: python tools/gpu_order_probe.py [--out FILE.txt] [--windows N] [--reps N] [--cases a,b,c,d] [--twin-threads N]

Cases: (a) 65 536 ta01 rows -- finished random rollouts, evaluated plain and with start, tail and pairs; (b) 4 096 ta01 rows x
their swap candidates (pair_cap 64, the lists as the rows' evaluation wrote them: entries behind a row's count are (-1, -1), no
swap, and are evaluated all the same); (c) 8 192 per-env 50 x 20 rows; (d) one whole improve on 4 096 SPT schedules of ta01:
iterations, wall time, mean makespan before and after.  HIP events around --reps back-to-back calls, warmed up, the median of
--windows such windows; the twin by the wall clock, the median of 3 calls.  Every case is a run of its own (--cases), so that a
caller can give each its own time limit.

Bytes a case must read: per candidate its rank row, 8 bytes of parent and 8 of swap where given, 4 written; the op table once
per distinct table (J x M x 4 bytes).  The floor is those bytes over 8 TB/s; it says how far the kernel is from a pure stream,
not what a latency-bound walk in rounds can reach."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from jssenv_amd import BatchedJssEnv, _abi, search  # noqa: E402
from jssenv_amd import instances as I  # noqa: E402
from jssenv_amd.env import CpuBackend, HipBackend  # noqa: E402

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


def wall_us(fn, calls=3):
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(out))


def make_env(be, tag, batch=None):
    if tag == "c":
        B = batch or 8192
        return BatchedJssEnv(I.synthetic_packed(B, 50, 20), batch=B, _backend=be, seed=3)
    return BatchedJssEnv("ta01", batch=batch or (65536 if tag == "a" else 4096), _backend=be, seed=1 if tag == "a" else 2)


def finished(env, kind="random"):
    env.reset()
    env.rollout(kind, n_iter=3 * env.jmax * env.mmax, autoreset=False)
    return env


def eval_call(be, env, arg):
    lib = search.order_library(be)

    def call():
        rc = lib.jss_order_eval(C.byref(env._desc), C.byref(env._state), C.byref(arg), be.stream())
        assert rc == 0, rc
    return call


def probe_eval(be, tag, windows, reps, twin_threads):
    t, dev, p = torch, be.device, be.ptr
    env = finished(make_env(be, tag))
    B, J, M = env.batch, env.jmax, env.mmax
    cap = 64
    rank = env.solution
    mk = t.zeros(B, dtype=t.int32, device=dev)
    start, tail = (t.zeros((B, J, M), dtype=t.int32, device=dev) for _ in range(2))
    pa, pb = (t.zeros((B, cap), dtype=t.int32, device=dev) for _ in range(2))
    found = t.zeros(B, dtype=t.int32, device=dev)
    plain = _abi.JssOrder(B, 0, p(rank), None, None, None, p(mk), None, None, None, None, None)
    full = _abi.JssOrder(B, cap, p(rank), None, None, None, p(mk), p(start), p(tail), p(pa), p(pb), p(found))
    eval_call(be, env, full)()
    t.cuda.synchronize()
    assert (mk > 0).all() and (mk <= env.makespan.to(t.int32).reshape(-1)).all(), "a re-timed schedule longer than the env's"
    tables = 1 if env.n_tables == 1 else B
    if tag == "b":                                                    # the rows' swap candidates
        n = B * cap
        par = t.arange(B, dtype=t.int32, device=dev).repeat_interleave(cap)
        cand_mk = t.zeros(n, dtype=t.int32, device=dev)
        arg = _abi.JssOrder(n, 0, p(rank), p(par), p(pa), p(pb), p(cand_mk), None, None, None, None, None)
        need = n * (J * M * 4 + 8 + 8 + 4) + tables * J * M * 4
        real = int(t.clamp(found, max=cap).sum())
    else:
        n, arg, real = B, plain, B
        need = n * (J * M * 4 + 4) + tables * J * M * 4
    row = {"case": tag, "rows": B, "candidates": n, "real": real, "J": J, "M": M, "bytes_needed": need,
           "floor_us": need / PEAK_BYTES_PER_S * 1e6, "mean_pairs": float(found.float().mean()), "max_pairs": int(found.max())}
    row["eval_us"], row["eval_min_us"], row["eval_max_us"] = median_us(eval_call(be, env, arg), windows, reps)
    if tag != "b":
        row["eval_full_us"] = median_us(eval_call(be, env, full), windows, reps)[0]
    # jss_lookahead("SPT") over as many candidates: fresh envs, no move, so every candidate is one whole SPT rollout
    la_env = make_env(be, tag)
    la_env.reset()
    la_par = (t.arange(n, dtype=t.int64, device=dev) % B).to(t.int32)
    la_act = t.full((n,), _abi.ACTION_SKIP, dtype=t.int32, device=dev)
    la_mk, la_st, la_rn = t.zeros(n, dtype=t.int32, device=dev), t.zeros(n, dtype=t.int32, device=dev), t.zeros(n, dtype=t.int64, device=dev)
    sel = la_env._selector("SPT", "probe")
    row["lookahead_us"] = median_us(lambda: search.lookahead_into(la_env, sel, la_par, la_act, la_mk, la_st, la_rn, la_env.seed, 0,
                                                                  3 * J * M), max(3, windows // 3), max(1, reps // 10))[0]
    # the twin, on a sixteenth of the candidates (the same rows), scaled
    cpu = CpuBackend()
    cpu.threads = twin_threads
    part = max(1, B // 16)
    cenv = finished(make_env(cpu, tag, batch=part))
    c_rank = np.ascontiguousarray(cenv.solution)
    if tag == "b":
        c_mk, c_pa, c_pb, _ = cenv.evaluate_order(c_rank, pairs=cap)
        c_par = np.repeat(np.arange(part, dtype=np.int32), cap)
        c_sa, c_sb = np.ascontiguousarray(c_pa.reshape(-1)), np.ascontiguousarray(c_pb.reshape(-1))
        row["twin_us"] = wall_us(lambda: cenv.evaluate_order(c_rank, c_par, (c_sa, c_sb))) * (B / part)
    else:
        row["twin_us"] = wall_us(lambda: cenv.evaluate_order(c_rank)) * (B / part)
    return row


def probe_improve(be):
    env = make_env(be, "d")
    torch.cuda.synchronize()
    warm = search.improve(finished(make_env(be, "d", batch=64), "SPT"))   # (loads the library, warms the launches)
    assert warm.iterations > 0
    env = finished(env, "SPT")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = search.improve(env)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return {"envs": env.batch, "iterations": res.iterations, "launched": int(res.history.shape[0]), "evaluations": res.evaluations,
            "truncated": res.truncated, "wall_ms": wall * 1e3, "before": float(res.makespan_before.mean()), "after": float(res.makespan.mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=11)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cases", default="a,b,c,d")
    ap.add_argument("--twin-threads", type=int, default=16)
    args = ap.parse_args()
    be = HipBackend("cuda:0")
    lines = [f"# device {torch.cuda.get_device_name(0)}; HIP events, median (min .. max) of {args.windows} windows of {args.reps} calls; "
             f"floor = bytes needed / 8 TB/s; twin on {args.twin_threads} threads, a sixteenth of the rows, scaled"]
    for tag in args.cases.split(","):
        first = len(lines)
        if tag == "d":
            r = probe_improve(be)
            lines.append(f"case d: improve on {r['envs']} SPT schedules of ta01, pair_cap 128, check_every 8")
            lines.append(f"  {r['iterations']} improving iterations ({r['launched']} counted, 3 launches each), {r['evaluations']} neighbours "
                         f"evaluated, {r['truncated']} truncated, wall {r['wall_ms']:.1f} ms")
            lines.append(f"  mean makespan {r['before']:.1f} -> {r['after']:.1f}")
        else:
            r = probe_eval(be, tag, args.windows, args.reps, args.twin_threads)
            lines.append(f"case {r['case']}: {r['rows']} rows, {r['candidates']} candidates ({r['real']} with a swap or a row of their own), "
                         f"{r['J']} x {r['M']}; pairs per row: mean {r['mean_pairs']:.1f}, max {r['max_pairs']}")
            lines.append(f"  jss_order_eval     {r['eval_us']:10.1f} us ({r['eval_min_us']:.1f} .. {r['eval_max_us']:.1f})"
                         + (f"   with start, tail and pairs {r['eval_full_us']:.1f} us" if "eval_full_us" in r else ""))
            lines.append(f"  twin               {r['twin_us']:10.1f} us   = {r['twin_us'] / r['eval_us']:.1f} x jss_order_eval")
            lines.append(f"  jss_lookahead SPT  {r['lookahead_us']:10.1f} us   = {r['lookahead_us'] / r['eval_us']:.1f} x jss_order_eval")
            lines.append(f"  bytes needed       {r['bytes_needed']:10d}      floor {r['floor_us']:.2f} us   jss_order_eval = "
                         f"{r['eval_us'] / r['floor_us']:.1f} x floor")
        print("\n".join(lines[first:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if os.path.isfile(args.out) else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
