"""Timings of jss_tabu_search (include/jss_tabu.h) on the device, next to the three launches of one search.improve iteration run as
often as the walk has moves, and to the host-core twin on 16 threads.
usage: python tools/gpu_tabu_probe.py [--out FILE.txt] [--windows N] [--moves N] [--cases a,b,c] [--twin-threads N]

Cases: (a) 4 096 ta01 walkers, (b) 64 ta01 walkers, (c) 1 024 walkers of one 50 x 20 instance; every walker starts from its own
SPT rollout with explore 0.1 and walks --moves moves with tenure 8.  HIP events around one call, warmed up, the median of
--windows calls; reported with the moves made and the neighbours evaluated per second.  The baseline is what the package offered
before: --moves times the three launches of an improve iteration (jss_order_eval of the rows with the pairs out, jss_order_eval
of batch x 128 candidates, jss_order_apply) on the same batch -- a descent, which stops moving at its local optimum but keeps
launching, so its time is the time of that launch structure, not of a search of equal quality.  The twin by the wall clock, the
median of 3 calls, on a sixteenth of the walkers, scaled.  Every case is a run of its own (--cases), so that a caller can give
each its own time limit."""
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

CASES = {"a": ("ta01", 4096), "b": ("ta01", 64), "c": ("50x20", 1024)}
TENURE, CAP = 8, 128


def median_us(fn, windows):
    for _ in range(2):
        fn()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1000.0)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def started(be, tag, batch=None):
    """the case's batch: every env reset and rolled out by SPT with explore 0.1"""
    name, B = CASES[tag]
    inst = I.taillard_instance(50, 20, 4711, 815, name="syn50x20") if name == "50x20" else name
    env = BatchedJssEnv(inst, batch=batch or B, _backend=be, seed=7)
    env.reset()
    env.rollout("SPT", n_iter=3 * env.jmax * env.mmax, autoreset=False, explore=0.1, seed=7)
    return env


def probe(be, tag, windows, moves, twin_threads):
    t, dev, p = torch, be.device, be.ptr
    env = started(be, tag)
    B, J, M = env.batch, env.jmax, env.mmax
    lib = search.tabu_library(be)
    mk = t.zeros(B, dtype=t.int32, device=dev)
    best = t.zeros((B, J, M), dtype=t.int32, device=dev)
    info = t.zeros((B, _abi.TABU_NI), dtype=t.int32, device=dev)
    arg = _abi.JssTabu(moves, TENURE, p(env.solution), None, None, p(mk), p(best), None, p(info), None)

    def tabu():
        rc = lib.jss_tabu_search(C.byref(env._desc), C.byref(env._state), C.byref(arg), be.stream())
        assert rc == 0, rc

    row = {"case": tag, "walkers": B, "J": J, "M": M, "moves": moves}
    row["tabu_us"], row["tabu_min_us"], row["tabu_max_us"] = median_us(tabu, windows)
    start = env.evaluate_order()
    t.cuda.synchronize()
    assert (mk > 0).all() and (mk <= start).all(), "a walk ended above its start"
    row["made"], row["evaluated"] = int(info[:, 1].sum()), int(info[:, 3].sum())
    row["before"], row["after"] = float(start.float().mean()), float(mk.float().mean())

    # the baseline: `moves` iterations of improve's three launches on the same batch
    olib = search.order_library(be)
    rank = env.solution.clone()
    cur = env.evaluate_order(rank)
    par = t.arange(B, dtype=t.int32, device=dev).repeat_interleave(CAP)
    pa, pb = (t.zeros((B, CAP), dtype=t.int32, device=dev) for _ in range(2))
    cand_mk = t.zeros(B * CAP, dtype=t.int32, device=dev)
    row_mk, found, improved = (t.zeros(B, dtype=t.int32, device=dev) for _ in range(3))
    rows = _abi.JssOrder(B, CAP, p(rank), None, None, None, p(row_mk), None, None, p(pa), p(pb), p(found))
    cands = _abi.JssOrder(B * CAP, 0, p(rank), p(par), p(pa), p(pb), p(cand_mk), None, None, None, None, None)
    apply = _abi.JssOrderApply(B, J, M, CAP, p(rank), p(cur), p(cand_mk), p(pa), p(pb), p(improved))
    d, s = C.byref(env._desc), C.byref(env._state)

    def three_launches():
        for _ in range(moves):
            assert olib.jss_order_eval(d, s, C.byref(rows), be.stream()) == 0
            assert olib.jss_order_eval(d, s, C.byref(cands), be.stream()) == 0
            assert olib.jss_order_apply(C.byref(apply), be.stream()) == 0

    row["descent_us"] = median_us(three_launches, max(3, windows // 3))[0]
    row["descent_after"] = float(cur.float().mean())

    # the twin, on a sixteenth of the walkers (at least 16), scaled
    cpu = CpuBackend()
    cpu.threads = twin_threads
    part = max(16, B // 16)
    cenv = started(cpu, tag, batch=part)
    calls = []
    for _ in range(3):
        t0 = time.perf_counter()
        cenv.tabu(None, moves, TENURE)
        calls.append((time.perf_counter() - t0) * 1e6)
    row["twin_us"] = float(np.median(calls)) * (B / part)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=11)
    ap.add_argument("--moves", type=int, default=100)
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--twin-threads", type=int, default=16)
    args = ap.parse_args()
    be = HipBackend("cuda:0")
    lines = [f"# device {torch.cuda.get_device_name(0)}; HIP events around one call, median (min .. max) of {args.windows} calls; tenure "
             f"{TENURE}; starts: SPT rollouts, explore 0.1; twin on {args.twin_threads} threads, a sixteenth of the walkers, scaled"]
    for tag in args.cases.split(","):
        r = probe(be, tag, args.windows, args.moves, args.twin_threads)
        sec = r["tabu_us"] * 1e-6
        lines.append(f"case {r['case']}: {r['walkers']} walkers, {r['J']} x {r['M']}, {r['moves']} moves each; mean makespan "
                     f"{r['before']:.1f} -> {r['after']:.1f}; {r['evaluated'] / max(1, r['made']):.1f} neighbours per move")
        lines.append(f"  jss_tabu_search        {r['tabu_us']:12.1f} us ({r['tabu_min_us']:.1f} .. {r['tabu_max_us']:.1f})   "
                     f"{r['made'] / sec:.3e} moves/s   {r['evaluated'] / sec:.3e} neighbour evaluations/s")
        lines.append(f"  {r['moves']} x improve's 3 launches {r['descent_us']:12.1f} us   = {r['descent_us'] / r['tabu_us']:.2f} x jss_tabu_search"
                     f"   (pair_cap {CAP}; a descent: mean makespan {r['before']:.1f} -> {r['descent_after']:.1f})")
        lines.append(f"  twin                   {r['twin_us']:12.1f} us   = {r['twin_us'] / r['tabu_us']:.2f} x jss_tabu_search")
        print("\n".join(lines[-4:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if os.path.isfile(args.out) else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
