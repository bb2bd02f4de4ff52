"""Time per move of jss_block_search (include/jss_block.h) on the device, next to jss_tabu_search (include/jss_tabu.h) as the
baseline: the same process, the same batch, the same starts, the two calls alternating.
usage: python tools/gpu_block_probe.py [--out FILE.txt] [--windows N] [--moves N] [--walkers N] [--cases ta01,ta41] [--reach R]

Per case: --walkers walkers of one instance, every one from its own SPT rollout with explore 0.1 (what search.tabu_search starts
from), tenure 8, --moves moves each.  HIP events around one call, two warm-up calls of each kind, then --windows rounds of one
block walk and one swap walk; reported are the median and the spread (min .. max) of a call, and from the median the microseconds
per move per walker -- a call's time over the moves its walkers made, times the walkers: with more walkers than the chip holds
wavefronts at once that is the time of a walker's move under the load of the others, not its latency alone.  Also what the walks
did: moves made, candidates scored (block) or neighbours re-timed (swap) per move, the mean best makespan."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from jssenv_amd import BatchedJssEnv, _abi, search  # noqa: E402
from jssenv_amd.env import HipBackend  # noqa: E402

TENURE = 8


def timed_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0


def probe(be, name, walkers, moves, windows, reach):
    t, dev, p = torch, be.device, be.ptr
    env = BatchedJssEnv(name, batch=walkers, _backend=be, seed=7)
    env.reset()
    env.rollout("SPT", n_iter=3 * env.jmax * env.mmax, autoreset=False, explore=0.1, seed=7)
    B, J, M = env.batch, env.jmax, env.mmax
    out = {}
    for kind, ni in (("block", _abi.BLOCK_NI), ("swap", _abi.TABU_NI)):
        out[kind] = (t.zeros(B, dtype=t.int32, device=dev), t.zeros((B, J, M), dtype=t.int32, device=dev),
                     t.zeros((B, ni), dtype=t.int32, device=dev))
    mk, best, info = out["block"]
    block_arg = _abi.JssBlock(moves, TENURE, reach, p(env.solution), None, None, p(mk), p(best), None, p(info), None, None)
    mk, best, info = out["swap"]
    swap_arg = _abi.JssTabu(moves, TENURE, p(env.solution), None, None, p(mk), p(best), None, p(info), None)
    block_lib, swap_lib = search.block_library(be), search.tabu_library(be)
    d, s = C.byref(env._desc), C.byref(env._state)

    def block():
        assert block_lib.jss_block_search(d, s, C.byref(block_arg), be.stream()) == 0

    def swap():
        assert swap_lib.jss_tabu_search(d, s, C.byref(swap_arg), be.stream()) == 0

    for _ in range(2):
        block(), swap()
    t.cuda.synchronize()
    times = {"block": [], "swap": []}
    for _ in range(windows):                                           # alternating: what else runs on the host hits both alike
        times["block"].append(timed_us(block))
        times["swap"].append(timed_us(swap))
    start = env.evaluate_order()
    t.cuda.synchronize()
    row = {"case": name, "walkers": B, "J": J, "M": M, "moves": moves, "before": float(start.float().mean())}
    for kind in ("block", "swap"):
        mk, _, info = out[kind]
        assert (mk > 0).all() and (mk <= start).all(), "a walk ended above its start"
        made = int(info[:, 1].sum())
        row[kind] = dict(us=float(np.median(times[kind])), lo=float(np.min(times[kind])), hi=float(np.max(times[kind])), made=made,
                         scored=int(info[:, 3].sum()), after=float(mk.float().mean()), stopped=int((info[:, 0] != 0).sum()))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--moves", type=int, default=200)
    ap.add_argument("--walkers", type=int, default=4096)
    ap.add_argument("--cases", default="ta01,ta41")
    ap.add_argument("--reach", type=int, default=0)
    args = ap.parse_args()
    be = HipBackend("cuda:0")
    lines = [f"# device {torch.cuda.get_device_name(0)}; HIP events around one call, median (min .. max) of {args.windows} calls, the two "
             f"kinds alternating; tenure {TENURE}; reach {args.reach}; starts: SPT rollouts, explore 0.1"]
    for name in args.cases.split(","):
        r = probe(be, name, args.walkers, args.moves, args.windows, args.reach)
        lines.append(f"case {r['case']}: {r['walkers']} walkers, {r['J']} x {r['M']}, at most {r['moves']} moves each; mean start {r['before']:.1f}")
        for kind, what in (("block", "jss_block_search"), ("swap", "jss_tabu_search ")):
            k = r[kind]
            per_move = k["us"] * r["walkers"] / max(1, k["made"])
            lines.append(f"  {what} {k['us']:12.1f} us ({k['lo']:.1f} .. {k['hi']:.1f})   {per_move:8.3f} us per move per walker "
                         f"({per_move * k['lo'] / k['us']:.3f} .. {per_move * k['hi'] / k['us']:.3f})   {k['made']} moves, "
                         f"{k['scored'] / max(1, k['made']):.1f} {'candidates scored' if kind == 'block' else 'neighbours re-timed'} per move, "
                         f"mean best {k['after']:.1f}, {k['stopped']} walkers stopped early")
        b, s = r["block"], r["swap"]
        ratio = (s["us"] / max(1, s["made"])) / (b["us"] / max(1, b["made"]))
        lines.append(f"  a swap walk's move takes {ratio:.2f} x a block walk's move")
        print("\n".join(lines[-4:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if os.path.isfile(args.out) else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
