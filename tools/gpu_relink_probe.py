"""Time per move of jss_relink_walk (include/jss_relink.h) on the device, next to jss_block_search (include/jss_block.h) as the
baseline: the same process, the same batch, the same starts, the two calls alternating.
usage: python tools/gpu_relink_probe.py [--out FILE.txt] [--windows N] [--moves N] [--walkers N] [--cases ta01,ta41]

Per case: --walkers walkers of one instance, every one from its own SPT rollout with explore 0.1 (what search.relink_search
starts from); the guide of every walker is walker 0's order, and a relinking walk goes all the way (until 0, no step limit), so
a walker makes as many moves as its order is apart from the guide's.  The block walk makes --moves moves per walker with tenure
8.  HIP events around one call, two warm-up calls of each kind, then --windows rounds of one relinking call and one block walk;
reported are the median and the spread (min .. max) of a call, and from the median the microseconds per move per walker -- a
call's time over the moves its walkers made, times the walkers: with more walkers than the chip holds wavefronts at once that is
the time of a walker's move under the load of the others, not its latency alone.  A relinking call ends with its longest walk, so
its per-move figure carries the idle tail of the shorter ones.  Also what the walks did: the distances, the candidates per move,
the moves without a sure candidate, and how far below both ends the best order on the path lies."""
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


def probe(be, name, walkers, moves, windows):
    t, dev, p = torch, be.device, be.ptr
    env = BatchedJssEnv(name, batch=walkers, _backend=be, seed=7)
    env.reset()
    env.rollout("SPT", n_iter=3 * env.jmax * env.mmax, autoreset=False, explore=0.1, seed=7)
    B, J, M = env.batch, env.jmax, env.mmax
    guide = env.solution[0:1].expand(B, J, M).contiguous()
    ints = lambda *shape: t.zeros(shape, dtype=t.int32, device=dev)   # noqa: E731
    mk, best, last, info = ints(B), ints(B, J, M), ints(B), ints(B, _abi.RELINK_NI)
    relink_arg = _abi.JssRelink(_abi.RELINK_MAX_STEPS, 0, 0, p(env.solution), p(guide), None, p(mk), p(best), p(last), None, p(info),
                                None, None)
    bmk, bbest, binfo = ints(B), ints(B, J, M), ints(B, _abi.BLOCK_NI)
    block_arg = _abi.JssBlock(moves, TENURE, 0, p(env.solution), None, None, p(bmk), p(bbest), None, p(binfo), None, None)
    relink_lib, block_lib = search.relink_library(be), search.block_library(be)
    d, s = C.byref(env._desc), C.byref(env._state)

    def relink():
        assert relink_lib.jss_relink_walk(d, s, C.byref(relink_arg), be.stream()) == 0

    def block():
        assert block_lib.jss_block_search(d, s, C.byref(block_arg), be.stream()) == 0

    for _ in range(2):
        relink(), block()
    t.cuda.synchronize()
    times = {"relink": [], "block": []}
    for _ in range(windows):                                           # alternating: what else runs on the host hits both alike
        times["relink"].append(timed_us(relink))
        times["block"].append(timed_us(block))
    start, end = env.evaluate_order(), env.evaluate_order(guide)
    t.cuda.synchronize()
    assert (mk > 0).all() and (info[:, 0] == 1).all() and (info[:, 4] == 0).all() and (last == end).all(), "a walk did not arrive"
    assert (mk <= t.minimum(start, end)).all() and (bmk > 0).all()
    row = {"case": name, "walkers": B, "J": J, "M": M, "moves": moves}
    for kind, made in (("relink", int(info[:, 1].sum())), ("block", int(binfo[:, 1].sum()))):
        row[kind] = dict(us=float(np.median(times[kind])), lo=float(np.min(times[kind])), hi=float(np.max(times[kind])), made=made)
    row["relink"].update(dist=float(info[:, 3].float().mean()), far=int(info[:, 3].max()), candidates=int(info[:, 5].sum()),
                         fallbacks=int(info[:, 6].sum()), retries=int(info[:, 7].sum()),
                         below=float((t.minimum(start, end) - mk).float().mean()), lower=int((mk < t.minimum(start, end)).sum()))
    row["block"].update(scored=int(binfo[:, 3].sum()))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--moves", type=int, default=200)
    ap.add_argument("--walkers", type=int, default=4096)
    ap.add_argument("--cases", default="ta01,ta41")
    args = ap.parse_args()
    be = HipBackend("cuda:0")
    lines = [f"# device {torch.cuda.get_device_name(0)}; HIP events around one call, median (min .. max) of {args.windows} calls, the two "
             f"kinds alternating; starts: SPT rollouts, explore 0.1; guide: walker 0's order; block walk: tenure {TENURE}"]
    for name in args.cases.split(","):
        r = probe(be, name, args.walkers, args.moves, args.windows)
        k = r["relink"]
        lines.append(f"case {r['case']}: {r['walkers']} walkers, {r['J']} x {r['M']}; mean distance to the guide {k['dist']:.1f}, "
                     f"largest {k['far']}")
        per = {}
        for kind, what in (("relink", "jss_relink_walk "), ("block", "jss_block_search")):
            k = r[kind]
            per[kind] = k["us"] * r["walkers"] / max(1, k["made"])
            lines.append(f"  {what} {k['us']:12.1f} us ({k['lo']:.1f} .. {k['hi']:.1f})   {per[kind]:8.3f} us per move per walker "
                         f"({per[kind] * k['lo'] / k['us']:.3f} .. {per[kind] * k['hi'] / k['us']:.3f})   {k['made']} moves")
        k = r["relink"]
        lines.append(f"  relinking: {k['candidates'] / max(1, k['made']):.1f} candidates per move, {k['fallbacks']} moves without a sure "
                     f"candidate, {k['retries']} swapped back; the best order on a path lies {k['below']:.1f} below the better end on "
                     f"average, strictly below it on {k['lower']} of {r['walkers']} paths")
        lines.append(f"  block walk: {r['block']['scored'] / max(1, r['block']['made']):.1f} candidates scored per move; a block walk's "
                     f"move takes {per['block'] / per['relink']:.2f} x a relinking move")
        print("\n".join(lines[-5:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if os.path.isfile(args.out) else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
