"""Timings of beam search on the device (jssenv_amd.search): jss_beam_select against the torch form of the same selection,
the selection's share of a level, and a whole beam_search.
usage: python tools/gpu_beam_probe.py [--out FILE.json] [--prefix LEVELS] [--windows N] [--reps N]

Per case, G copies of one instance at width W.  The state that is timed is the beam after --prefix levels of the search (every
slot filled).  HIP events around --reps back-to-back calls, warmed up, the median of --windows such windows.  The torch form is
what a user would write without the kernel: a masked key, one topk per problem row, integer divisions and gathers; it gives
the plain top-W only (no dedupe), and its src / action are asserted equal to the kernel's with dedupe off."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from jssenv_amd import search  # noqa: E402
from jssenv_amd.env import HipBackend  # noqa: E402

CASES = [("a", "ta01", 64, 64), ("b", "ta41", 16, 32), ("c", "ta61", 8, 32)]        # ta61: 50 x 20


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
    return float(np.median(out))


def torch_select(cand_parent, makespan, done, env_makespan, G, W, A):
    """the plain top-W of include/jss_beam.h in torch: (src, action), -1 where a slot stays empty"""
    S = G * W
    slot = torch.arange(S, device=makespan.device)
    live = cand_parent.view(S, A)[:, 0] == slot
    fin = done.view(torch.bool)
    first = torch.arange(A, device=makespan.device) == 0
    m = torch.where(fin[:, None], torch.where(first[None, :], env_makespan[:, None], -1), makespan.view(S, A))
    valid = live[:, None] & (m >= 0)
    c = torch.arange(W * A, device=makespan.device)
    key = torch.where(valid.view(G, W * A), m.view(G, W * A).long() * (W * A) + c, torch.iinfo(torch.int64).max)
    best, _ = key.topk(min(W, W * A), dim=1, largest=False, sorted=True)
    got = best != torch.iinfo(torch.int64).max
    c_best = best % (W * A)
    src = torch.arange(G, device=makespan.device)[:, None] * W + c_best // A
    src = torch.where(got, src, -1)
    action = torch.where(got & ~fin[src.clamp(min=0)], c_best % A, -1)
    return src.view(-1).int(), action.view(-1).int()


def probe(be, tag, name, G, W, prefix, windows, reps):
    insts = [name] * G if G > 1 else name
    res = search.beam_search(insts, "SPT", width=W, max_levels=prefix, check_every=prefix, record=False, _backend=be)
    a = res.env
    S, A = a.batch, a.jmax + 1
    b = a.fork(np.arange(S))
    t = torch
    dev = be.device
    acts = t.arange(A, dtype=t.int32, device=dev).repeat(S)
    mk, st = t.zeros(S * A, dtype=t.int32, device=dev), t.zeros(S * A, dtype=t.int32, device=dev)
    rn = t.zeros(S * A, dtype=t.int64, device=dev)
    out = {k: t.zeros(S, dtype=t.int32, device=dev) for k in ("src", "action", "score")}
    nxt, counts = t.zeros(S * A, dtype=t.int32, device=dev), t.zeros((G, 4), dtype=t.int32, device=dev)
    sel = a._selector("SPT", "probe")
    lib = search.beam_library(be)
    n_iter = 3 * a.jmax * a.mmax
    cand = res.cand_parent

    def lookahead():
        search.lookahead_into(a, sel, cand, acts, mk, st, rn, a.seed, 0, n_iter)

    def select(dedupe=True):
        search._select_call(be, lib, G, W, A, dedupe, cand, mk, st, rn, a.done, a.makespan, out["src"], out["action"], out["score"],
                            nxt, counts)

    def expand():
        b._clone_from(a, out["src"])
        b.step(out["action"])

    def back():                                       # (timed into a third batch: `a` stays the state that is measured)
        spare._clone_from(b, nxt[::A])

    spare = a.fork(np.arange(S))
    lookahead()
    select(False)
    ts, ta = torch_select(cand, mk, a.done, a.makespan, G, W, A)
    assert t.equal(ts, out["src"]) and t.equal(ta, out["action"]), "the torch chain and the kernel disagree"
    row = {"case": tag, "instance": name, "groups": G, "width": W, "actions": A, "prefix_levels": res.levels}
    row["select_plain_us"] = median_us(lambda: select(False), windows, reps)
    row["torch_plain_us"] = median_us(lambda: torch_select(cand, mk, a.done, a.makespan, G, W, A), windows, reps)
    row["select_dedupe_us"] = median_us(select, windows, reps)
    select()
    t.cuda.synchronize()
    c = counts.cpu().numpy()
    row["valid_per_group"] = [int(c[:, 3].min()), int(c[:, 3].max())]
    row["dropped_per_group"] = [int(c[:, 2].min()), int(c[:, 2].max())]
    row["lookahead_us"] = median_us(lookahead, windows, max(1, reps // 4))
    row["clone_step_us"] = median_us(expand, windows, reps)
    row["clone_back_us"] = median_us(back, windows, reps)
    level = row["lookahead_us"] + row["select_dedupe_us"] + row["clone_step_us"] + row["clone_back_us"]
    row["level_us"] = level
    row["select_share_of_level"] = row["select_dedupe_us"] / level
    t.cuda.synchronize()
    t0 = time.perf_counter()
    full = search.beam_search(insts, "SPT", width=W, record=False, _backend=be)
    t.cuda.synchronize()
    row["search_s"] = time.perf_counter() - t0
    row["search_levels"] = full.levels
    row["search_makespans"] = sorted(set(full.makespan.tolist()))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--prefix", type=int, default=40)
    ap.add_argument("--windows", type=int, default=11)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cases", default="a,b,c")
    args = ap.parse_args()
    be = HipBackend("cuda:0")
    rows = []
    for tag, name, G, W in CASES:
        if tag in args.cases.split(","):
            rows.append(probe(be, tag, name, G, W, args.prefix, args.windows, args.reps))
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "windows": args.windows, "reps": args.reps, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
