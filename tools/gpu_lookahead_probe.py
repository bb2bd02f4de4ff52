"""Candidate moves scored by rule rollouts (jss_lookahead) against the same scores built from clones (GPU box):

  (a) ta01, compact records: 4 096 parents mid-episode x 16 candidates (SKIP + the 15 jobs; the NOPE column of ta01 is the
      16th action, SKIP takes its place so that every candidate of a parent sits in one 16-lane group)
  (b) synthetic 50 x 20, medium records, one table per env: 512 parents x 21 candidates (SKIP + the 20 first jobs)
  (c) config 5 by shape (ta01-ta80, the envs dealt out by shape class): 2 048 parents x every action (jmax + 1 = 101 columns)

For each: `lookahead("SPT")` on the candidate list against fork(parents) + step(actions) + rollout("SPT") on the same list,
same seeds -- the makespans of the legal candidates must agree (the script asserts it) -- and a whole `pilot_step("SPT")`
against the same step built from a fork (fork every legal candidate, step, rollout, masked argmin, step).  Device times are
HIP events: warm-up, then the median of windows of K calls each.  The pilot steps run on a fresh copy of the batch each time
(the copy is not timed).  "fork bytes" is the memory of the fork that lookahead never makes, computed from the fork's
shapes (its arena, solution and own tables), not measured.

usage: python tools/gpu_lookahead_probe.py [--windows N] [--warmup W] [--calls K] [--only a|b|c]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from jssenv_amd import BatchedJssEnv, _abi  # noqa: E402
from jssenv_amd.instances import synthetic_packed  # noqa: E402

TA = [f"ta{i:02d}" for i in range(1, 81)]


def time_events(call, windows, warmup, k, prepare=None):
    """median over windows of the mean device time of one call (us); `prepare` runs untimed before every call"""
    for _ in range(warmup):
        if prepare:
            prepare()
        call()
    torch.cuda.synchronize()
    ev = []
    for _ in range(windows):
        total = 0.0
        for _ in range(k):
            if prepare:
                prepare()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            total += e0.elapsed_time(e1) * 1e3
        ev.append(total / k)
    return statistics.median(ev)


def build(case):
    """(name, env, parents, actions) -- parents / actions device int32, parent-major"""
    dev = "cuda:0"
    if case == "a":
        env = BatchedJssEnv("ta01", batch=4096, device=dev, seed=1)
        env.reset()
        env.rollout("random", n_iter=60, autoreset=False, seed=2)
        par, act = np.repeat(np.arange(4096), 16), np.tile(np.arange(-1, 15), 4096)
        name = "(a) ta01 compact, 4096 x 16"
    elif case == "b":
        env = BatchedJssEnv(synthetic_packed(512, 50, 20), batch=512, device=dev, seed=1, records="medium")
        env.reset()
        env.rollout("random", n_iter=300, autoreset=False, seed=2)
        par, act = np.repeat(np.arange(512), 21), np.tile(np.arange(-1, 20), 512)
        name = "(b) 50x20 medium per-env, 512 x 21"
    else:
        env = BatchedJssEnv(TA, batch=2048, device=dev, seed=1)
        env.reset()
        env.rollout("random", n_iter=120, autoreset=False, seed=2)
        A = env.jmax + 1
        par, act = np.repeat(np.arange(2048), A), np.tile(np.arange(A), 2048)
        name = f"(c) config 5 by shape, 2048 x {A}"
    t = lambda x: torch.tensor(x.astype(np.int32), device=dev)   # noqa: E731
    return name, env, t(par), t(act)


def legal_of(env, par, act):
    """host bool per candidate: the parent is not done and the action is SKIP or set in its mask"""
    mask, done = env.action_mask.cpu().numpy(), env.done.cpu().numpy()
    p, a = par.cpu().numpy(), act.cpu().numpy()
    J = env.jobs_per_env[p]
    inside = (a >= 0) & (a <= J)
    m = np.zeros(p.size, bool)
    m[inside] = mask[p[inside], a[inside]] != 0
    return (done[p] == 0) & ((a == -1) | m)


def fork_bytes(f):
    n = f._arena.numel() * f._arena.element_size() + f.solution.numel() * 4
    if f._table_kind() == "own":
        n += sum(x.numel() * x.element_size() for x in (f._ops, f._rem, f._inst))
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--only", default="abc")
    args = ap.parse_args()
    W, WU, KC = args.windows, args.warmup, args.calls
    print(f"# {torch.cuda.get_device_name(0)}; median of {W} windows x {KC} calls, warm-up {WU}; HIP events; kind SPT, seed 7")
    for case in args.only:
        name, env, par, act = build(case)
        ok = torch.tensor(legal_of(env, par, act), device="cuda:0")
        lp, la = par[ok], act[ok]                                  # the legal candidates: what a fork-based caller would clone
        n_iter = 3 * env.jmax * env.mmax
        # scores: lookahead on the legal list vs fork + step + rollout on the same list, same seeds
        ms = env.lookahead("SPT", actions=la, parents=lp, seed=7)[0]
        f = env.fork(lp)
        f.step(la)
        f.rollout("SPT", n_iter=n_iter, seed=7, autoreset=False)
        torch.cuda.synchronize()
        assert bool(f.done.all()) and torch.equal(ms, f.makespan), name
        fb = fork_bytes(f)
        del f
        t_look = time_events(lambda: env.lookahead("SPT", actions=la, parents=lp, seed=7), W, WU, KC)

        def by_fork():
            g = env.fork(lp)
            g.step(la)
            g.rollout("SPT", n_iter=n_iter, seed=7, autoreset=False)
            return g
        t_fork = time_events(by_fork, W, WU, KC)
        n = int(lp.numel())
        print(f"{name}: {n} legal candidates of {int(par.numel())}; fork bytes {fb / n:.0f} B/candidate, "
              f"{fb / 1e6:.1f} MB avoided (from shapes)")
        print(f"    scores   lookahead {t_look:10.1f} us    fork + step + rollout {t_fork:10.1f} us    ({t_fork / t_look:.2f} x)")
        # a whole pilot step: pilot_step vs the same step built from a fork, each on a fresh copy of the batch
        work = {}

        def fresh():
            work["e"] = env.fork(torch.arange(env.batch, device="cuda:0"))

        def pilot():
            work["e"].pilot_step("SPT", seed=7)

        def pilot_by_fork():
            e = work["e"]
            A = e.jmax + 1
            cand = (e.action_mask != 0).nonzero()                  # legal (env, action) pairs, parent-major
            g = e.fork(cand[:, 0])
            g.step(cand[:, 1])
            g.rollout("SPT", n_iter=n_iter, seed=7, autoreset=False)
            score = torch.full((e.batch * A,), 0x7FFFFFFF, dtype=torch.int32, device="cuda:0")
            score[cand[:, 0] * A + cand[:, 1]] = torch.where(g.done != 0, g.makespan, torch.full_like(g.makespan, 0x7FFFFFFF))
            score = score.view(e.batch, A)
            none = (score == 0x7FFFFFFF).all(1)
            e.step(torch.where(none, torch.full_like(none, -1, dtype=torch.int64), score.argmin(1)))
        # the two forms take the same actions
        fresh()
        pilot()
        a_look = work["e"].env_header.clone()
        fresh()
        pilot_by_fork()
        assert torch.equal(a_look, work["e"].env_header), name
        t_pilot = time_events(pilot, W, WU, KC, prepare=fresh)
        t_pilot_fork = time_events(pilot_by_fork, W, WU, KC, prepare=fresh)
        print(f"    pilot    pilot_step {t_pilot:9.1f} us    fork-built step {t_pilot_fork:17.1f} us    "
              f"({t_pilot_fork / t_pilot:.2f} x)")
        sys.stdout.flush()
        del env, work
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
