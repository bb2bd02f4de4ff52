"""Instances generated on the device (jss_generate), what they cost (GPU box):

  (a) full generation    BatchedJssEnv.generate() of every env of a generated batch (one jss_generate launch, derived seeds)
                         against the host path it replaces: synthetic_packed(n, J, M) on the host + the upload of its three
                         tables (wall clock, one run)
  (b) per step           step(policy("random"), autoreset=True) and step_logits(logits, autoreset=True) on 65 536 generated
                         15 x 15 envs, fresh=False (the instances stay) against fresh=True (a jss_generate launch with
                         which = done in front of every step)
  (c) sparse generate    generate(which) alone with about 1 env in 225 flagged (what a fresh step adds)

Device times are HIP events on the launch stream: warm-up, then windows of K calls each bracketed by torch.cuda.synchronize(),
median window.

usage: python tools/gpu_generate_probe.py [--windows N] [--warmup W]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from jssenv_amd import BatchedJssEnv  # noqa: E402
from jssenv_amd.instances import synthetic_packed  # noqa: E402

K = 20
FULL = ((65536, 15, 15), (8192, 50, 20), (4096, 100, 20))


def time_events(call, windows, warmup):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ev = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(K):
            call()
        e1.record()
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1) / K * 1e3)
    return statistics.median(ev)


def host_path(n, J, M, dev):
    t0 = time.perf_counter()
    pk = synthetic_packed(n, J, M)
    t1 = time.perf_counter()
    tabs = [torch.from_numpy(a).to(dev) for a in (pk.ops, pk.rem, pk.inst)]
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    del tabs
    return (t1 - t0) * 1e6, (t2 - t1) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"# {torch.cuda.get_device_name(dev)}; K = {K} calls per window, {args.windows} windows, warm-up {args.warmup}; "
          "median window, HIP events", flush=True)

    print("# (a) full generation: every env of the batch", flush=True)
    for n, J, M in FULL:
        env = BatchedJssEnv.generated(J, M, n, device=dev, fresh=False)
        us = time_events(env.generate, args.windows, args.warmup)
        gen_host, upload = host_path(n, J, M, dev)
        print(f"{n:6d} x {J:3d}x{M:<3d} jss_generate {us:10.1f} us ({us * 1e3 / n:7.1f} ns per env)   host synthetic_packed "
              f"{gen_host / 1e3:9.1f} ms + upload {upload / 1e3:6.2f} ms  ({(gen_host + upload) / us:7.0f} x)", flush=True)
        del env
        torch.cuda.empty_cache()

    print("# (b) one batch step, 65536 generated 15x15 envs, episodes staggered (env i starts after a random 0..225 skipped "
          "steps), so that about 1 env in 225 finishes per step", flush=True)
    res = {}
    for fresh in (False, True):
        env = BatchedJssEnv.generated(15, 15, 65536, device=dev, fresh=fresh, seed=1)
        env.reset()
        g = torch.Generator(device=dev).manual_seed(1)
        logits = torch.randn(env.batch, env.jmax + 1, generator=g, device=dev) * 2
        phase = torch.randint(0, 226, (env.batch,), generator=torch.Generator().manual_seed(2)).to(dev)
        skip = torch.full((env.batch,), -1, dtype=torch.int32, device=dev)
        for t in range(226):
            env.step(torch.where(phase > t, skip, env.policy("random")), autoreset=True)
        for _ in range(300):
            env.step_logits(logits, autoreset=True)
        torch.cuda.synchronize()
        for name, call in (("policy + step(autoreset=True)", lambda: env.step(env.policy("random"), autoreset=True)),
                           ("step_logits(autoreset=True)", lambda: env.step_logits(logits, autoreset=True))):
            ep0 = env.stats()["episodes"]
            res[(name, fresh)] = time_events(call, args.windows, args.warmup)
            per = (env.stats()["episodes"] - ep0) / (args.warmup + args.windows * K)
            print(f"fresh={str(fresh):5s} {name:32s} {res[(name, fresh)]:8.2f} us  ({per:.0f} envs finish per step)", flush=True)
        if fresh:
            print("# (c) generate(which) alone, ~1 env in 225 flagged", flush=True)
            rng = np.random.default_rng(0)
            which = torch.from_numpy((rng.random(env.batch) < 1 / 225).astype(np.uint8)).to(dev)
            us = time_events(lambda: env.generate(which), args.windows, args.warmup)
            print(f"generate(which) {int(which.sum())} of {env.batch} envs {us:8.2f} us", flush=True)
            none = torch.zeros_like(which)
            us0 = time_events(lambda: env.generate(none), args.windows, args.warmup)
            print(f"generate(which) 0 of {env.batch} envs {us0:8.2f} us  (the flag sweep and the launch)", flush=True)
        del env, logits
        torch.cuda.empty_cache()
    for name in ("policy + step(autoreset=True)", "step_logits(autoreset=True)"):
        a, b = res[(name, False)], res[(name, True)]
        print(f"{name:32s} fresh=True adds {b - a:6.2f} us per step ({b / a:5.3f} x)", flush=True)


if __name__ == "__main__":
    main()
