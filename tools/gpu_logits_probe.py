"""The step between a policy network and the env, three ways, microseconds per env-step batch (GPU box):

  (a) step_logits      BatchedJssEnv.step_logits(logits, autoreset=True): the masked Gumbel-max draw, its log-probability and
                       the step in ONE launch (jss_step_logits)
  (b) torch sampler    what a caller writes without it: mask -> masked_fill -> log_softmax -> Gumbel argmax -> gather, then
                       step(actions, autoreset=True)
  (c) fused random     rollout("random", n_iter=1): the on-device random policy + step, the upper bound (no logits to read)

On config 5 (ta01-ta80 x 32 768) two more forms:

  (a') per-range           by shape class: what step_logits issued before the fused grid had kLogits bodies -- one single-set
                           jss_step_logits per range of the batch (below 64 jobs / the rest) on the current + a side stream,
                           driven through the C ABI
  (a) for BucketedJssEnv   BucketedJssEnv.step_logits({class: logits}): one jss_multi_step_logits grid over the classes; (a'')
                           each bucket's own BatchedJssEnv.step_logits one after the other (the loop a learner had to write);
                           (b) the torch sampler per bucket + BucketedJssEnv.step; (c) rollout_steps("random", 1)

The logits are one (B, jmax + 1) float32 tensor made up front (the network's cost is not the env's).  Warm-up, then windows of
K steps each bracketed by torch.cuda.synchronize(), timed by HIP events on the launch stream and by the wall clock; the median
window is reported.  Sizes: the headline (ta01 x 65 536), config 3 (ta41 x 16 384), config 4's share (50x20 x 8 192), config 5
by shape class (ta01-ta80 x 32 768), config 5 bucketed.

usage: python tools/gpu_logits_probe.py [--windows N] [--warmup W] [--only LABEL-SUBSTRING]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HSA_ENABLE_INTERRUPT", "0")
import torch  # noqa: E402

from jssenv_amd import BatchedJssEnv, _abi, builtin_instance  # noqa: E402
from jssenv_amd.bucketed import BucketedJssEnv  # noqa: E402
from jssenv_amd.instances import synthetic_packed  # noqa: E402

K = 20
SIZES = (("headline ta01 x 65536", lambda: dict(instances=builtin_instance("ta01"), batch=65536)),
         ("config 3 ta41 x 16384", lambda: dict(instances=builtin_instance("ta41"), batch=16384)),
         ("config 4 share syn50x20 x 8192", lambda: dict(instances=synthetic_packed(8192, 50, 20), batch=8192)),
         ("config 5 by shape ta01-80 x 32768", lambda: dict(instances=[builtin_instance(f"ta{k:02d}") for k in range(1, 81)],
                                                            batch=32768, order="by_shape")),
         ("config 5 bucketed ta01-80 x 32768", lambda: dict(instances=[builtin_instance(f"ta{k:02d}") for k in range(1, 81)],
                                                            batch=32768, bucketed=True)))


def torch_sampler(env, logits, gen, T=1.0):
    """the caller's sampler: masked log_softmax, Gumbel-max, log-probability of the draw"""
    mask = env.action_mask.bool()
    masked = logits.masked_fill(~mask, float("-inf"))
    lsm = torch.log_softmax(masked / T, dim=1)
    u = torch.rand(logits.shape, generator=gen, device=logits.device)
    a = torch.argmax(lsm - torch.log(-torch.log(u)), dim=1)
    logp = lsm.gather(1, a[:, None])[:, 0]
    return a.to(torch.int32), logp


def per_range_step_logits(env, logits):
    """step_logits(logits, autoreset=True) on a by-shape batch the way it was issued before jss_multi_step_logits: one
    jss_step_logits per range of env._ranges(), several ranges on the current stream + side streams forked from it"""
    arg = env._logits_arg(logits)
    keep = []

    def call(d, s, o, first, stream):
        keep.append(env._logits_struct(arg, 1.0, True, False, first))
        return env.lib.jss_step_logits(d, s, C.byref(keep[-1]), env.seed, _abi.ROLLOUT_AUTORESET, o, stream)
    env._over_ranges(call, "jss_step_logits")


def forms(env, logits, gen):
    """[(name, one step)] of the size"""
    if isinstance(env, BucketedJssEnv):
        each = env._each()
        per = {k: logits[torch.as_tensor(env.members[k], device=logits.device)][:, :b.jmax + 1].contiguous() for k, b in each}

        def bucket_loop():
            for k, b in each:
                b.step_logits(per[k], autoreset=True)

        def sampler_step():
            env.step({k: torch_sampler(b, per[k], gen)[0] for k, b in each}, autoreset=True)
        return [("(a) step_logits", lambda: env.step_logits(per, autoreset=True)),
                ("(a'') per-bucket step_logits", bucket_loop),
                ("(b) torch sampler + step", sampler_step),
                ("(c) fused random rollout", lambda: env.rollout_steps("random", steps=1, autoreset=True))]

    def sampler_step():
        a, _ = torch_sampler(env, logits, gen)
        env.step(a, autoreset=True)
    out = [("(a) step_logits", lambda: env.step_logits(logits, autoreset=True))]
    if env.steps_by_shape_class:
        out.append(("(a') per-range jss_step_logits", lambda: per_range_step_logits(env, logits)))
    return out + [("(b) torch sampler + step", sampler_step),
                  ("(c) fused random rollout", lambda: env.rollout("random", n_iter=1, autoreset=True))]


def time_form(step, windows, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(K):
            step()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) / K * 1e6)
        ev.append(e0.elapsed_time(e1) / K * 1e3)
    return statistics.median(ev), statistics.median(wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"# {torch.cuda.get_device_name(dev)}; K = {K} steps per window, {args.windows} windows, warm-up {args.warmup}; "
          f"median window, us per batch step (HIP events / wall)", flush=True)
    for label, kw in SIZES:
        if args.only and args.only not in label:
            continue
        kw = kw()
        if kw.pop("bucketed", False):
            env = BucketedJssEnv(kw["instances"], batch=kw["batch"], device=dev, seed=0)
        else:
            env = BatchedJssEnv(device=dev, seed=0, **kw)
        env.reset()
        env.rollout("random", n_iter=100)
        gen = torch.Generator(device=dev).manual_seed(1)
        logits = torch.randn(env.batch, env.jmax + 1, generator=gen, device=dev) * 2
        res = {}
        for name, fn in forms(env, logits, gen):
            res[name] = time_form(fn, args.windows, args.warmup)
        a_ev = res["(a) step_logits"][0]
        for name, (ev, wall) in res.items():
            print(f"{label:36s} {name:31s} events {ev:8.2f} us  wall {wall:8.2f} us  ({ev / a_ev:5.2f} x (a))", flush=True)
        del env, logits
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
