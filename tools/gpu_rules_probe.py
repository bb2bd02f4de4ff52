"""What the caller-weighted selector (jss_rule_*, include/jss_rules.h) costs (GPU box).  One case per process (--only):

  a  ta01 x 65 536, shared table            whole episodes: jss_rollout(SPT) against jss_rule_rollout with the SPT row -- one
  b  ta41 x 16 384, shared table            shared row, and one row per env -- from the same reset.  The two calls launch the
  c  synthetic 50 x 20 per env x 8 192      same kRollout kernel, so the ratio is the selector's cost.  Makespans must agree.
  l  ta01, 4 096 parents mid-episode x every action: jss_lookahead(SPT) against jss_rule_lookahead with the SPT row
  e  evaluate_weights of 65 536 random rows on ta01 (wall clock of the whole call, and of its rollout alone) against the same
     population played by the facade loop -- WeightedRule.__call__ + JssEnv.step at B = 1 --, extrapolated from 8 rows

Device times are HIP events: warm-up, then the median of --windows windows of one call each; the reset in front of every
rollout is not timed.  With JSSENV_AMD_LIB naming a library older than include/jss_rules.h the stock calls alone are timed
(the parent's kRollout / kLookahead kernels against this tree's, which carry the branch).

usage: python tools/gpu_rules_probe.py --only a|b|c|l|e [--windows N] [--warmup W]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from jssenv_amd import BatchedJssEnv, make  # noqa: E402
from jssenv_amd.dispatching import RULE_WEIGHTS, WeightedRule, evaluate_weights  # noqa: E402
from jssenv_amd.instances import synthetic_packed  # noqa: E402

DEV = "cuda:0"


def time_events(call, windows, warmup, prepare=None):
    """median over windows of the device time of one call (us); `prepare` runs untimed before every call"""
    out = []
    for i in range(warmup + windows):
        if prepare:
            prepare()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(out)


def has_rules(env):
    return hasattr(env.backend.lib, "jss_rule_rollout")


def rollout_case(name, env, args):
    n_iter = 3 * env.jmax * env.mmax
    row = torch.from_numpy(RULE_WEIGHTS["SPT"]).to(DEV)
    rows = row.repeat(env.batch, 1).contiguous()
    res = {"case": name, "batch": env.batch}
    forms = [("stock", lambda: env.rollout("SPT", n_iter=n_iter, autoreset=False))]
    if has_rules(env):
        forms += [("shared_row", lambda: env.rollout("weighted", n_iter=n_iter, autoreset=False, weights=row)),
                  ("row_per_env", lambda: env.rollout("weighted", n_iter=n_iter, autoreset=False, weights=rows))]
    makespans = {}
    for form, call in forms:
        res[form + "_us"] = round(time_events(call, args.windows, args.warmup, prepare=env.reset), 1)
        assert bool(env.done.all()), form
        makespans[form] = env.makespan.clone()
    for form in makespans:
        assert torch.equal(makespans[form], makespans["stock"]), form
        if form != "stock":
            res[form + "_over_stock"] = round(res[form + "_us"] / res["stock_us"], 3)
    res["mean_makespan"] = round(float(makespans["stock"].float().mean()), 1)
    return res


def lookahead_case(args):
    env = BatchedJssEnv("ta01", batch=4096, device=DEV, seed=1)
    env.reset()
    env.rollout("random", n_iter=60, autoreset=False, seed=2)
    row = torch.from_numpy(RULE_WEIGHTS["SPT"]).to(DEV)
    res = {"case": "l ta01 4096 parents x 16 actions", "batch": env.batch}
    res["stock_us"] = round(time_events(lambda: env.lookahead("SPT"), args.windows, args.warmup), 1)
    if has_rules(env):
        res["shared_row_us"] = round(time_events(lambda: env.lookahead("weighted", weights=row), args.windows, args.warmup), 1)
        assert torch.equal(env.lookahead("SPT")[0], env.lookahead("weighted", weights=row)[0])
        res["shared_row_over_stock"] = round(res["shared_row_us"] / res["stock_us"], 3)
    return res


def population_case(args, P=65536, sample=8):
    w = np.random.default_rng(1).integers(-8, 9, size=(P, 8)).astype(np.int32)
    w[:, 7] = np.where(np.arange(P) % 2 == 0, w[:, 7] * 20, -2**31)
    evaluate_weights("ta01", w[:256], device=DEV)                          # warm-up: library, allocator
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ms = evaluate_weights("ta01", w, device=DEV)
        walls.append(time.perf_counter() - t0)
    env = BatchedJssEnv("ta01", batch=P, device=DEV)
    rows = torch.from_numpy(w).to(DEV)
    n_iter = 3 * env.jmax * env.mmax
    dev_us = time_events(lambda: env.rollout("weighted", n_iter=n_iter, autoreset=False, weights=rows), args.windows, args.warmup,
                         prepare=env.reset)
    one = make("jss-v1", env_config={"instance_path": "ta01"}, device=DEV)
    t0 = time.perf_counter()
    for i in range(sample):
        rule = WeightedRule(w[i])
        one.reset()
        done = False
        while not done:
            _, _, done, _, _ = one.step(rule(one))
        assert one.current_time_step == ms[i, 0], i                        # the host mirror plays what the device played
    loop = (time.perf_counter() - t0) / sample
    wall = statistics.median(walls)
    return {"case": f"e evaluate_weights, {P} rows on ta01", "evaluate_weights_wall_ms": round(wall * 1e3, 1),
            "rollout_device_ms": round(dev_us / 1e3, 2), "facade_loop_s_per_row": round(loop, 3),
            "facade_loop_extrapolated_s": round(loop * P, 0), "facade_over_evaluate_weights": round(loop * P / wall, 0),
            "best_makespan": int(ms.min()), "mean_makespan": round(float(ms.mean()), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", required=True, choices=["a", "b", "c", "l", "e"])
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if args.only == "a":
        res = rollout_case("a ta01 x 65536", BatchedJssEnv("ta01", batch=65536, device=DEV), args)
    elif args.only == "b":
        res = rollout_case("b ta41 x 16384", BatchedJssEnv("ta41", batch=16384, device=DEV), args)
    elif args.only == "c":
        res = rollout_case("c 50x20 per env x 8192", BatchedJssEnv(synthetic_packed(8192, 50, 20), batch=8192, device=DEV, records="medium"), args)
    elif args.only == "l":
        res = lookahead_case(args)
    else:
        res = population_case(args)
    res["library"] = os.path.basename(os.environ.get("JSSENV_AMD_LIB", "libjss_hip.so"))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
