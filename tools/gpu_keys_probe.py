"""What the per-operation key selector (jss_key_*, include/jss_keys.h) costs (GPU box).  One case per process (--only):

  a  ta01 x 65 536, shared table            whole episodes: jss_rollout(SPT) against jss_key_rollout with the SPT table -- one
  b  ta41 x 16 384, shared table            shared table, and one table per env -- and against jss_rule_rollout with the SPT row,
  c  synthetic 50 x 20 per env x 8 192      from the same reset.  All launch the same kRollout kernel, so a ratio is a selector's
                                            cost.  Makespans must agree.
  l  ta01, 4 096 parents mid-episode x every action: jss_lookahead(SPT) against jss_key_lookahead with the SPT table
  e  evaluate_keys of 65 536 random tables on ta01 (wall clock of the whole call, and device time of its rollout alone) against
     the same population played with one step() launch per decision -- jss_step with a torch gather and arg-max over the key
     tables in between, the form without jss_key_* --, extrapolated from --loop-steps decisions

Device times are HIP events: warm-up, then the median of --windows windows of one call each; the reset in front of every
rollout is not timed.  With JSSENV_AMD_LIB naming a library older than include/jss_keys.h the stock calls alone are timed (the
parent's kRollout / kLookahead kernels against this tree's, which carry the branch).

usage: python tools/gpu_keys_probe.py --only a|b|c|l|e [--windows N] [--warmup W]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from jssenv_amd import BatchedJssEnv  # noqa: E402
from jssenv_amd.dispatching import RULE_WEIGHTS  # noqa: E402
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


def has_keys(env):
    return hasattr(env.backend.lib, "jss_key_rollout")


def spt_tables(env):
    """(B, jmax, mmax) int32 on the device: -duration of every op of every env's instance, from the batch's own op tables"""
    ops = env.backend.torch.as_tensor(env.packed.ops, device=DEV).to(torch.int32)          # (n_tables, jmax, mmax) machine << 16 | duration
    neg = -(ops & 0xFFFF)
    if neg.shape[0] == 1:
        return neg[0].contiguous(), neg.expand(env.batch, -1, -1).contiguous()
    toe = torch.as_tensor(np.asarray(env.table_of_env_host), device=DEV).long()
    return None, neg[toe].contiguous()


def rollout_case(name, env, args):
    n_iter = 3 * env.jmax * env.mmax
    res = {"case": name, "batch": env.batch}
    forms = [("stock", lambda: env.rollout("SPT", n_iter=n_iter, autoreset=False))]
    if has_keys(env):
        shared, per_env = spt_tables(env)
        row = torch.from_numpy(RULE_WEIGHTS["SPT"]).to(DEV)
        if shared is not None:
            forms.append(("shared_table", lambda: env.rollout("keys", n_iter=n_iter, autoreset=False, keys=shared)))
        forms += [("table_per_env", lambda: env.rollout("keys", n_iter=n_iter, autoreset=False, keys=per_env)),
                  ("weighted_row", lambda: env.rollout("weighted", n_iter=n_iter, autoreset=False, weights=row))]
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
    res = {"case": "l ta01 4096 parents x 16 actions", "batch": env.batch}
    res["stock_us"] = round(time_events(lambda: env.lookahead("SPT"), args.windows, args.warmup), 1)
    if has_keys(env):
        shared, per_env = spt_tables(env)
        for form, t in (("shared_table", shared), ("table_per_env", per_env)):
            res[form + "_us"] = round(time_events(lambda: env.lookahead("keys", keys=t), args.windows, args.warmup), 1)
            assert torch.equal(env.lookahead("SPT")[0], env.lookahead("keys", keys=t)[0]), form
            res[form + "_over_stock"] = round(res[form + "_us"] / res["stock_us"], 3)
    return res


def population_case(args, P=65536):
    from jssenv_amd.dispatching import evaluate_keys
    pop = np.random.default_rng(1).integers(-2**31, 2**31, size=(P, 15, 15), dtype=np.int64).astype(np.int32)
    evaluate_keys("ta01", pop[:256], device=DEV)                          # warm-up: library, allocator
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ms = evaluate_keys("ta01", pop, device=DEV)
        walls.append(time.perf_counter() - t0)
    env = BatchedJssEnv("ta01", batch=P, device=DEV)
    tables = torch.from_numpy(pop).to(DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    on_device = evaluate_keys("ta01", tables, device=DEV)
    wall_device_tensor = time.perf_counter() - t0
    assert np.array_equal(on_device, ms)
    n_iter = 3 * env.jmax * env.mmax
    dev_us = time_events(lambda: env.rollout("keys", n_iter=n_iter, autoreset=False, keys=tables), args.windows, args.warmup,
                         prepare=env.reset)
    assert np.array_equal(env.makespan.cpu().numpy(), ms)
    # the form without jss_key_*: per decision one gather of every job's current key, a masked arg-max, one jss_step launch
    def decide_and_step(env, tables):
        J = env.jmax
        todo = (env.job_state[:, :, 0] & _todo_mask(env)).long().clamp(max=env.mmax - 1)
        key = tables.gather(2, todo.unsqueeze(2)).squeeze(2).long()
        mask = env.action_mask[:, :J].bool()
        a = torch.where(mask, key, torch.full_like(key, -2**31 - 1)).argmax(dim=1)   # (the first maximum: the lowest index)
        nope = torch.where(env.action_mask[:, J].bool(), J, -1)
        env.step(torch.where(mask.any(dim=1), a, nope).to(torch.int32))
    small = BatchedJssEnv("ta01", batch=256, device=DEV)                  # ... played to the end once: it decodes what the device decodes
    small.reset()
    while not bool(small.done.all()):
        decide_and_step(small, tables[:256])
    assert np.array_equal(small.makespan.cpu().numpy(), ms[:256])
    env.reset()
    for _ in range(5):
        decide_and_step(env, tables)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.loop_steps):
        decide_and_step(env, tables)
    torch.cuda.synchronize()
    per_step = (time.perf_counter() - t0) / args.loop_steps
    env.reset()
    env.zero_counters()
    env.rollout("keys", n_iter=n_iter, autoreset=False, keys=tables)
    decisions = int(env.counters[:, 0].max())                            # the loop runs until the slowest env is done
    wall = statistics.median(walls)
    return {"case": f"e evaluate_keys, {P} tables on ta01", "evaluate_keys_wall_ms": round(wall * 1e3, 1),
            "evaluate_keys_wall_ms_device_tensor": round(wall_device_tensor * 1e3, 1), "rollout_device_ms": round(dev_us / 1e3, 2),
            "step_loop_us_per_decision": round(per_step * 1e6, 1), "decisions_of_the_longest_episode": decisions,
            "step_loop_extrapolated_ms": round(per_step * decisions * 1e3, 1),
            "step_loop_over_rollout": round(per_step * decisions / (dev_us * 1e-6), 1),
            "best_makespan": int(ms.min()), "mean_makespan": round(float(ms.mean()), 1)}


def _todo_mask(env):
    from jssenv_amd import _abi
    return {_abi.NFC: _abi.FC_TODO_MASK, _abi.NFM: _abi.FM_TODO_MASK, _abi.NF: _abi.TODO_MASK}[int(env.job_state.shape[2])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", required=True, choices=["a", "b", "c", "l", "e"])
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-steps", type=int, default=40)
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
