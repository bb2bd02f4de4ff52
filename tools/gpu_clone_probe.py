"""Env states cloned on the device (jss_clone), what it costs (GPU box):

  (a) ta01, compact records, 65 536 envs: a fan-out (1 024 parents x 64 children) and a random permutation between two
      batches of 65 536
  (b) synthetic 50 x 20, medium records, one table per env, 8 192 envs (permutation, the tables copied too)
  (c) generated 100 x 20, 8 192 envs (permutation, the tables copied too)
  (d) the facade's copy.deepcopy (wall clock)

Each of (a)-(c) times the one-launch jss_clone (through the C ABI, structs bound once) against the obvious alternative: one
torch.index_select(..., out=) per copied tensor.  Bytes per cloned env are read + write of every copied row, from the shapes;
"of 8 TB/s" is that traffic over the device time.  Device times are HIP events on the launch stream: warm-up, then windows
of K calls each bracketed by torch.cuda.synchronize(), median window.

usage: python tools/gpu_clone_probe.py [--windows N] [--warmup W]"""
import argparse
import copy
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from jssenv_amd import BatchedJssEnv, _abi, make  # noqa: E402
from jssenv_amd.instances import synthetic_packed  # noqa: E402

K = 20
PEAK = 8e12


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


def copied(env):
    """(name, tensor) of every tensor a clone copies, as jss_clone copies them"""
    names = ["env_header", "env_const", "job_state"] + ([] if env.no_clocks else ["machine_state"]) + \
            ["solution", "real_obs", "action_mask", "reward", "done", "makespan"]
    out = [(n, getattr(env, n)) for n in names]
    if env._table_of_env is not None:
        out.append(("table_of_env", env._table_of_env))
    elif env._table_kind() == "own":
        out += [("ops", env._ops), ("rem", env._rem), ("inst", env._inst)]
    return out


def bytes_per_env(env):
    return 2 * sum(int(t[0].numel()) * t.element_size() for _, t in copied(env))


def case(label, dst, src, index, windows, warmup):
    be = dst.backend
    idx32 = torch.as_tensor(index, dtype=torch.int32, device=be.device)
    idx64 = idx32.long()
    p = be.ptr
    dt = _abi.JssCloneDst(p(dst._table_of_env), p(dst._ops), p(dst._rem), p(dst._inst))
    args = (C.byref(dst._desc), C.byref(dst._state), C.byref(dst._out), C.byref(dt), C.byref(src._desc),
            C.byref(src._state), C.byref(src._out), p(idx32))
    lib = be.lib

    def clone():
        rc = lib.jss_clone(*args, be.stream())
        assert rc == 0, rc

    pairs = [(d, s) for (_, d), (_, s) in zip(copied(dst), copied(src))]

    def gather():
        for d, s in pairs:
            torch.index_select(s, 0, idx64, out=d)

    # the two give the same bytes (but for the table word of per-env tables, which only the clone rewrites)
    clone()
    torch.cuda.synchronize()
    a = {n: t.clone() for n, t in copied(dst)}
    gather()
    torch.cuda.synchronize()
    for n, t in copied(dst):
        x, y = a[n], t
        if n == "env_const" and dst._table_kind() == "own":
            keep = [c for c in range(_abi.NC) if c != _abi.C_TABLE]
            x, y = x[:, keep], y[:, keep]
        assert torch.equal(x, y), n
    t_clone = time_events(clone, windows, warmup)
    t_gather = time_events(gather, windows, warmup)
    nb = bytes_per_env(dst)
    total = nb * dst.batch
    print(f"{label:44s} {nb:6d} B/env  {total / 1e6:7.1f} MB  jss_clone {t_clone:8.2f} us ({total / (t_clone * 1e-6) / PEAK:5.1%} of 8 TB/s)"
          f"   {len(pairs):2d} x index_select {t_gather:8.2f} us  ({t_gather / t_clone:4.2f} x)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    dev = "cuda:0"
    rng = np.random.default_rng(0)
    print(f"python tools/gpu_clone_probe.py (MI355X, one run)\n# {torch.cuda.get_device_name(0)}; K = {K} calls per window, "
          f"{a.windows} windows, warm-up {a.warmup}; median window, HIP events")
    # (a) ta01 compact
    parents = BatchedJssEnv("ta01", batch=1024, device=dev, seed=1)
    parents.reset()
    parents.rollout("random", n_iter=60, autoreset=False)
    fan = np.repeat(np.arange(1024), 64)
    kids = parents.fork(fan)
    case("ta01 compact 65536: fan-out from 1024", kids, parents, fan, a.windows, a.warmup)
    big = BatchedJssEnv("ta01", batch=65536, device=dev, seed=2)
    big.reset()
    big.rollout("random", n_iter=60, autoreset=False)
    perm = rng.permutation(65536)
    other = big.fork(np.arange(65536))
    case("ta01 compact 65536: permutation", other, big, perm, a.windows, a.warmup)
    del parents, kids, big, other
    # (b) synthetic 50 x 20, medium records, one table per env
    syn = BatchedJssEnv(synthetic_packed(8192, 50, 20), device=dev, seed=3)
    assert syn.medium and syn._table_kind() == "own"
    syn.reset()
    syn.rollout("random", n_iter=200, autoreset=False)
    perm = rng.permutation(8192)
    syn2 = syn.fork(np.arange(8192))
    case("50x20 medium 8192: permutation (+ tables)", syn2, syn, perm, a.windows, a.warmup)
    del syn, syn2
    # (c) generated 100 x 20
    gen = BatchedJssEnv.generated(100, 20, 8192, device=dev, seed=4)
    gen.reset()
    gen.rollout("random", n_iter=300, autoreset=False)
    perm = rng.permutation(8192)
    gen2 = gen.fork(np.arange(8192))
    case(f"generated 100x20 {'medium' if gen.medium else 'full'} 8192: permutation (+ tables)", gen2, gen, perm,
         a.windows, a.warmup)
    del gen, gen2
    # (d) facade deepcopy
    env = make("jss-v1", env_config={"instance_path": "ta01"}, device=dev)
    env.reset()
    for _ in range(100):
        env.step(int(np.flatnonzero(env.legal_actions)[0]))
    ts = []
    for _ in range(30):
        t0 = time.perf_counter()
        c = copy.deepcopy(env)
        c.close()
        ts.append((time.perf_counter() - t0) * 1e6)
        del c
    print(f"facade copy.deepcopy (ta01, mid-episode, host arena)   median {statistics.median(ts[5:]):8.1f} us  "
          f"(constructor + clone + the copy's close; {len(ts) - 5} runs)")


if __name__ == "__main__":
    main()
