"""Backend-agnostic cases of jss_order_eval / jss_order_apply (include/jss_order.h), BatchedJssEnv.evaluate_order and
search.improve, run against the host-core twin, the kernel source (jssenv_amd/csrc/jss_order.hip) under the SIMT emulator and
the HIP library libjss_order_hip.so.

The reference is search.order_eval_reference (NumPy, written from the header's definition).  A case's batch, rank tensor and
candidate list are made once, on the twin, and its reference once; another backend builds the same batch (only env_const and
the instance tables are read, which a reset writes identically everywhere) and is compared with that reference bit for bit."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

from clone_cases import rows_of
from jssenv_amd import BatchedJssEnv, _abi, search
from jssenv_amd import instances as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
ORDER_SRC = os.path.join(ROOT, "jssenv_amd", "csrc", "jss_order.hip")
EMU_LIB = os.path.join(EMU, "libjss_order_emu.so")
FILL = -77777                       # what the optional outputs hold before a call: rows of refused and cyclic candidates keep it
# instance, rule -> makespan before, after, improving iterations, neighbours evaluated (steepest descent, B = 1, pair_cap 128)
ANCHORS = {("ta01", "SPT"): (1462, 1400, 7, 144), ("ta01", "FIFO"): (1486, 1455, 2, 35), ("ta41", "SPT"): (2499, 2406, 6, 279)}


def build_emu_order():
    """jss_order.hip, unmodified, compiled with g++ against the SIMT emulator's hip_runtime.h: a library of its own"""
    deps = [ORDER_SRC, os.path.join(EMU, "hip", "hip_runtime.h"), os.path.join(ROOT, "include", "jss_order.h"),
            os.path.join(ROOT, "jssenv_amd", "csrc", "jss_abi_checks.hpp")]
    if not os.path.isfile(EMU_LIB) or any(os.path.getmtime(d) > os.path.getmtime(EMU_LIB) for d in deps):
        tmp = EMU_LIB + f".tmp{os.getpid()}"
        subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
                               "-Wno-unknown-pragmas", "-I" + EMU, "-I" + os.path.join(ROOT, "include"), ORDER_SRC, "-o", tmp])
        os.replace(tmp, EMU_LIB)
    return EMU_LIB


def emu_backend():
    """the emulator backend of the env kernels, with the emulated order library attached as its `order_lib`"""
    sys.path.insert(0, EMU)
    from emu_backend import EmuBackend
    be = EmuBackend(default_kernel="auto")
    be.order_lib = _abi.bind_order(C.CDLL(build_emu_order()))
    return be


_TWIN = []


def twin_backend():
    if not _TWIN:
        from jssenv_amd.env import CpuBackend
        _TWIN.append(CpuBackend())
    return _TWIN[0]


# ---- the batches -------------------------------------------------------------------------------------------------------------
def inst(name, machine, duration):
    return I.Instance(name, np.asarray(machine, np.int32), np.asarray(duration, np.int32))


def _wide(jobs, machines, seed):
    return I.taillard_instance(jobs, machines, 1000 + seed, 2000 + seed, name=f"syn{jobs}x{machines}")


def syn50x20():
    return I.taillard_instance(50, 20, 4711, 815, name="syn50x20")


# name -> (constructor on a backend, envs).  The shapes are the smallest at which the kernel takes another path: one job, 3 x 2,
# 15 x 15, 65 jobs (two jobs on lane 0), one 100 x 20 (one wavefront per workgroup), a per-env-table batch, a table_of_env batch,
# a batch dealt out by shape class (rows padded to the largest), machines that repeat within a job with one the instance never
# uses.  The last env of every batch is never reset.
CASES = {
    "1x2": (lambda be: BatchedJssEnv(inst("one", [[1, 0]], [[4, 9]]), batch=3, _backend=be, seed=1), 3),
    "3x2": (lambda be: BatchedJssEnv(inst("three", [[0, 1], [0, 1], [1, 0]], [[2, 3], [4, 1], [5, 2]]), batch=4, _backend=be, seed=2), 4),
    "ta01": (lambda be: BatchedJssEnv("ta01", batch=4, _backend=be, seed=3), 4),
    "J65": (lambda be: BatchedJssEnv(_wide(65, 4, 3), batch=3, _backend=be, seed=5), 3),
    "100x20": (lambda be: BatchedJssEnv("ta71", batch=3, _backend=be, seed=6), 3),
    "per-env": (lambda be: BatchedJssEnv(I.synthetic_packed(5, 7, 6), batch=5, _backend=be, seed=10), 5),
    "table-of-env": (lambda be: BatchedJssEnv(["ta01", "ta02", "ta11"], batch=5, table_of_env=[0, 1, 2, 1, 0], _backend=be, seed=7), 5),
    "by-shape": (lambda be: BatchedJssEnv(["ta01", "ta11", "ta41"], batch=6, order="by_shape", _backend=be, seed=9), 6),
    "repeats": (lambda be: BatchedJssEnv(inst("repeats", [[0, 0, 1, 3], [1, 0, 0, 1], [3, 1, 1, 0]],
                                              [[3, 5, 2, 4], [6, 1, 1, 7], [2, 2, 9, 3]]), batch=4, _backend=be, seed=13), 4),
}
CAPS = (3, 128)                     # pair_cap below the count of most schedules, and above every count
_STATES = {}


def host_tables(env):
    return dict(env_const=np.asarray(env.backend.numpy(env.env_const)), ops=np.array(env.packed.ops, copy=True))


def reference(host, rank, parents=None, swap_a=None, swap_b=None, cap=None, fill=FILL):
    return search.order_eval_reference(host["env_const"], host["ops"], rank, parents, swap_a, swap_b, cap, fill)


def make_env(be, name):
    """the case's batch on `be`: every env but the last reset"""
    make, B = CASES[name]
    env = make(be)
    which = np.ones(B, np.uint8)
    which[B - 1] = 0
    env.reset(which=which)
    return env


def case_state(name):
    """The case's batch on the twin and what is derived from it, made once.  The rank tensor: env 0 the solution of a finished
    random rollout; env 1 the solution of a finished SPT rollout where the batch has that many reset envs; the next one
    operation index * 1000 + a small random number (always a schedule, with ties in rank); the next random small numbers
    (ties, mostly cyclic); the env never reset a finished solution's copy.  The candidate list: every reset env with no swap,
    with swaps from the reference's pairs, with random swaps of two real operations, and what the header refuses."""
    if name in _STATES:
        return _STATES[name]
    B = CASES[name][1]
    be = twin_backend()
    env = make_env(be, name)
    n_iter = 3 * env.jmax * env.mmax + 16
    env.rollout("random", n_iter=n_iter, autoreset=False)
    sol_random = np.asarray(be.numpy(env.solution)).copy()
    spt = make_env(be, name)
    spt.rollout("SPT", n_iter=n_iter, autoreset=False)
    sol_spt = np.asarray(be.numpy(spt.solution)).copy()
    host = host_tables(env)
    rng = np.random.default_rng(len(name) * 7919 + B)
    jmax, mmax, region = env.jmax, env.mmax, env.jmax * env.mmax
    rank = sol_random.copy()
    kinds = ["random rollout", "SPT rollout", "by operation index", "small random"]
    for i in range(B - 1):
        kind = kinds[i % 4]
        if kind == "SPT rollout":
            rank[i] = sol_spt[i]
        elif kind == "by operation index":
            rank[i] = np.arange(mmax)[None, :] * 1000 + rng.integers(0, 3, (jmax, mmax))
        elif kind == "small random":
            rank[i] = rng.integers(0, 4, (jmax, mmax))
    rank[B - 1] = sol_random[0]
    rank = np.ascontiguousarray(rank, np.int32)
    rows = {cap: reference(host, rank, cap=cap) for cap in CAPS}
    J = host["env_const"][:, _abi.C_JOBS]
    M = host["env_const"][:, _abi.C_MACHINES]
    par, sa, sb = [], [], []
    for i in range(B - 1):
        real = [j * mmax + k for j in range(J[i]) for k in range(M[i])]
        par.append(i), sa.append(-1), sb.append(-1)
        found = rows[128][5][i]
        for k in range(max(0, min(int(found), 6))):                   # (a cyclic row has none)
            par.append(i), sa.append(int(rows[128][3][i, k])), sb.append(int(rows[128][4][i, k]))
        for _ in range(3):
            a, b = rng.choice(real, 2)
            par.append(i), sa.append(int(a)), sb.append(int(b))
        par.append(i), sa.append(real[0]), sb.append(real[0])         # a == b: no change
    refused = [(0, 0, -1), (0, -1, 0), (0, region, 0), (0, 0, region), (0, -5, 0), (0, 0, 2 ** 31 - 1), (0, -2 ** 31, 0),
               (-1, -1, -1), (B, -1, -1), (B - 1, -1, -1), (2 ** 31 - 1, 0, 0), (-2 ** 31, 0, 0)]
    pad = [e for e in range(region) if not (e // mmax < J[0] and e % mmax < M[0])]
    if pad:                                                           # a padding entry of env 0's row, as either index
        refused += [(0, pad[0], 0), (0, 0, pad[-1])]
    refused_at = slice(len(par), len(par) + len(refused))
    for p_, a, b in refused:
        par.append(p_), sa.append(a), sb.append(b)
    if len(par) % 4 == 0:
        par.append(0), sa.append(-1), sb.append(-1)
    par, sa, sb = (np.asarray(x, np.int64).astype(np.int32) for x in (par, sa, sb))
    # one more rank tensor: env 0's with a real operation's rank negative (an unfinished env's solution)
    negative = rank.copy()
    negative[0, J[0] - 1, M[0] - 1] = -1
    st = dict(env=env, host=host, rank=rank, rows=rows, par=par, sa=sa, sb=sb, B=B, refused_at=refused_at, negative=negative,
              cands={cap: reference(host, rank, par, sa, sb, cap) for cap in CAPS}, kinds=kinds)
    _STATES[name] = st
    return st


def env_on(be, name):
    st = case_state(name)
    return st["env"] if be is twin_backend() else make_env(be, name)


def call_eval(be, env, rank, parents=None, swap_a=None, swap_b=None, want=("start", "tail", "pairs"), cap=128, n=None):
    """jss_order_eval through the backend's library: (rc, makespan, start, tail, pair_a, pair_b, n_pairs) as host arrays (None
    where not asked for); the outputs are prefilled (FILL), so what a call leaves alone can be told from what it writes"""
    lib = search.order_library(be)
    n = (env.batch if parents is None else len(parents)) if n is None else n
    rows = max(n, 1)
    with be.on_device():
        dev = lambda x: None if x is None else be.from_numpy(np.asarray(x, np.int32))   # noqa: E731
        rk, par, sa, sb = dev(rank), dev(parents), dev(swap_a), dev(swap_b)
        full = lambda shape: be.from_numpy(np.full(shape, FILL, np.int32))   # noqa: E731
        mk = full(rows)
        st = full((rows, env.jmax, env.mmax)) if "start" in want else None
        tl = full((rows, env.jmax, env.mmax)) if "tail" in want else None
        pa, pb, npairs = (full((rows, cap)), full((rows, cap)), full(rows)) if "pairs" in want else (None, None, None)
        p = be.ptr
        arg = _abi.JssOrder(n, cap, p(rk), p(par), p(sa), p(sb), p(mk), p(st), p(tl), p(pa), p(pb), p(npairs))
        rc = lib.jss_order_eval(C.byref(env._desc), C.byref(env._state), C.byref(arg), be.stream())
        be.sync()
    host = lambda x: None if x is None else np.asarray(be.numpy(x))   # noqa: E731
    return (rc,) + tuple(host(x) for x in (mk, st, tl, pa, pb, npairs))


def same(got, ref, what):
    """a call's outputs against the reference's (makespan, start, tail, pair_a, pair_b, n_pairs), those that were asked for"""
    assert got[0] == 0, (what, got[0])
    n = ref[0].size
    assert got[1].dtype == np.int32 and np.array_equal(got[1][:n], ref[0]), (what, "makespan")
    for k, label in ((2, "start"), (3, "tail"), (4, "pair_a"), (5, "pair_b"), (6, "n_pairs")):
        if got[k] is not None:
            assert np.array_equal(got[k][:n], ref[k - 1]), (what, label)


def case_against_mirror(be, name):
    """the rows and the candidate list, at both pair capacities, against the mirror; every combination of the optional
    outputs; a negative rank; n == 0; the batch and the rank tensor untouched"""
    st = case_state(name)
    env = env_on(be, name)
    B, rank, par, sa, sb = st["B"], st["rank"], st["par"], st["sa"], st["sb"]
    before = rows_of(env)
    assert par.size % 4
    for cap in CAPS:
        same(call_eval(be, env, rank, cap=cap), st["rows"][cap], (name, "rows", cap))
        same(call_eval(be, env, rank, par, sa, sb, cap=cap), st["cands"][cap], (name, "candidates", cap))
    ref = st["cands"][128]
    mk = ref[0]
    assert (mk[st["refused_at"]] == -1).all(), (name, mk[st["refused_at"]])
    # refused and cyclic rows keep the fill in every optional output; the others hold none of it
    dead = mk < 0
    for k in (1, 2, 3, 4):
        assert (ref[k][dead] == FILL).all() and not (ref[k][~dead] == FILL).any(), (name, k)
    assert (ref[5][dead] == FILL).all() and (ref[5][~dead] >= 0).all()
    assert mk[0] >= 0 and (mk[~dead] > 0).all()
    # the optional outputs in every combination, on the rows (parent == NULL, no swaps)
    rows = st["rows"][3]
    for mask in range(8):
        want = tuple(w for bit, w in enumerate(("start", "tail", "pairs")) if mask >> bit & 1)
        same(call_eval(be, env, rank, want=want, cap=3), rows, (name, want))
    # swaps given, parent NULL: candidate c is env c
    first = np.array([st["sa"][np.flatnonzero(par == i)[1]] if i < B - 1 else -1 for i in range(B)], np.int32)
    second = np.array([st["sb"][np.flatnonzero(par == i)[1]] if i < B - 1 else -1 for i in range(B)], np.int32)
    same(call_eval(be, env, rank, None, first, second), reference(st["host"], rank, None, first, second, 128), (name, "swaps, no parents"))
    # a real operation with a negative rank: env 0 refused, the others as before
    got = call_eval(be, env, st["negative"], cap=3)
    assert got[1][0] == -1 and (got[2][0] == FILL).all() and np.array_equal(got[1][1:], rows[0][1:])
    # n == 0: nothing runs
    got = call_eval(be, env, rank, par, sa, sb, n=0)
    assert got[0] == 0 and all((x == FILL).all() for x in got[1:])
    after = rows_of(env)
    for k in before:
        assert np.array_equal(before[k], after[k]), (name, k)


def what_the_cases_cover():
    """over all cases the references hold schedules, refusals, cycles, truncated pair lists and lists that fit"""
    seen = dict(ok=0, refused=0, cyclic=0, truncated=0, fits=0, swap_cyclic=0)
    for name in CASES:
        st = case_state(name)
        mk, found = st["cands"][3][0], st["cands"][3][5]
        seen["ok"] += int((mk >= 0).sum())
        seen["refused"] += int((mk == -1).sum())
        seen["cyclic"] += int((st["rows"][3][0] == -2).sum())
        seen["swap_cyclic"] += int(((mk == -2) & (st["rows"][3][0][np.clip(st["par"], 0, st["B"] - 1)] >= 0)).sum())
        seen["truncated"] += int((found[mk >= 0] > 3).sum())
        seen["fits"] += int((found[mk >= 0] <= 3).sum())
    return seen


# ---- the hand cases ----------------------------------------------------------------------------------------------------------------
def hand_arrays():
    """2 x 2 -- J0: (m0, 3), (m1, 2); J1: (m1, 4), (m0, 1) -- with a rank that is a schedule and the cyclic one; 3 x 2 -- J0:
    (m0, 2), (m1, 3); J1: (m0, 4), (m1, 1); J2: (m1, 5), (m0, 2) -- with ties in rank on both machines"""
    const = np.zeros((3, _abi.NC), np.int32)
    const[:, _abi.C_JOBS], const[:, _abi.C_MACHINES], const[:, _abi.C_TABLE] = [2, 2, 3], 2, [0, 0, 1]
    ops = np.zeros((2, 3, 2), np.int32)
    ops[0, :2] = [[0 << 16 | 3, 1 << 16 | 2], [1 << 16 | 4, 0 << 16 | 1]]
    ops[1] = [[0 << 16 | 2, 1 << 16 | 3], [0 << 16 | 4, 1 << 16 | 1], [1 << 16 | 5, 0 << 16 | 2]]
    rank = np.array([[[0, 1], [0, 1], [0, 0]], [[1, 0], [1, 0], [0, 0]], [[0, 5], [0, 5], [0, 5]]], np.int32)
    return const, ops, rank


def check_hand(makespan, start, tail, pair_a, pair_b, n_pairs, fill):
    assert makespan.tolist() == [6, -2, 9]
    assert start[0].tolist() == [[0, 4], [0, 4], [-1, -1]] and tail[0].tolist() == [[2, 0], [2, 0], [-1, -1]]
    assert n_pairs.tolist() == [1, fill, 2]
    assert pair_a[0].tolist() == [2, -1, -1] and pair_b[0].tolist() == [1, -1, -1]       # J1's first op, then J0's second, on m1
    assert (start[1] == fill).all() and (tail[1] == fill).all() and (pair_a[1] == fill).all() and (pair_b[1] == fill).all()
    # the ties (rank 0 on m0, rank 5 on m1) go to the lower job: J0 before J1 on both machines
    assert start[2].tolist() == [[0, 5], [2, 8], [0, 6]] and tail[2].tolist() == [[6, 1], [2, 0], [4, 0]]
    assert pair_a[2].tolist() == [4, 1, -1] and pair_b[2].tolist() == [1, 3, -1]


def case_hand(be):
    """the hand cases through the library: a table_of_env batch of the two instances"""
    two = inst("hand2x2", [[0, 1], [1, 0]], [[3, 2], [4, 1]])
    three = inst("hand3x2", [[0, 1], [0, 1], [1, 0]], [[2, 3], [4, 1], [5, 2]])
    env = BatchedJssEnv([two, three], batch=3, table_of_env=[0, 0, 1], _backend=be)
    env.reset()
    got = call_eval(be, env, hand_arrays()[2], cap=3)
    assert got[0] == 0
    check_hand(*got[1:], FILL)
    # swaps: the one pair of the first rank reversed (J0's second op before J1's first on m1: 0-3-5, then 5-9-10); its two m0
    # operations exchanged; the first pair of the 3 x 2 reversed (J2's first op last on m1); two equal ranks exchanged
    got = call_eval(be, env, hand_arrays()[2], [0, 0, 2, 2], [2, 0, 4, 1], [1, 3, 1, 3], cap=3)
    assert got[1].tolist() == [10, 10, 14, 9]
    assert got[2][0].tolist() == [[0, 3], [5, 9], [-1, -1]]
    assert got[2][2].tolist() == [[0, 2], [2, 6], [7, 12]] and got[2][3].tolist() == [[0, 5], [2, 8], [0, 6]]


# ---- properties of re-timed rollouts ---------------------------------------------------------------------------------------------
def feasible(start, machine, duration):
    """plain NumPy: job order holds and no two operations overlap on a machine; returns the makespan"""
    J, M = machine.shape
    s, d = np.asarray(start)[:J, :M].astype(np.int64), duration.astype(np.int64)
    assert (s >= 0).all() and (s[:, 1:] >= (s + d)[:, :-1]).all()
    for m in np.unique(machine):
        on = machine == m
        order = np.argsort(s[on], kind="stable")
        assert ((s[on][order])[1:] >= ((s + d)[on][order])[:-1]).all(), m
    return int((s + d).max())


def case_properties(be, instance, kind, seed=21):
    """a finished `kind` rollout, re-timed: see the asserts"""
    env = BatchedJssEnv(instance, batch=1, _backend=be, seed=seed)
    env.reset()
    env.rollout(kind, n_iter=3 * env.jmax * env.mmax, autoreset=False)
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    assert n(env.done).all()
    host = host_tables(env)
    J, M = int(host["env_const"][0, _abi.C_JOBS]), int(host["env_const"][0, _abi.C_MACHINES])
    mach, dur = (host["ops"][0, :J, :M] >> 16) & 63, host["ops"][0, :J, :M] & 0xFFFF
    sol = n(env.solution)
    mk, start, tail, pa, pb, found = (n(x) for x in env.evaluate_order(start=True, tail=True, pairs=128))
    ref = reference(host, sol, cap=128, fill=-1)
    for g, r in zip((mk, start, tail, pa, pb, found), ref):
        assert np.array_equal(g, r)
    s, t = start[0, :J, :M].astype(np.int64), tail[0, :J, :M].astype(np.int64)
    assert (s <= sol[0, :J, :M]).all() and 0 < mk[0] <= n(env.makespan)[0]
    assert (start[0, J:] == -1).all() and (start[0, :, M:] == -1).all() and (tail[0, J:] == -1).all() and (tail[0, :, M:] == -1).all()
    assert (s + dur + t <= mk[0]).all() and (t >= 0).all()
    assert feasible(start[0], mach, dur) == mk[0]
    # a chain of critical operations from time 0 to the makespan, each starting as the one before -- of its job or on its
    # machine -- ends: follow it from every critical operation to the end
    critical = s + dur + t == mk[0]
    assert (critical & (s == 0)).any() and (critical & (t == 0)).any()
    behind = {}
    for m in np.unique(mach):
        on = np.argwhere(mach == m)
        on = on[np.lexsort((on[:, 1], on[:, 0], sol[0][on[:, 0], on[:, 1]]))]
        for u, v in zip(on[:-1], on[1:]):
            behind[tuple(u)] = tuple(v)
    for j, k in np.argwhere(critical):
        if t[j, k] == 0:
            continue
        nxt = [(j, k + 1)] if k + 1 < M else []
        nxt += [behind[(j, k)]] if (j, k) in behind else []
        assert any(critical[v] and s[v] == s[j, k] + dur[j, k] for v in nxt), (j, k)
    # the re-timed starts order the machines as before: evaluating them gives them back
    again = env.evaluate_order(start, start=True)
    assert np.array_equal(n(again[0]), mk) and np.array_equal(n(again[1]), start)
    # the neighbourhood: no swap of a listed pair is cyclic, and the swap in the kernel is the swap on the host
    count = int(found[0])
    assert 0 < count <= 128 and (pa[0, :count] >= 0).all() and (pa[0, count:] == -1).all() and (pb[0, count:] == -1).all()
    got = [n(x) for x in env.evaluate_order(None, np.zeros(count, np.int32), (pa[0, :count], pb[0, :count]), start=True, tail=True)]
    assert (got[0] > 0).all()
    for c in range(count):
        swapped = sol.copy().reshape(1, -1)
        a, b = int(pa[0, c]), int(pb[0, c])
        swapped[0, a], swapped[0, b] = sol.reshape(-1)[b], sol.reshape(-1)[a]
        one = [n(x) for x in env.evaluate_order(swapped.reshape(sol.shape), start=True, tail=True)]
        assert one[0][0] == got[0][c] and np.array_equal(one[1][0], got[1][c]) and np.array_equal(one[2][0], got[2][c]), c


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def definition_loop(env, cap=128, max_iter=None):
    """search.improve written with evaluate_order, a NumPy arg-min and a swap on the host: returns the makespans at the start
    of every iteration run (the last one improves nothing), the final rank, improving iterations, evaluations, truncations"""
    be = env.backend
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    B = env.batch
    rank = n(env.solution).copy()
    cur = n(env.evaluate_order(rank)).copy()
    history, iterations, evaluations, truncated = [], 0, 0, 0
    while max_iter is None or len(history) < max_iter:
        mk, pa, pb, found = (n(x) for x in env.evaluate_order(rank, pairs=cap))
        history.append(mk.copy())
        par = np.repeat(np.arange(B, dtype=np.int32), cap)
        cand = n(env.evaluate_order(rank, par, (pa.reshape(-1), pb.reshape(-1)))).reshape(B, cap)
        evaluations += int(np.minimum(np.maximum(found, 0), cap).sum())
        truncated += int((found > cap).sum())
        any_improved = False
        for i in range(B):
            valid = (cand[i] >= 0) & (pa[i] >= 0)
            if not valid.any():
                continue
            k = int(np.argmin(np.where(valid, cand[i], np.iinfo(np.int32).max)))      # (the first of equal makespans)
            if cand[i, k] < cur[i]:
                row = rank[i].reshape(-1)
                row[pa[i, k]], row[pb[i, k]] = row[pb[i, k]], row[pa[i, k]]
                cur[i] = cand[i, k]
                any_improved = True
        if not any_improved:
            break
        iterations += 1
    return np.array(history), rank, cur, iterations, evaluations, truncated


def rolled_out(be, instances, kind):
    one = not isinstance(instances, list)
    if one:
        env = BatchedJssEnv(instances, batch=1, _backend=be)
    else:
        env = BatchedJssEnv(instances, batch=len(instances), table_of_env=np.arange(len(instances)), order="interleaved", _backend=be)
    env.reset()
    env.rollout(kind, n_iter=3 * env.jmax * env.mmax, autoreset=False)
    return env


def case_driver(be, instances, kind, cap=128, check_every=(1, 3, 8), anchor=None):
    """improve against the definition loop for every check_every; the anchor's figures; the result replayed"""
    env = rolled_out(be, instances, kind)
    history, rank, cur, iterations, evaluations, truncated = definition_loop(env, cap)
    if anchor is not None:
        assert (int(history[0][0]), int(cur[0]), iterations, evaluations) == anchor and truncated == 0
    host = host_tables(env)
    for ce in check_every:
        res = search.improve(instances, kind, pair_cap=cap, check_every=ce, _backend=be)
        assert np.array_equal(res.history, history), ce
        assert np.array_equal(res.rank, rank) and np.array_equal(res.makespan, cur) and np.array_equal(res.makespan_before, history[0])
        assert (res.iterations, res.evaluations, res.truncated) == (iterations, evaluations, truncated), ce
        assert res.makespan.dtype == np.int32 and (res.makespan <= res.makespan_before).all()
    for i in range(env.batch):
        tab = int(host["env_const"][i, _abi.C_TABLE])
        J, M = int(host["env_const"][i, _abi.C_JOBS]), int(host["env_const"][i, _abi.C_MACHINES])
        assert feasible(res.start[i], (host["ops"][tab, :J, :M] >> 16) & 63, host["ops"][tab, :J, :M] & 0xFFFF) == res.makespan[i]
    # max_iter stops early at the definition's makespans; a done batch is taken as it is
    part = search.improve(env, max_iter=1, pair_cap=cap)
    assert np.array_equal(part.history, history[:1]) and np.array_equal(part.makespan, history[min(1, len(history) - 1)])
    return res


def case_apply(be):
    """jss_order_apply alone, on arrays written out here: the lowest (makespan, index) among the candidates that count; taken
    only if it is lower than the current makespan"""
    lib = search.order_library(be)
    B, jmax, mmax, cap = 5, 2, 3, 4
    rank0 = np.arange(B * jmax * mmax, dtype=np.int32).reshape(B, jmax, mmax)
    mk = np.array([[9, 7, 7, -1], [-1, -2, -1, -1], [5, 5, 5, 5], [3, 8, 2, 2], [4, 1, 6, 1]], np.int32)
    pa = np.array([[0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 6, 3], [0, -1, 2, 4]], np.int32)
    pb = np.array([[5, 4, 3, 2], [5, 4, 3, 2], [5, 4, 3, 2], [5, 4, 3, 2], [5, 4, 3, 2]], np.int32)
    cur0 = np.array([8, 8, 5, 9, 9], np.int32)
    with be.on_device():
        rank, cur, d_mk, d_pa, d_pb = (be.from_numpy(x) for x in (rank0, cur0, mk, pa, pb))
        improved = be.from_numpy(np.full(B, FILL, np.int32))
        p = be.ptr
        arg = _abi.JssOrderApply(B, jmax, mmax, cap, p(rank), p(cur), p(d_mk), p(d_pa), p(d_pb), p(improved))
        assert lib.jss_order_apply(C.byref(arg), be.stream()) == 0
        be.sync()
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    # env 0: 7 at index 1 (the first of the two); env 1: no candidate; env 2: 5 is not lower than 5; env 3: index 2 names entry 6
    # of a 6-entry row and does not count, so 2 at index 3; env 4: index 1 has no pair, so 1 at index 3
    assert n(improved).tolist() == [1, 0, 0, 1, 1] and n(cur).tolist() == [7, 8, 5, 2, 1]
    want = rank0.copy().reshape(B, -1)
    for i, (a, b) in ((0, (1, 4)), (3, (3, 2)), (4, (4, 2))):
        want[i, a], want[i, b] = want[i, b], want[i, a]
    assert np.array_equal(n(rank).reshape(B, -1), want)
    # errors leave everything alone; batch == 0 runs nothing
    keep = [n(x).copy() for x in (rank, cur, improved)]
    for field, value, code in (("rank", None, _abi.E_NULL), ("cur", None, _abi.E_NULL), ("makespan", None, _abi.E_NULL),
                               ("pair_a", None, _abi.E_NULL), ("pair_b", None, _abi.E_NULL), ("improved", None, _abi.E_NULL),
                               ("batch", -1, _abi.E_SHAPE), ("jmax", 0, _abi.E_SHAPE), ("jmax", 129, _abi.E_SHAPE),
                               ("mmax", 0, _abi.E_SHAPE), ("mmax", 65, _abi.E_SHAPE), ("pair_cap", 0, _abi.E_SHAPE), ("batch", 0, 0)):
        bad = _abi.JssOrderApply.from_buffer_copy(arg)
        setattr(bad, field, value)
        assert lib.jss_order_apply(C.byref(bad), be.stream()) == code, field
    assert lib.jss_order_apply(None, be.stream()) == _abi.E_NULL
    be.sync()
    for x, k in zip((rank, cur, improved), keep):
        assert np.array_equal(n(x), k)


# ---- ABI errors ------------------------------------------------------------------------------------------------------------------
def case_abi_errors(be):
    """every code of jss_order_eval, before anything runs: the outputs keep their fill"""
    lib = search.order_library(be)
    env = env_on(be, "3x2")
    st = case_state("3x2")
    B = env.batch
    with be.on_device():
        idx = be.from_numpy(np.zeros(B, dtype=np.int32))
        rank = be.from_numpy(st["rank"])
        out = {k: be.from_numpy(np.full(s, FILL, np.int32)) for k, s in (("makespan", B), ("start", (B, env.jmax, env.mmax)),
                                                                         ("tail", (B, env.jmax, env.mmax)), ("pair_a", (B, 4)),
                                                                         ("pair_b", (B, 4)), ("n_pairs", B))}
    p = be.ptr

    def call(n=B, desc=None, state=True, arg=True, **fields):
        d = _abi.JssDesc.from_buffer_copy(env._desc)
        for k, v in ({} if desc in (None, "null") else desc).items():
            setattr(d, k, v)
        o = _abi.JssOrder(n, 4, p(rank), p(idx), p(idx), p(idx), p(out["makespan"]), p(out["start"]), p(out["tail"]), p(out["pair_a"]),
                          p(out["pair_b"]), p(out["n_pairs"]))
        for k, v in fields.items():
            setattr(o, k, v)
        rc = lib.jss_order_eval(C.byref(d) if desc != "null" else None, C.byref(env._state) if state else None,
                                C.byref(o) if arg else None, be.stream())
        be.sync()
        return rc

    assert call(desc="null") == _abi.E_NULL and call(state=False) == _abi.E_NULL and call(arg=False) == _abi.E_NULL
    assert call(rank=None) == _abi.E_NULL and call(makespan=None) == _abi.E_NULL and call(desc={"ops": None}) == _abi.E_NULL
    assert call(n=-1) == _abi.E_SHAPE
    assert call(n=B - 1, parent=None) == _abi.E_SHAPE and call(n=B + 1, parent=None) == _abi.E_SHAPE
    assert call(swap_a=None) == _abi.E_SHAPE and call(swap_b=None) == _abi.E_SHAPE
    for missing in (("pair_a",), ("pair_b",), ("n_pairs",), ("pair_a", "pair_b"), ("pair_a", "n_pairs"), ("pair_b", "n_pairs")):
        assert call(**{k: None for k in missing}) == _abi.E_SHAPE, missing
    assert call(pair_cap=0) == _abi.E_SHAPE and call(pair_cap=-3) == _abi.E_SHAPE
    assert call(desc={"jmax": 0}) == _abi.E_SHAPE and call(desc={"mmax": 65}) == _abi.E_SHAPE and call(desc={"batch": -1}) == _abi.E_SHAPE
    assert call(desc={"kernel": 64}) == _abi.E_KIND
    # a row of more than 5352 entries does not fit one candidate's 64 KB of LDS: both libraries say so; 128 x 40 fits (not run)
    assert call(desc={"jmax": 128, "mmax": 64}) == _abi.E_LDS and call(desc={"jmax": 128, "mmax": 42}) == _abi.E_LDS
    assert call(n=0, desc={"jmax": 128, "mmax": 40}) == 0
    assert call(n=0) == 0
    for k, v in out.items():
        assert (np.asarray(be.numpy(v)) == FILL).all(), k
    # pair_cap is not looked at without the pair outputs; the full call and the parent == NULL call run
    assert call(pair_cap=0, pair_a=None, pair_b=None, n_pairs=None) == 0
    assert call() == 0 and call(parent=None, swap_a=None, swap_b=None) == 0
    assert not (np.asarray(be.numpy(out["makespan"])) == FILL).any()


# ---- the built library ------------------------------------------------------------------------------------------------------------
def order_kernel_rows():
    """[(name, vgprs, sgprs, spilled vgprs, spilled sgprs, scratch bytes, static LDS bytes)] of libjss_order_hip.so"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import LLVM, kernel_resources
    from jssenv_amd.build import build_order_extension
    so = build_order_extension()                                      # (built here if build() has not run)
    rows = kernel_resources(so)
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "order.co")
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", so, fat], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    lds = [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", notes)]
    assert len(lds) == len(rows)
    return [r + (b,) for r, b in zip(rows, lds)]


def exported(path):
    """the dynamic symbols a shared library defines"""
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}
