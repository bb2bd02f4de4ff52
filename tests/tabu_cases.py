"""Backend-agnostic cases of jss_tabu_search (include/jss_tabu.h), BatchedJssEnv.tabu and search.tabu_search, run against the
host-core twin, the kernel source (jssenv_amd/csrc/jss_tabu.hip) under the SIMT emulator and the HIP library libjss_tabu_hip.so.

The reference is search.tabu_reference (NumPy, written from the header's definition on top of order_eval_reference).  The batches
and the rank tensors are order_cases': finished random and SPT rollouts, orders that are schedules with ties, cyclic ones, and a
last env that was never reset.  A run's reference is made once and shared by the three backends, which are compared with it bit
for bit in all five outputs."""
import ctypes as C
import os
import subprocess

import numpy as np

import order_cases as K
from clone_cases import rows_of
from jssenv_amd import BatchedJssEnv, _abi, search

ROOT = K.ROOT
TABU_SRC = os.path.join(ROOT, "jssenv_amd", "csrc", "jss_tabu.hip")
EMU_LIB = os.path.join(K.EMU, "libjss_tabu_emu.so")
FILL = K.FILL                       # what the outputs hold before a call: the rows of refused and cyclic walkers keep it
OUTPUTS = ("last", "info", "trace")

# B = 1, start rollout(kind): (instance, kind, tenure, iters) -> (start, best, at move, evaluations)
ANCHORS = {("ta01", "SPT", 8, 300): (1462, 1297, 153, 4094), ("ta01", "FIFO", 8, 300): (1486, 1371, 267, 3496),
           ("ta41", "SPT", 8, 200): (2499, 2356, 131, 8107), ("ta01", "SPT", 3, 64): (1462, 1361, 50, 990)}
# ta01 SPT, tenure 8, 300 moves: target -> info row
TARGET_ANCHORS = {1400: (2, 7, 7, 117), 1462: (2, 0, 0, 0)}
MIXED = dict(instances=["ta01", "ta02", "ta11"], table_of_env=[0, 1, 2, 2, 1, 0], kind="FIFO", tenure=[8, 8, 8, 5, 5, 5], iters=120,
             start=(1486, 1463, 1685, 1685, 1463, 1486), best=(1408, 1420, 1613, 1636, 1420, 1391),
             best_move=(119, 25, 85, 9, 36, 100), evaluations=(1345, 2298, 3162, 3368, 2234, 1427))


def build_emu_tabu():
    """jss_tabu.hip, unmodified, compiled with g++ against the SIMT emulator's hip_runtime.h: a library of its own"""
    deps = [TABU_SRC, os.path.join(K.EMU, "hip", "hip_runtime.h"), os.path.join(ROOT, "include", "jss_tabu.h"),
            os.path.join(ROOT, "include", "jss_order.h"), os.path.join(ROOT, "jssenv_amd", "csrc", "jss_abi_checks.hpp")]
    if not os.path.isfile(EMU_LIB) or any(os.path.getmtime(d) > os.path.getmtime(EMU_LIB) for d in deps):
        tmp = EMU_LIB + f".tmp{os.getpid()}"
        subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
                               "-Wno-unknown-pragmas", "-I" + K.EMU, "-I" + os.path.join(ROOT, "include"), TABU_SRC, "-o", tmp])
        os.replace(tmp, EMU_LIB)
    return EMU_LIB


def emu_backend():
    """order_cases' emulator backend (the env kernels and jss_order.hip) with the emulated tabu library as its `tabu_lib`"""
    be = K.emu_backend()
    be.tabu_lib = _abi.bind_tabu(C.CDLL(build_emu_tabu()))
    return be


twin_backend = K.twin_backend


# ---- the runs ------------------------------------------------------------------------------------------------------------------
# Per case: (iters, tenure, target).  tenure: an int, or "each": one per walker from TENURES, so that one launch holds the
# tenures 0, 2 and 64; or "bad": per walker, with the first two outside [0, 64].  target: None; "best": per walker what the
# walk without a target ends with, so that it stops in mid-walk (or at move 0 where the start is never beaten), the odd walkers
# their start, so that they stop at move 0; "never": 0 for everyone.  The small cases run every tenure, the others one launch
# with a tenure per walker, at the move counts that keep a reference at a few seconds.
TENURES = (0, 2, 64, 5, 1, 8)
SMALL = ("1x2", "3x2", "repeats", "per-env")
RUNS = {
    "1x2": [(6, 0, None), (6, 2, None), (6, 64, None), (6, "each", None), (6, 2, "best"), (0, 2, None)],
    "3x2": [(20, 0, None), (20, 2, None), (20, 64, None), (20, "each", None), (20, 2, "best"), (20, "bad", "never"), (0, 64, "best")],
    "repeats": [(24, 0, None), (24, 2, None), (24, 64, None), (24, "each", "best"), (0, 0, None)],
    "per-env": [(16, 0, None), (16, 2, None), (16, 64, None), (16, "each", None), (16, "each", "best")],
    "table-of-env": [(10, "each", None)],
    "by-shape": [(6, "each", None)],
    "J65": [(40, "each", None)],
    "ta01": [(40, "each", None), (40, 2, "best")],
    "100x20": [(3, "each", None)],
}
_REFS = {}
_EVENTS = {}


def tenure_of_run(name, tenure):
    B = K.CASES[name][1]
    if tenure == "each":
        return np.array([TENURES[i % len(TENURES)] for i in range(B)], np.int32)
    if tenure == "bad":
        return np.array([65, -1] + [TENURES[i % len(TENURES)] for i in range(2, B)], np.int32)
    return int(tenure)


def cyclic_and_unfinished():
    """the 3 x 2's rank tensor with env 0 a schedule, env 1 cyclic with the job chains (J2's second operation before J0's first on
    machine 0, J0's second before J2's first on machine 1), env 2 an unfinished solution (-1 on a real operation); env 3 is the
    one never reset"""
    rank = K.case_state("3x2")["rank"].copy()
    rank[1] = [[5, 0], [5, 5], [5, 0]]
    rank[2] = rank[0]
    rank[2, 1, 1] = -1
    return rank


def reference(name, run):
    """(best_makespan, best_rank, last_rank, info, trace) of the mirror for run `run` of case `name`, with the rank tensor, the
    tenure and the target the backends are to be given; made once"""
    key = (name, run)
    if key in _REFS:
        return _REFS[key]
    st = K.case_state(name)
    rank = cyclic_and_unfinished() if run == "hand" else st["rank"]
    iters, tenure, target = (12, 2, None) if run == "hand" else RUNS[name][run]
    tenure = tenure_of_run(name, tenure)
    host = st["host"]
    if target == "best":
        free = search.tabu_reference(host["env_const"], host["ops"], rank, iters, tenure, None, fill=FILL)
        starts = search.order_eval_reference(host["env_const"], host["ops"], rank)[0]
        target = np.where(np.arange(st["B"]) % 2 == 1, starts, free[0]).astype(np.int32)
    elif target == "never":
        target = np.zeros(st["B"], np.int32)
    log = []
    ref = search.tabu_reference(host["env_const"], host["ops"], rank, iters, tenure, target, fill=FILL, log=log)
    _REFS[key] = dict(rank=rank, iters=iters, tenure=tenure, target=target, ref=ref)
    _EVENTS[key] = log
    return _REFS[key]


def call_tabu(be, env, rank, iters, tenure, target=None, want=OUTPUTS, desc=None):
    """jss_tabu_search through the backend's library: (rc, best_makespan, best_rank, last_rank, info, trace) as host arrays (None
    where not asked for); the outputs are prefilled (FILL), so what a call leaves alone can be told from what it writes"""
    lib = search.tabu_library(be)
    B = env.batch
    with be.on_device():
        dev = lambda x: None if x is None else be.from_numpy(np.asarray(x, np.int32))   # noqa: E731
        full = lambda shape: be.from_numpy(np.full(shape, FILL, np.int32))   # noqa: E731
        rk = dev(rank)
        ten = dev(tenure) if np.ndim(tenure) else None
        tgt = dev(target)
        mk, best = full(B), full((B, env.jmax, env.mmax))
        last = full((B, env.jmax, env.mmax)) if "last" in want else None
        info = full((B, _abi.TABU_NI)) if "info" in want else None
        trace = full((B, max(iters, 1))) if "trace" in want else None
        p = be.ptr
        arg = _abi.JssTabu(iters, 0 if ten is not None else int(tenure), p(rk), p(ten), p(tgt), p(mk), p(best), p(last), p(info), p(trace))
        rc = lib.jss_tabu_search(C.byref(env._desc if desc is None else desc), C.byref(env._state), C.byref(arg), be.stream())
        be.sync()
    host = lambda x: None if x is None else np.asarray(be.numpy(x))   # noqa: E731
    trace = None if trace is None else host(trace).reshape(-1)[:B * iters].reshape(B, iters)   # (rows of `iters` words)
    return rc, host(mk), host(best), host(last), host(info), trace


def same(got, ref, what):
    """a call's outputs against the mirror's (best_makespan, best_rank, last_rank, info, trace), those that were asked for"""
    assert got[0] == 0, (what, got[0])
    assert got[1].dtype == np.int32 and np.array_equal(got[1], ref[0]), (what, "best_makespan", got[1], ref[0])
    assert np.array_equal(got[2], ref[1]), (what, "best_rank")
    for k, label in ((3, "last_rank"), (4, "info"), (5, "trace")):
        if got[k] is not None:
            assert np.array_equal(got[k], ref[k - 1]), (what, label)


def case_against_mirror(be, name):
    """every run of the case against the mirror, with all optional outputs; on the small cases' first run the optional outputs in
    every combination; the batch untouched"""
    st = K.case_state(name)
    env = K.env_on(be, name)
    before = rows_of(env)
    runs = list(range(len(RUNS[name]))) + (["hand"] if name == "3x2" else [])
    for run in runs:
        r = reference(name, run)
        same(call_tabu(be, env, r["rank"], r["iters"], r["tenure"], r["target"]), r["ref"], (name, run))
    r = reference(name, 0)
    for mask in (range(8) if name in SMALL else ()):
        want = tuple(w for bit, w in enumerate(OUTPUTS) if mask >> bit & 1)
        same(call_tabu(be, env, r["rank"], r["iters"], r["tenure"], r["target"], want=want), r["ref"], (name, want))
    ref = reference(name, 0)["ref"]
    dead = ref[0] < 0
    assert dead[st["B"] - 1] and ref[0][st["B"] - 1] == -1 and not dead[0]                 # the env never reset; a walk
    for k in (1, 2, 4):
        assert (ref[k][dead] == FILL).all() and not (ref[k][~dead] == FILL).any(), (name, k)
    assert (ref[3][dead, 1:] == 0).all() and np.array_equal(ref[3][dead, 0], ref[0][dead])
    after = rows_of(env)
    for k in before:
        assert np.array_equal(before[k], after[k]), (name, k)


def case_hand_rows(be):
    """a cyclic rank (-2) and an unfinished solution (-1) next to a walk: their rows keep the fill"""
    r = reference("3x2", "hand")
    got = call_tabu(be, K.env_on(be, "3x2"), r["rank"], r["iters"], r["tenure"], r["target"])
    same(got, r["ref"], "hand")
    assert got[1][0] > 0 and got[1][1:].tolist() == [-2, -1, -1]
    assert got[4][1:].tolist() == [[-2, 0, 0, 0], [-1, 0, 0, 0], [-1, 0, 0, 0]]
    for k in (2, 3, 5):
        assert (got[k][1:] == FILL).all() and not (got[k][0] == FILL).any()


def what_the_cases_cover():
    """over all runs of all cases the references hold: a tabu move taken by aspiration, a forced move (none admissible), every
    way a walk stops -- no neighbour left, the target at move 0, the target in mid-walk, iters moves made -- a refused and a cyclic row"""
    seen = dict(aspired=0, forced=0, stop1=0, stop2_at_0=0, stop2_mid=0, stop0=0, refused=0, cyclic=0, bad_tenure=0)
    for name in RUNS:
        for run in list(range(len(RUNS[name]))) + (["hand"] if name == "3x2" else []):
            r = reference(name, run)
            info, mk = r["ref"][3], r["ref"][0]
            for _, _, kind in _EVENTS[(name, run)]:
                seen[kind] += 1
            seen["stop1"] += int((info[:, 0] == 1).sum())
            seen["stop2_at_0"] += int(((info[:, 0] == 2) & (info[:, 1] == 0)).sum())
            seen["stop2_mid"] += int(((info[:, 0] == 2) & (info[:, 1] > 0)).sum())
            seen["stop0"] += int(((info[:, 0] == 0) & (mk >= 0)).sum())
            seen["refused"] += int((mk == -1).sum())
            seen["cyclic"] += int((mk == -2).sum())
            if np.ndim(r["tenure"]):
                seen["bad_tenure"] += int((((r["tenure"] < 0) | (r["tenure"] > 64)) & (mk == -1))[:-1].sum())
    return seen


# ---- the anchors -----------------------------------------------------------------------------------------------------------------
def rolled_out(be, instance, kind):
    return K.rolled_out(be, instance, kind)


def case_anchor(be, key, mirror=False):
    """B = 1 from rollout(kind): the listed start, best, move and evaluations; with `mirror` the NumPy mirror gives them too"""
    name, kind, tenure, iters = key
    env = rolled_out(be, name, kind)
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    start = int(n(env.evaluate_order())[0])
    mk, _, info = (n(x) for x in env.tabu(None, iters, tenure))
    assert (start, int(mk[0]), int(info[0, 2]), int(info[0, 3])) == ANCHORS[key] and info[0, :2].tolist() == [0, iters]
    if mirror:
        host = K.host_tables(env)
        ref = search.tabu_reference(host["env_const"], host["ops"], n(env.solution), iters, tenure)
        assert (int(ref[0][0]), int(ref[3][0, 2]), int(ref[3][0, 3])) == ANCHORS[key][1:]


def case_target_anchors(be, mirror=False):
    env = rolled_out(be, "ta01", "SPT")
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    for target, row in TARGET_ANCHORS.items():
        mk, _, info = (n(x) for x in env.tabu(None, 300, 8, target))
        assert tuple(info[0].tolist()) == row and mk[0] <= target
        if mirror:
            host = K.host_tables(env)
            ref = search.tabu_reference(host["env_const"], host["ops"], n(env.solution), 300, 8, target)
            assert tuple(ref[3][0].tolist()) == row


def case_mixed(be):
    """three instances dealt onto six envs, two tenures: every env's figures"""
    m = MIXED
    env = BatchedJssEnv(m["instances"], batch=6, table_of_env=m["table_of_env"], _backend=be)
    env.reset()
    env.rollout(m["kind"], n_iter=3 * env.jmax * env.mmax, autoreset=False)
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    assert tuple(n(env.evaluate_order()).tolist()) == m["start"]
    mk, _, info = (n(x) for x in env.tabu(None, m["iters"], np.asarray(m["tenure"], np.int32)))
    assert tuple(mk.tolist()) == m["best"] and tuple(info[:, 2].tolist()) == m["best_move"]
    assert tuple(info[:, 3].tolist()) == m["evaluations"] and (info[:, 0] == 0).all() and (info[:, 1] == m["iters"]).all()


# ---- properties ------------------------------------------------------------------------------------------------------------------
def case_properties(be, instance, kind, iters, tenure):
    """a walk from a finished `kind` rollout: see the asserts"""
    env = rolled_out(be, instance, kind)
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    host = K.host_tables(env)
    J, M = int(host["env_const"][0, _abi.C_JOBS]), int(host["env_const"][0, _abi.C_MACHINES])
    mach, dur = (host["ops"][0, :J, :M] >> 16) & 63, host["ops"][0, :J, :M] & 0xFFFF
    start = int(n(env.evaluate_order())[0])
    mk, best_rank, info, trace, last_rank = (n(x) for x in env.tabu(None, iters, tenure, trace=True, last=True))
    stop, moves, best_move, evaluations = (int(x) for x in info[0])
    assert stop == 0 and moves == iters and evaluations >= moves and trace.shape == (1, iters) and (trace > 0).all()
    # either rank reproduces its schedule; the best one's start times are a feasible schedule of that length
    again, times = (n(x) for x in env.evaluate_order(best_rank, start=True))
    assert again[0] == mk[0] and K.feasible(times[0], mach, dur) == mk[0]
    assert n(env.evaluate_order(last_rank))[0] == trace[0, moves - 1]
    # positions: on every machine 0 ... count - 1, -1 in the padding
    for r in (best_rank[0], last_rank[0]):
        assert (r[J:] == -1).all() and (r[:, M:] == -1).all()
        for m in np.unique(mach):
            assert sorted(r[:J, :M][mach == m].tolist()) == list(range(int((mach == m).sum())))
    # the best is the lowest makespan the walk saw, found at the first move that reached it
    seen = np.concatenate(([start], trace[0]))
    assert mk[0] == seen.min() and best_move == int(np.argmax(seen == seen.min()))
    # a prefix of the walk is the shorter walk
    half = [n(x) for x in env.tabu(None, iters // 2, tenure, trace=True)]
    assert np.array_equal(half[3][0], trace[0, :iters // 2]) and half[0][0] == seen[:iters // 2 + 1].min()
    # iters = 0: the plain evaluation, best_rank the normalised order
    mk0, rank0, info0 = (n(x) for x in env.tabu(None, 0, tenure))
    assert mk0[0] == start and info0[0].tolist() == [0, 0, 0, 0] and n(env.evaluate_order(rank0))[0] == start
    assert np.array_equal(n(env.evaluate_order(rank0, start=True)[1]), n(env.evaluate_order(start=True)[1]))


def case_descent(be, instance, kind, tenures=(0, 3, 64)):
    """while every move improves, aspiration makes the tabu walk the steepest descent: with iters = improve().iterations from the
    same start, the same makespans after every move, for any tenure"""
    res = search.improve(instance, kind, _backend=be)
    env = rolled_out(be, instance, kind)
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    assert res.iterations > 0 and res.truncated == 0
    for tenure in tenures:
        mk, _, info, trace = (n(x) for x in env.tabu(None, res.iterations, tenure, trace=True))
        assert np.array_equal(mk, res.makespan) and np.array_equal(trace.T, res.history[1:]), tenure
        assert info[0].tolist()[:3] == [0, res.iterations, res.iterations]


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def definition_loop(be, instances, kind, walkers, iters, tenure, explore, seed, target):
    """search.tabu_search written with the public calls: returns (makespan, walker, rank, start, optimal, best_makespan, info)"""
    names = instances if isinstance(instances, list) else [instances]
    G, W = len(names), walkers
    if G == 1:
        env = BatchedJssEnv(names[0], batch=W, seed=seed, _backend=be)
    else:
        env = BatchedJssEnv(names, batch=G * W, table_of_env=np.repeat(np.arange(G), W), order="interleaved", seed=seed, _backend=be)
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    env.reset()
    tgt = n(env.lower_bound()).copy() if target == "lower_bound" else None if target is None else np.repeat(np.asarray(target, np.int32), W)
    env.rollout(kind, n_iter=3 * env.jmax * env.mmax, autoreset=False, explore=explore, seed=seed)
    lo, hi = tenure
    ten = np.array([lo + w % (hi - lo + 1) for _ in range(G) for w in range(W)], np.int32)
    mk, best_rank, info = (n(x) for x in env.tabu(None, iters, ten, tgt))
    makespan, walker = [], []
    for g in range(G):
        low = min((int(mk[g * W + w]), w) for w in range(W) if mk[g * W + w] >= 0)
        makespan.append(low[0]), walker.append(low[1])
    winner = np.array([g * W + w for g, w in enumerate(walker)], np.int32)
    again, start = (n(x) for x in env.evaluate_order(best_rank, winner, start=True))
    assert again.tolist() == makespan
    optimal = [bool(info[i, 0] == 1 or (tgt is not None and mk[i] <= tgt[i])) for i in winner]
    return np.array(makespan), np.array(walker), best_rank[winner], start, np.array(optimal), mk, info


def case_driver(be, instances, kind="SPT", walkers=4, iters=30, tenure=(5, 12), explore=0.1, seed=0, target="lower_bound"):
    want = definition_loop(be, instances, kind, walkers, iters, tenure, explore, seed, target)
    res = search.tabu_search(instances, kind, walkers, iters, tenure, explore, seed, target, _backend=be)
    for g, w, label in zip((res.makespan, res.walker, res.rank, res.start, res.optimal, res.best_makespan, res.info), want,
                           ("makespan", "walker", "rank", "start", "optimal", "best_makespan", "info")):
        assert np.array_equal(g, w), label
    G = len(res.makespan)
    assert np.array_equal(res.makespan, res.best_makespan.reshape(G, walkers).min(axis=1))   # the group's best walker
    assert res.makespan.dtype == np.int32 and res.env.batch == G * walkers
    return res


# ---- ABI errors ------------------------------------------------------------------------------------------------------------------
def case_abi_errors(be):
    """every code of jss_tabu_search, before anything runs: the outputs keep their fill"""
    lib = search.tabu_library(be)
    env = K.env_on(be, "3x2")
    st = K.case_state("3x2")
    B = env.batch
    with be.on_device():
        rank = be.from_numpy(st["rank"])
        ten, tgt = be.from_numpy(np.full(B, 2, np.int32)), be.from_numpy(np.zeros(B, np.int32))
        out = {k: be.from_numpy(np.full(s, FILL, np.int32)) for k, s in (("best_makespan", B), ("best_rank", (B, env.jmax, env.mmax)),
                                                                         ("last_rank", (B, env.jmax, env.mmax)),
                                                                         ("info", (B, _abi.TABU_NI)), ("trace", (B, 5)))}
    p = be.ptr

    def call(desc=None, state=True, arg=True, **fields):
        d = _abi.JssDesc.from_buffer_copy(env._desc)
        for k, v in ({} if desc in (None, "null") else desc).items():
            setattr(d, k, v)
        t = _abi.JssTabu(5, 2, p(rank), p(ten), p(tgt), p(out["best_makespan"]), p(out["best_rank"]), p(out["last_rank"]),
                         p(out["info"]), p(out["trace"]))
        for k, v in fields.items():
            setattr(t, k, v)
        rc = lib.jss_tabu_search(C.byref(d) if desc != "null" else None, C.byref(env._state) if state else None,
                                 C.byref(t) if arg else None, be.stream())
        be.sync()
        return rc

    assert call(desc="null") == _abi.E_NULL and call(state=False) == _abi.E_NULL and call(arg=False) == _abi.E_NULL
    assert call(rank=None) == _abi.E_NULL and call(best_makespan=None) == _abi.E_NULL and call(best_rank=None) == _abi.E_NULL
    assert call(desc={"ops": None}) == _abi.E_NULL
    assert call(iters=-1) == _abi.E_SHAPE and call(iters=65537) == _abi.E_SHAPE
    assert call(tenure=-1, tenure_of=None) == _abi.E_SHAPE and call(tenure=65, tenure_of=None) == _abi.E_SHAPE
    assert call(desc={"jmax": 0}) == _abi.E_SHAPE and call(desc={"mmax": 65}) == _abi.E_SHAPE and call(desc={"batch": -1}) == _abi.E_SHAPE
    assert call(desc={"kernel": 64}) == _abi.E_KIND
    # a row of more than 5352 entries does not fit one walker's 64 KB of LDS: both libraries say so; 128 x 40 fits (not run)
    assert call(desc={"jmax": 128, "mmax": 64}) == _abi.E_LDS and call(desc={"jmax": 128, "mmax": 42}) == _abi.E_LDS
    assert call(desc={"jmax": 128, "mmax": 40, "batch": 0}) == 0 and call(desc={"batch": 0}) == 0      # batch == 0 launches nothing
    for k, v in out.items():
        assert (np.asarray(be.numpy(v)) == FILL).all(), k
    # tenure is not looked at where tenure_of is given; the optional pointers may all be NULL; iters at its bounds is accepted
    assert call(tenure=99) == 0 and call(iters=0, tenure_of=None, target=None, last_rank=None, info=None, trace=None) == 0
    assert call(tenure=64, tenure_of=None) == 0 and call(tenure=0, tenure_of=None, iters=1) == 0
    assert not (np.asarray(be.numpy(out["best_makespan"])) == FILL).any()


# ---- the built library ------------------------------------------------------------------------------------------------------------
def tabu_kernel_rows():
    """[(name, vgprs, sgprs, spilled vgprs, spilled sgprs, scratch bytes, static LDS bytes)] of libjss_tabu_hip.so"""
    import re
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import LLVM, kernel_resources
    from jssenv_amd.build import build_tabu_extension
    so = build_tabu_extension()                                       # (built here if build() has not run)
    rows = kernel_resources(so)
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "tabu.co")
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", so, fat], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    lds = [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", notes)]
    assert len(lds) == len(rows)
    return [r + (b,) for r, b in zip(rows, lds)]
