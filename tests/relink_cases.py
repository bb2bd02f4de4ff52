"""Backend-agnostic cases of jss_relink_walk (include/jss_relink.h), BatchedJssEnv.relink / order_distance and search.relink_search,
run against the host-core twin, the kernel source (jssenv_amd/csrc/jss_relink.hip) under the SIMT emulator and the HIP library
libjss_relink_hip.so.

The reference is search.relink_reference (NumPy, written from the header's definition on top of order_eval_reference).  The batches
and the source ranks are block_cases' (order_cases' and the "chain"); a hand instance, "fallback", adds a move on which no candidate
passes the screen.  A run's reference is made once and shared by the three backends, which are compared with it bit for bit in all
seven outputs."""
import ctypes as C
import os
import subprocess

import numpy as np

import order_cases as K
import tabu_cases as T
import block_cases as Bk
from clone_cases import rows_of
from jssenv_amd import BatchedJssEnv, _abi, search

ROOT = K.ROOT
RELINK_SRC = os.path.join(ROOT, "jssenv_amd", "csrc", "jss_relink.hip")
EMU_LIB = os.path.join(K.EMU, "libjss_relink_emu.so")
FILL = K.FILL                       # what the outputs hold before a call: the rows of refused and cyclic walkers keep it
OUTPUTS = ("last_mk", "last", "info", "trace", "log")
ENOUGH = 200                        # more moves than any pair of orders of a small case is apart

# B = 1, source and guide the solutions of finished rule rollouts used as ranks:
# (instance, source, guide) -> (dist0, the source's makespan, the guide's, the lowest on the path, its move, the highest)
ANCHORS = {
    ("ta01", "SPT", "FIFO"): (204, 1462, 1486, 1440, 92, 1592),
    ("ta01", "FIFO", "SPT"): (204, 1486, 1462, 1431, 73, 1618),
    ("ta01", "SPT", "MWR"): (206, 1462, 1491, 1435, 128, 1505),
    ("ta01", "MWR", "FIFO"): (134, 1491, 1486, 1451, 85, 1510),
    ("ta41", "SPT", "FIFO"): (1165, 2499, 2543, 2472, 177, 2783),
    ("ta41", "FIFO", "SPT"): (1165, 2543, 2499, 2452, 336, 2891),
    ("ta41", "SPT", "MWR"): (1461, 2499, 2620, 2444, 614, 3183),
    ("ta41", "MWR", "FIFO"): (1224, 2620, 2543, 2497, 1223, 3039),
}

# the hand case: 3 jobs x 5 machines, positive and zero durations mixed; forwards one move finds no candidate that passes the screen
HAND_MACHINE = [[0, 2, 4, 1, 3], [4, 2, 3, 1, 0], [2, 0, 3, 4, 1]]
HAND_DURATION = [[0, 3, 3, 0, 0], [3, 0, 0, 1, 1], [1, 3, 1, 3, 2]]
HAND_SOURCE = [[0, 0, 1, 0, 0], [0, 1, 2, 1, 2], [2, 1, 1, 2, 2]]
HAND_GUIDE = [[0, 1, 2, 0, 2], [1, 2, 1, 1, 2], [0, 1, 0, 0, 2]]
# direction -> (dist0, the makespans of the source and of every move, fallbacks, retries, candidates)
HAND_WALKS = {"forward": (6, [13, 13, 13, 12, 12, 14, 17], 1, 0, 12), "back": (6, [17, 14, 12, 12, 13, 13, 13], 0, 0, 13)}

# a walk that swaps a candidate back (retries = 1), found by case_seeded_search (seed 2024): 3 jobs x 4 machines, eight of the
# twelve durations 0, so that on one move no start time tells the screen anything and the first candidate the fallback tries
# closes a cycle
RETRY_MACHINE = [[1, 2, 3, 0], [2, 0, 3, 1], [3, 1, 2, 0]]
RETRY_DURATION = [[1, 1, 0, 0], [0, 0, 0, 0], [0, 0, 1, 1]]
RETRY_SOURCE = [[0, 5, 8, 9], [1, 2, 6, 11], [3, 4, 7, 10]]
RETRY_GUIDE = [[2, 3, 4, 6], [1, 7, 9, 10], [0, 5, 8, 11]]


def build_emu_relink():
    """jss_relink.hip, unmodified, compiled with g++ against the SIMT emulator's hip_runtime.h: a library of its own"""
    deps = [RELINK_SRC, os.path.join(K.EMU, "hip", "hip_runtime.h"), os.path.join(ROOT, "jssenv_amd", "csrc", "jss_abi_checks.hpp")]
    deps += [os.path.join(ROOT, "include", h) for h in ("jss_relink.h", "jss_block.h", "jss_tabu.h", "jss_order.h")]
    if not os.path.isfile(EMU_LIB) or any(os.path.getmtime(d) > os.path.getmtime(EMU_LIB) for d in deps):
        tmp = EMU_LIB + f".tmp{os.getpid()}"
        subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
                               "-Wno-unknown-pragmas", "-I" + K.EMU, "-I" + os.path.join(ROOT, "include"), RELINK_SRC, "-o", tmp])
        os.replace(tmp, EMU_LIB)
    return EMU_LIB


def emu_backend():
    """block_cases' emulator backend (the env kernels, jss_order.hip, jss_tabu.hip, jss_block.hip) with the emulated relink
    library as its `relink_lib`"""
    be = Bk.emu_backend()
    be.relink_lib = _abi.bind_relink(C.CDLL(build_emu_relink()))
    return be


twin_backend = K.twin_backend


# ---- the batches -----------------------------------------------------------------------------------------------------------------
def inst_with_zeros(name, machine, duration):
    """an Instance whose durations may be 0.  Instance refuses them because the step kernels need d >= 1; the walks here read the
    op table only and nothing steps these envs, so the zeros are written into the array behind a valid instance"""
    duration = np.asarray(duration, np.int32)
    inst = K.inst(name, machine, np.maximum(duration, 1))
    inst.duration[...] = duration
    return inst


def hand_instance():
    return inst_with_zeros("fallback", HAND_MACHINE, HAND_DURATION)


def retry_instance():
    return inst_with_zeros("retry", RETRY_MACHINE, RETRY_DURATION)


HAND = {"fallback": (lambda be: BatchedJssEnv(hand_instance(), batch=3, _backend=be, seed=19), 3),
        "retry": (lambda be: BatchedJssEnv(retry_instance(), batch=3, _backend=be, seed=23), 3)}
HAND_RANKS = {"fallback": (HAND_SOURCE, HAND_GUIDE), "retry": (RETRY_SOURCE, RETRY_GUIDE)}
CASES = dict(Bk.CASES, **HAND)
ONE_TABLE = ("1x2", "3x2", "ta01", "J65", "100x20", "repeats", "chain", "fallback", "retry")   # every env reads the same table
_HAND_STATES = {}


def make_env(be, name):
    if name in Bk.CASES:
        return Bk.make_env(be, name)
    make, B = HAND[name]
    env = make(be)
    which = np.ones(B, np.uint8)
    which[B - 1] = 0
    env.reset(which=which)
    return env


def case_state(name):
    """block_cases.case_state for its cases; for "fallback" and "retry" the same keys: env 0 the hand source, env 1 the hand guide
    (so that the guide "other" walks forwards on env 0 and back on env 1), the env never reset a copy of env 0's"""
    if name in Bk.CASES:
        return Bk.case_state(name)
    if name not in _HAND_STATES:
        env = make_env(twin_backend(), name)
        source, guide = HAND_RANKS[name]
        rank = np.array([source, guide, source], np.int32)
        _HAND_STATES[name] = dict(env=env, host=K.host_tables(env), rank=np.ascontiguousarray(rank), B=HAND[name][1])
    return _HAND_STATES[name]


def env_on(be, name):
    return case_state(name)["env"] if be is twin_backend() else make_env(be, name)


# ---- the runs ------------------------------------------------------------------------------------------------------------------
# Per case: (steps, until, margin, guide).  until: an int; "each": per walker from UNTILS; "bad": per walker with the first one
# negative.  guide: "asc" / "desc": job index ascending / descending on every machine (always a schedule); "other": the source
# of the next reset env of the batch (a cyclic one among them), where all envs read one table; "self": the source itself,
# dist0 = 0; "negative": "asc" with a negative rank on a real operation of env 0; "hand": tabu_cases' tensor with a cyclic row
# (env 1) and an unfinished one (env 2) as the guide; "hand-source": that tensor as the source, the guide "asc".  margin 1000
# is one no order satisfies.
UNTILS = (0, 3, 1, 2, 7, 0)
SMALL = ("1x2", "3x2", "repeats", "per-env", "chain", "fallback", "retry")


def _small(other=True):
    runs = [(ENOUGH, 0, 0, "desc"), (0, 0, 0, "asc"), (1, 0, 0, "desc"), (3, 0, 0, "asc"), (ENOUGH, 0, 0, "asc"), (ENOUGH, 2, 0, "desc"),
            (ENOUGH, "each", 0, "asc"), (ENOUGH, 0, 2, "desc"), (ENOUGH, 2, 2, "asc"), (ENOUGH, 0, 1000, "desc"), (3, 0, 1000, "asc"),
            (ENOUGH, 0, 0, "self"), (0, 0, 0, "self")]
    if other:
        runs += [(ENOUGH, 0, 0, "other"), (3, "each", 0, "other"), (ENOUGH, 0, 2, "other"), (0, 0, 0, "other")]
    return runs


RUNS = {
    "1x2": _small(),
    "3x2": _small() + [(ENOUGH, "bad", 0, "desc"), (ENOUGH, 0, 0, "negative"), (ENOUGH, 0, 0, "hand"), (ENOUGH, 0, 0, "hand-source")],
    "repeats": _small(),
    "per-env": _small(other=False),
    "chain": _small(),
    "fallback": _small(),
    "retry": _small(),
    "table-of-env": [(10, 0, 0, "asc"), (10, "each", 2, "desc")],
    "by-shape": [(6, 0, 0, "desc")],
    "J65": [(8, 0, 0, "asc"), (8, "each", 0, "other")],
    "ta01": [(40, 0, 0, "asc"), (40, "each", 2, "other"), (0, 0, 0, "desc")],
    "100x20": [(3, 0, 0, "desc")],
}
_REFS = {}
_EVENTS = {}


def until_of_run(name, until):
    B = CASES[name][1]
    if until == "each":
        return np.array([UNTILS[i % len(UNTILS)] for i in range(B)], np.int32)
    if until == "bad":
        return np.array([-1] + [UNTILS[i % len(UNTILS)] for i in range(1, B)], np.int32)
    return int(until)


def guide_of_run(name, kind):
    st = case_state(name)
    rank, B = st["rank"], st["B"]
    jobs = np.arange(rank.shape[1], dtype=np.int32)[None, :, None] * np.ones((B, 1, rank.shape[2]), np.int32)
    if kind == "hand":
        return T.cyclic_and_unfinished()
    if kind in ("asc", "negative", "hand-source"):
        guide = jobs.copy()
        if kind == "negative":
            J, M = (int(x) for x in st["host"]["env_const"][0, [_abi.C_JOBS, _abi.C_MACHINES]])
            guide[0, J - 1, M - 1] = -1
        return guide
    if kind == "desc":
        return rank.shape[1] - 1 - jobs
    if kind == "self":
        return rank.copy()
    assert kind == "other" and name in ONE_TABLE
    return np.ascontiguousarray(rank[[(i + 1) % (B - 1) for i in range(B - 1)] + [0]])


def reference(name, run):
    """(best_makespan, best_rank, last_makespan, last_rank, info, trace, move_log) of the mirror for run `run` of case `name`, with
    the rank tensors, the steps, the until and the margin the backends are to be given; made once"""
    key = (name, run)
    if key not in _REFS:
        st = case_state(name)
        steps, until, margin, kind = RUNS[name][run]
        until, guide, host = until_of_run(name, until), guide_of_run(name, kind), st["host"]
        rank = T.cyclic_and_unfinished() if kind == "hand-source" else st["rank"]
        log = []
        ref = search.relink_reference(host["env_const"], host["ops"], rank, guide, steps, until, margin, fill=FILL, log=log)
        _REFS[key] = dict(rank=rank, guide=guide, steps=steps, until=until, margin=margin, ref=ref)
        _EVENTS[key] = log
    return _REFS[key]


def call_relink(be, env, rank, guide, steps, until, margin=0, want=OUTPUTS, desc=None):
    """jss_relink_walk through the backend's library: (rc, best_makespan, best_rank, last_makespan, last_rank, info, trace,
    move_log) as host arrays (None where not asked for); the outputs are prefilled (FILL), so what a call leaves alone can be told
    from what it writes"""
    lib = search.relink_library(be)
    B = env.batch
    with be.on_device():
        dev = lambda x: None if x is None else be.from_numpy(np.asarray(x, np.int32))   # noqa: E731
        full = lambda shape: be.from_numpy(np.full(shape, FILL, np.int32))   # noqa: E731
        rk, gd = dev(rank), dev(guide)
        unt = dev(until) if np.ndim(until) else None
        mk, best = full(B), full((B, env.jmax, env.mmax))
        last_mk = full(B) if "last_mk" in want else None
        last = full((B, env.jmax, env.mmax)) if "last" in want else None
        info = full((B, _abi.RELINK_NI)) if "info" in want else None
        trace = full((B, max(steps, 1))) if "trace" in want else None
        moved = full((B, max(steps, 1), 2)) if "log" in want else None
        p = be.ptr
        arg = _abi.JssRelink(steps, 0 if unt is not None else int(until), margin, p(rk), p(gd), p(unt), p(mk), p(best), p(last_mk),
                             p(last), p(info), p(trace), p(moved))
        rc = lib.jss_relink_walk(C.byref(env._desc if desc is None else desc), C.byref(env._state), C.byref(arg), be.stream())
        be.sync()
    host = lambda x: None if x is None else np.asarray(be.numpy(x))   # noqa: E731
    trace = None if trace is None else host(trace).reshape(-1)[:B * steps].reshape(B, steps)   # (rows of `steps` words)
    moved = None if moved is None else host(moved).reshape(-1)[:B * steps * 2].reshape(B, steps, 2)
    return rc, host(mk), host(best), host(last_mk), host(last), host(info), trace, moved


def same(got, ref, what):
    """a call's outputs against the mirror's seven, those asked for"""
    assert got[0] == 0, (what, got[0])
    assert got[1].dtype == np.int32 and np.array_equal(got[1], ref[0]), (what, "best_makespan", got[1], ref[0])
    assert np.array_equal(got[2], ref[1]), (what, "best_rank", got[2], ref[1])
    for k, label in ((3, "last_makespan"), (4, "last_rank"), (5, "info"), (6, "trace"), (7, "move_log")):
        if got[k] is not None:
            assert np.array_equal(got[k], ref[k - 1]), (what, label, got[k], ref[k - 1])


def case_against_mirror(be, name):
    """every run of the case against the mirror, with all optional outputs; on the small cases' run of 3 moves the optional outputs
    in every combination; refused, cyclic and never-reset rows keep their fill; the batch untouched"""
    st = case_state(name)
    env = env_on(be, name)
    before = rows_of(env)
    for run in range(len(RUNS[name])):
        r = reference(name, run)
        same(call_relink(be, env, r["rank"], r["guide"], r["steps"], r["until"], r["margin"]), r["ref"], (name, run))
        ref = r["ref"]
        dead = ref[0] < 0
        assert dead[st["B"] - 1] and ref[0][st["B"] - 1] == -1                                 # the env never reset
        for k in (1, 3, 5, 6):
            assert (ref[k][dead] == FILL).all() and not (ref[k][~dead] == FILL).any(), (name, run, k)
        assert (ref[4][dead, 1:] == 0).all() and np.array_equal(ref[4][dead, 0], ref[0][dead]) and np.array_equal(ref[2][dead], ref[0][dead])
    r = reference(name, 3 if name in SMALL else 0)                     # (the small cases' run of 3 moves: 32 calls stay cheap)
    assert not (r["ref"][0][0] < 0) and r["steps"] == (3 if name in SMALL else r["steps"])   # a walk on env 0
    for mask in (range(32) if name in SMALL else ()):
        want = tuple(w for bit, w in enumerate(OUTPUTS) if mask >> bit & 1)
        same(call_relink(be, env, r["rank"], r["guide"], r["steps"], r["until"], r["margin"], want=want), r["ref"], (name, want))
    after = rows_of(env)
    for k in before:
        assert np.array_equal(before[k], after[k]), (name, k)


def case_refused_rows(be):
    """a guide with a negative rank on a real operation (-1), a negative until (-1), a cyclic and an unfinished row as guides and
    as sources (-2, -1) next to walks: their rows keep the fill; rank=None on an env that has not finished is refused"""
    runs = RUNS["3x2"]
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    for kind, codes in (((ENOUGH, 0, 0, "negative"), [-1, 0, 0, -1]), ((ENOUGH, "bad", 0, "desc"), [-1, 0, 0, -1]),
                        ((ENOUGH, 0, 0, "hand"), [0, -2, -1, -1]), ((ENOUGH, 0, 0, "hand-source"), [0, -2, -1, -1])):
        r = reference("3x2", runs.index(kind))
        got = call_relink(be, env_on(be, "3x2"), r["rank"], r["guide"], r["steps"], r["until"], r["margin"])
        same(got, r["ref"], ("3x2", kind))
        for i, code in enumerate(codes):
            if code:
                assert got[1][i] == code and got[3][i] == code and got[5][i].tolist() == [code] + [0] * 7, (kind, i)
                assert all((got[k][i] == FILL).all() for k in (2, 4, 6, 7)), (kind, i)
            else:
                assert got[1][i] >= 0 and got[5][i, 0] in (1, 2) and not any((got[k][i] == FILL).any() for k in (2, 4)), (kind, i)
    fresh = make_env(be, "3x2")                                       # reset, nothing scheduled: the solution is unfinished
    guide = be.from_numpy(guide_of_run("3x2", "asc"))
    out = fresh.relink(None, guide)
    assert n(out[0]).tolist() == [-1] * 4 and n(out[2]).tolist() == [-1] * 4
    assert n(fresh.order_distance(None, guide)).tolist() == [-1] * 4


def what_the_cases_cover():
    """over all runs of all cases the references hold: a move without a sure candidate (fallbacks > 0) and candidates the screen
    did not pass; the stops 0, 1 and 2, the latter two at move 0 and in mid-walk; best_move == -1 (no eligible order), 0 and
    later; a refused and a cyclic row.  `retries` is reported: no known input has one."""
    seen = {k: 0 for k in ("fallback", "unsure", "stop0", "stop1_at_0", "stop1_mid", "stop2_at_0", "stop2_mid", "no_eligible", "best_at_0",
                           "best_later", "refused", "cyclic", "retries")}
    for name in RUNS:
        for run in range(len(RUNS[name])):
            r = reference(name, run)
            info, mk = r["ref"][4], r["ref"][0]
            alive = mk >= 0
            for _, _, kind in _EVENTS[(name, run)]:
                if kind in ("fallback", "unsure"):
                    seen[kind] += 1
            assert sum(1 for e in _EVENTS[(name, run)] if e[2] == "fallback") == info[alive, 6].sum()
            for s in (1, 2):
                seen[f"stop{s}_at_0"] += int(((info[:, 0] == s) & (info[:, 1] == 0) & alive).sum())
                seen[f"stop{s}_mid"] += int(((info[:, 0] == s) & (info[:, 1] > 0)).sum())
            seen["stop0"] += int(((info[:, 0] == 0) & alive).sum())
            seen["no_eligible"] += int(((info[:, 2] == -1) & alive).sum())
            seen["best_at_0"] += int(((info[:, 2] == 0) & alive).sum())
            seen["best_later"] += int((info[:, 2] > 0).sum())
            seen["refused"] += int((mk == -1).sum())
            seen["cyclic"] += int((mk == -2).sum())
            seen["retries"] += int(info[alive, 7].sum())
            assert not (info[:, 0] == 4).any()
    return seen


# ---- arrival ---------------------------------------------------------------------------------------------------------------------
def case_arrival(be, name, kind):
    """with steps >= dist0 and until = 0 every walk arrives: stop 1, moves == dist0, dist == 0, the last order the guide's
    normalised positions (tabu_blocks(guide, 0)'s best_rank) and its makespan evaluate_order(guide)'s"""
    env = env_on(be, name)
    st = case_state(name)
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    rank, guide = be.from_numpy(st["rank"]), be.from_numpy(guide_of_run(name, kind))
    best, best_rank, last, last_rank, info = (n(x) for x in env.relink(rank, guide))
    want_rank, want_mk = n(env.tabu_blocks(guide, 0)[1]), n(env.evaluate_order(guide))
    alive = best >= 0
    assert alive[0] and np.array_equal(alive, (n(env.evaluate_order(rank)) >= 0) & (want_mk >= 0))
    assert (info[alive, 0] == 1).all() and np.array_equal(info[alive, 1], info[alive, 3]) and (info[alive, 4] == 0).all()
    assert np.array_equal(last_rank[alive], want_rank[alive]) and np.array_equal(last[alive], want_mk[alive])
    assert (best[alive] <= np.minimum(last[alive], n(env.evaluate_order(rank))[alive])).all()
    assert np.array_equal(n(env.order_distance(rank, guide)), np.where(alive, info[:, 3], best))
    return info


# ---- replay: a walk checked without the mirror -----------------------------------------------------------------------------------
def inversions(mach, a, b):
    """the distance of two position tensors (J x M) by brute force: the pairs of one machine that they put the other way round"""
    flat_m, fa, fb = mach.reshape(-1), a.reshape(-1), b.reshape(-1)
    count = 0
    for x in range(flat_m.size):
        for y in range(x + 1, flat_m.size):
            if flat_m[x] == flat_m[y] and (fa[x] < fa[y]) != (fb[x] < fb[y]):
                count += 1
    return count


def pair_of(be, instance, source, guide):
    """a B = 1 env of `instance` and the two orders as (1, jmax, mmax) rank tensors: rule names are rolled out, arrays are taken
    as they are"""
    if isinstance(source, str):
        env = K.rolled_out(be, instance, source)
        src = np.asarray(be.numpy(env.solution)).copy()
        gd = np.asarray(be.numpy(K.rolled_out(be, instance, guide).solution)).copy()
    else:
        env = BatchedJssEnv(instance, batch=1, _backend=be)
        env.reset()
        src, gd = np.asarray(source, np.int32)[None], np.asarray(guide, np.int32)[None]
    return env, np.ascontiguousarray(src, np.int32), np.ascontiguousarray(gd, np.int32)


def case_replay(be, instance, source, guide, margin=0):
    """a walk to arrival, replayed on the host from its move log: see the asserts"""
    env, src, gd = pair_of(be, instance, source, guide)
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    host = K.host_tables(env)
    J, M = int(host["env_const"][0, _abi.C_JOBS]), int(host["env_const"][0, _abi.C_MACHINES])
    mach = (host["ops"][0, :J, :M] >> 16) & 63
    mmax = env.mmax
    dist0 = int(n(env.order_distance(src, gd))[0])
    assert dist0 == int(n(env.order_distance(gd, src))[0])                                  # symmetric
    rank0, guide0 = n(env.tabu_blocks(src, 0)[1]), n(env.tabu_blocks(gd, 0)[1])             # both as positions
    assert dist0 == inversions(mach, rank0[0, :J, :M], guide0[0, :J, :M])
    best, best_rank, last, last_rank, info, trace, moved = (n(x) for x in env.relink(src, gd, dist0, 0, margin, trace=True, log=True))
    stop, moves, best_move, d0, dist, candidates, fallbacks, retries = (int(x) for x in info[0])
    assert (stop, moves, d0, dist) == (1, dist0, dist0, 0) and candidates >= moves and trace.shape == (1, dist0)
    orders = {int(m): sorted((int(j) * mmax + int(k) for j, k in np.argwhere(mach == m)), key=lambda e: rank0[0].reshape(-1)[e])
              for m in np.unique(mach)}
    g = guide0[0].reshape(-1)

    def positions():
        pos = np.full((1, env.jmax, env.mmax), -1, np.int32)
        for order in orders.values():
            for at, e in enumerate(order):
                pos[0, e // mmax, e % mmax] = at
        return pos

    start = int(n(env.evaluate_order(src))[0])
    for t in range(moves):
        u, v = (int(x) for x in moved[0, t])
        order = orders[int(mach[u // mmax, u % mmax])]
        at = order.index(u)
        assert order[at + 1] == v and g[u] > g[v], t                 # adjacent on the machine, inverted with respect to the guide
        order[at], order[at + 1] = v, u
        assert n(env.evaluate_order(positions()))[0] == trace[0, t], t
        if t + 1 == best_move:
            assert np.array_equal(positions(), best_rank)
    assert np.array_equal(positions(), last_rank) and np.array_equal(last_rank, guide0)
    assert last[0] == (trace[0, -1] if moves else start) == n(env.evaluate_order(gd))[0]
    # the best: the first minimum of the eligible part of [source] + trace
    seen = np.concatenate(([start], trace[0]))
    eligible = [t for t in range(moves + 1) if t >= margin and dist0 - t >= margin]
    if eligible:
        low = min(seen[t] for t in eligible)
        assert best[0] == low and best_move == next(t for t in eligible if seen[t] == low)
        assert n(env.evaluate_order(best_rank))[0] == best[0]
    else:
        assert best_move == -1 and best[0] == last[0] and np.array_equal(best_rank, last_rank)
    # a shorter walk is a prefix
    half = [n(x) for x in env.relink(src, gd, moves // 2, 0, margin, trace=True, log=True)]
    assert np.array_equal(half[5][0], trace[0, :moves // 2]) and np.array_equal(half[6][0], moved[0, :moves // 2])
    assert half[4][0, :2].tolist() == ([0, moves // 2] if moves else [1, 0]) and half[4][0, 4] == dist0 - moves // 2
    return info[0], seen


# ---- the anchors -----------------------------------------------------------------------------------------------------------------
def case_anchor(be, key, mirror=False):
    """B = 1 between two rule rollouts: the listed distance, makespans of both ends, the lowest on the path and its move, the
    highest; no fallback; with `mirror` the NumPy mirror gives the same seven outputs"""
    env, src, gd = pair_of(be, *key)
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    dist0 = ANCHORS[key][0]
    out = [n(x) for x in env.relink(src, gd, dist0, 0, 0, trace=True, log=True)]
    best, _, last, _, info, trace, _ = out
    seen = np.concatenate(([n(env.evaluate_order(src))[0]], trace[0]))
    assert (int(info[0, 3]), int(seen[0]), int(last[0]), int(best[0]), int(info[0, 2]), int(seen.max())) == ANCHORS[key]
    assert info[0].tolist()[:2] == [1, dist0] and info[0].tolist()[4] == 0 and info[0].tolist()[6:] == [0, 0]
    assert int(np.argmin(seen)) == info[0, 2] and seen.min() == best[0]
    if mirror:
        host = K.host_tables(env)
        ref = search.relink_reference(host["env_const"], host["ops"], src, gd, dist0, 0)
        for got, want in zip(out, ref):
            assert np.array_equal(got, want)


def case_hand_walks(be, mirror=False):
    """the hand case both ways: the listed distance, makespans, fallbacks, retries and candidates"""
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    for way, (src, gd) in (("forward", (HAND_SOURCE, HAND_GUIDE)), ("back", (HAND_GUIDE, HAND_SOURCE))):
        env, src, gd = pair_of(be, hand_instance(), src, gd)
        dist0, makespans, fallbacks, retries, candidates = HAND_WALKS[way]
        out = [n(x) for x in env.relink(src, gd, None, 0, 0, trace=True, log=True)]
        runs = [out] if not mirror else [out, search.relink_reference(K.host_tables(env)["env_const"], K.host_tables(env)["ops"], src, gd,
                                                                      _abi.RELINK_MAX_STEPS, 0)]
        for best, _, last, _, info, trace, _ in runs:
            assert info[0].tolist() == [1, dist0, int(np.argmin(makespans)), dist0, 0, candidates, fallbacks, retries], (way, info)
            assert [n(env.evaluate_order(src))[0]] + trace[0, :dist0].tolist() == makespans and (trace[0, dist0:] == -1).all()
            assert best[0] == min(makespans) and last[0] == makespans[-1]
        if mirror:
            for got, want in zip(*runs):
                assert np.array_equal(got, want)


def case_retry(be, mirror=False):
    """the walk that swaps a candidate back: it arrives, with one retry on a move without a sure candidate"""
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    env, src, gd = pair_of(be, retry_instance(), RETRY_SOURCE, RETRY_GUIDE)
    out = [n(x) for x in env.relink(src, gd, None, 0, 0, trace=True, log=True)]
    info = out[4][0]
    assert info[0] == 1 and info[1] == info[3] > 0 and info[4] == 0 and info[6] >= 1 and info[7] == 1, info
    assert np.array_equal(out[3], n(env.tabu_blocks(gd, 0)[1])) and out[2][0] == n(env.evaluate_order(gd))[0]
    if mirror:
        host = K.host_tables(env)
        log = []
        ref = search.relink_reference(host["env_const"], host["ops"], src, gd, _abi.RELINK_MAX_STEPS, 0, log=log)
        for got, want in zip(out, ref):
            assert np.array_equal(got, want)
        assert sum(1 for e in log if e[2] == "retry") == 1


# ---- a seeded search for a retry ------------------------------------------------------------------------------------------------
def random_instance(rng):
    """2-6 jobs x 2-5 machines; machines may repeat within a job; durations from {0, 1} up to 1-99"""
    J, M = int(rng.integers(2, 7)), int(rng.integers(2, 6))
    if rng.random() < 0.5:
        machine = np.stack([rng.permutation(M) for _ in range(J)])
    else:
        machine = rng.integers(0, M, (J, M))
    top = int(rng.choice([1, 1, 2, 3, 9, 99]))
    duration = rng.integers(0 if top <= 3 or rng.random() < 0.5 else 1, top + 1, (J, M))
    duration[0, 0] = max(1, duration[0, 0])                           # (an instance has some work)
    return inst_with_zeros("random", machine, duration)


def random_order(rng, J, M):
    """a machine order that has a schedule: the ranks of a random interleaving of the job chains"""
    chains = rng.permutation(np.repeat(np.arange(J), M))
    rank = np.zeros((J, M), np.int32)
    k = np.zeros(J, np.int64)
    for at, j in enumerate(chains):
        rank[j, k[j]] = at
        k[j] += 1
    return rank


def case_seeded_search(be, walks, seed=2024, every=50):
    """`walks` random tiny walks to arrival; the twin against the mirror on every `every`th; returns the summed info rows and the
    instances of walks with a retry"""
    rng = np.random.default_rng(seed)
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    total, with_retry = np.zeros(_abi.RELINK_NI, np.int64), []
    for w in range(walks):
        inst = random_instance(rng)
        J, M = inst.machine.shape
        src, gd = random_order(rng, J, M)[None], random_order(rng, J, M)[None]
        env = BatchedJssEnv(inst, batch=1, _backend=be)
        env.reset()
        out = [n(x) for x in env.relink(src, gd, None, 0, 0, trace=w % every == 0, log=w % every == 0)]
        best, best_rank, last, last_rank, info = out[:5]
        assert info[0, 0] == 1 and info[0, 1] == info[0, 3] and info[0, 4] == 0, (w, info)
        assert np.array_equal(last_rank, n(env.tabu_blocks(gd, 0)[1])) and last[0] == n(env.evaluate_order(gd))[0], w
        total += info[0]
        if info[0, 7]:
            with_retry.append((inst, src, gd))
        if w % every == 0:
            host = K.host_tables(env)
            ref = search.relink_reference(host["env_const"], host["ops"], src, gd, _abi.RELINK_MAX_STEPS, 0)
            for got, want in zip(out, ref):
                assert np.array_equal(got, want), w
    return total, with_retry


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def definition_loop(be, instances, kind, walkers, iters, rounds, share, tenure, explore, seed, target, reach):
    """search.relink_search written with the public calls, on the host: returns (makespan, walker, rank, start, optimal,
    best_makespan, info, history, distance)"""
    names = instances if isinstance(instances, list) else [instances]
    G, W = len(names), walkers
    if G == 1:
        env = BatchedJssEnv(names[0], batch=W, seed=seed, _backend=be)
    else:
        env = BatchedJssEnv(names, batch=G * W, table_of_env=np.repeat(np.arange(G), W), order="interleaved", seed=seed, _backend=be)
    n = lambda x: np.asarray(be.numpy(x)).copy()   # noqa: E731
    env.reset()
    tgt = n(env.lower_bound()) if target == "lower_bound" else None if target is None else np.repeat(np.asarray(target, np.int32), W)
    env.rollout(kind, n_iter=3 * env.jmax * env.mmax, autoreset=False, explore=explore, seed=seed)
    lo, hi = tenure
    ten = np.array([lo + w % (hi - lo + 1) for _ in range(G) for w in range(W)], np.int32)
    mk, best_rank, info = (n(x) for x in env.tabu_blocks(None, iters, ten, tgt, reach))

    def lowest():
        return [min((int(mk[g * W + w]), w) for w in range(W) if mk[g * W + w] >= 0) for g in range(G)]

    history, distance = [[low[0] for low in lowest()]], []
    for _ in range(rounds):
        elite = [g * W + low[1] for g, low in enumerate(lowest())]
        guide = np.stack([best_rank[elite[i // W]] for i in range(G * W)])
        d = n(env.order_distance(best_rank, guide))
        assert (d >= 0).all() and all(d[e] == 0 for e in elite)
        until = np.array([int(x) - int(x) * share[0] // share[1] for x in d], np.int32)
        if tgt is not None:
            until = np.where(mk <= tgt, d, until).astype(np.int32)
        last_rank = n(env.relink(best_rank, guide, until=until)[3])
        new, new_rank, new_info = (n(x) for x in env.tabu_blocks(last_rank, iters, ten, tgt, reach))
        for i in range(G * W):
            if new[i] < mk[i]:
                mk[i], best_rank[i], info[i] = new[i], new_rank[i], new_info[i]
        history.append([low[0] for low in lowest()])
        distance.append(d)
    makespan, walker = [low[0] for low in lowest()], [low[1] for low in lowest()]
    winner = np.array([g * W + w for g, w in enumerate(walker)], np.int32)
    again, start = (n(x) for x in env.evaluate_order(best_rank, winner, start=True))
    assert again.tolist() == makespan
    optimal = [bool(info[i, 0] == 1 or (tgt is not None and mk[i] <= tgt[i])) for i in winner]
    return (np.array(makespan), np.array(walker), best_rank[winner], start, np.array(optimal), mk, info,
            np.array(history).T.reshape(G, rounds + 1), np.array(distance).T.reshape(G * W, rounds))


FIELDS = ("makespan", "walker", "rank", "start", "optimal", "best_makespan", "info")


def case_driver(be, instances, kind="SPT", walkers=4, iters=30, rounds=2, share=(1, 2), tenure=(5, 12), explore=0.1, seed=0,
                target="lower_bound", reach=0):
    want = definition_loop(be, instances, kind, walkers, iters, rounds, share, tenure, explore, seed, target, reach)
    res = search.relink_search(instances, kind, walkers, iters, rounds, share, tenure, explore, seed, target, reach, _backend=be)
    for label, w in zip(FIELDS + ("history", "distance"), want):
        assert np.array_equal(getattr(res, label), w), (label, getattr(res, label), w)
    G = len(res.makespan)
    assert res.history.shape == (G, rounds + 1) and res.distance.shape == (G * walkers, rounds) and res.history.dtype == np.int32
    assert (np.diff(res.history, axis=1) <= 0).all() and np.array_equal(res.history[:, -1], res.makespan)   # it never rises
    assert np.array_equal(res.makespan, res.best_makespan.reshape(G, walkers).min(axis=1)) and res.info.shape == (G * walkers, _abi.BLOCK_NI)
    return res


def case_driver_rounds_0(be, instances, **kw):
    """rounds = 0 is tabu_search(moves="block"), field for field"""
    a = search.relink_search(instances, rounds=0, _backend=be, **kw)
    b = search.tabu_search(instances, moves="block", _backend=be, **kw)
    for label in FIELDS + ("target", "tenure"):
        x, y = getattr(a, label), getattr(b, label)
        assert (x is None and y is None) or np.array_equal(x, y), label
    assert a.history.shape == (len(a.makespan), 1) and np.array_equal(a.history[:, 0], a.makespan) and a.distance.shape[1] == 0


# ---- ABI errors ------------------------------------------------------------------------------------------------------------------
def case_abi_errors(be):
    """every code of jss_relink_walk, before anything runs: the outputs keep their fill"""
    lib = search.relink_library(be)
    env = K.env_on(be, "3x2")
    st = K.case_state("3x2")
    B = env.batch
    with be.on_device():
        rank, guide = be.from_numpy(st["rank"]), be.from_numpy(guide_of_run("3x2", "asc"))
        unt = be.from_numpy(np.full(B, 1, np.int32))
        out = {k: be.from_numpy(np.full(s, FILL, np.int32)) for k, s in (("best_makespan", B), ("best_rank", (B, env.jmax, env.mmax)),
                                                                         ("last_makespan", B), ("last_rank", (B, env.jmax, env.mmax)),
                                                                         ("info", (B, _abi.RELINK_NI)), ("trace", (B, 5)),
                                                                         ("move_log", (B, 5, 2)))}
    p = be.ptr

    def call(desc=None, state=True, arg=True, **fields):
        d = _abi.JssDesc.from_buffer_copy(env._desc)
        for k, v in ({} if desc in (None, "null") else desc).items():
            setattr(d, k, v)
        t = _abi.JssRelink(5, 0, 0, p(rank), p(guide), p(unt), p(out["best_makespan"]), p(out["best_rank"]), p(out["last_makespan"]),
                           p(out["last_rank"]), p(out["info"]), p(out["trace"]), p(out["move_log"]))
        for k, v in fields.items():
            setattr(t, k, v)
        rc = lib.jss_relink_walk(C.byref(d) if desc != "null" else None, C.byref(env._state) if state else None,
                                 C.byref(t) if arg else None, be.stream())
        be.sync()
        return rc

    assert call(desc="null") == _abi.E_NULL and call(state=False) == _abi.E_NULL and call(arg=False) == _abi.E_NULL
    assert call(rank=None) == _abi.E_NULL and call(guide=None) == _abi.E_NULL
    assert call(best_makespan=None) == _abi.E_NULL and call(best_rank=None) == _abi.E_NULL
    assert call(desc={"ops": None}) == _abi.E_NULL
    assert call(steps=-1) == _abi.E_SHAPE and call(steps=65537) == _abi.E_SHAPE
    assert call(until=-1) == _abi.E_SHAPE and call(until=-1, until_of=None) == _abi.E_SHAPE and call(margin=-1) == _abi.E_SHAPE
    assert call(desc={"jmax": 0}) == _abi.E_SHAPE and call(desc={"mmax": 65}) == _abi.E_SHAPE and call(desc={"batch": -1}) == _abi.E_SHAPE
    assert call(desc={"kernel": 64}) == _abi.E_KIND
    # a row of more than 3584 entries does not fit one walker's 64 KB of LDS: both libraries say so; 128 x 28 fits (not run)
    assert call(desc={"jmax": 128, "mmax": 64}) == _abi.E_LDS and call(desc={"jmax": 128, "mmax": 29}) == _abi.E_LDS
    assert call(desc={"jmax": 128, "mmax": 28, "batch": 0}) == 0 and call(desc={"batch": 0}) == 0      # batch == 0 launches nothing
    for k, v in out.items():
        assert (np.asarray(be.numpy(v)) == FILL).all(), k
    # the optional pointers may all be NULL; steps and margin at their bounds
    assert call(steps=0, until_of=None, last_makespan=None, last_rank=None, info=None, trace=None, move_log=None) == 0
    assert call(margin=2 ** 31 - 1, until=2 ** 31 - 1, until_of=None) == 0 and call(steps=1) == 0
    assert not (np.asarray(be.numpy(out["best_makespan"])) == FILL).any()


# ---- the built library ------------------------------------------------------------------------------------------------------------
def relink_kernel_rows():
    """[(name, vgprs, sgprs, spilled vgprs, spilled sgprs, scratch bytes, static LDS bytes)] of libjss_relink_hip.so"""
    import re
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import LLVM, kernel_resources
    from jssenv_amd.build import build_relink_extension
    so = build_relink_extension()                                     # (built here if build() has not run)
    rows = kernel_resources(so)
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "relink.co")
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", so, fat], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    lds = [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", notes)]
    assert len(lds) == len(rows)
    return [r + (b,) for r, b in zip(rows, lds)]
