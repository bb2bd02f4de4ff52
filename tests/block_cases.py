"""Backend-agnostic cases of jss_block_search (include/jss_block.h), BatchedJssEnv.tabu_blocks and search.tabu_search(moves="block"),
run against the host-core twin, the kernel source (jssenv_amd/csrc/jss_block.hip) under the SIMT emulator and the HIP library
libjss_block_hip.so.

The reference is search.block_reference (NumPy, written from the header's definition on top of order_eval_reference).  The batches
and the rank tensors are order_cases'; a hand instance adds a critical block of four operations.  A run's reference is made once and
shared by the three backends, which are compared with it bit for bit in all six outputs."""
import ctypes as C
import os
import subprocess

import numpy as np

import order_cases as K
import tabu_cases as T
from clone_cases import rows_of
from jssenv_amd import BatchedJssEnv, _abi, search

ROOT = K.ROOT
BLOCK_SRC = os.path.join(ROOT, "jssenv_amd", "csrc", "jss_block.hip")
EMU_LIB = os.path.join(K.EMU, "libjss_block_emu.so")
FILL = K.FILL                       # what the outputs hold before a call: the rows of refused and cyclic walkers keep it
OUTPUTS = ("last", "info", "trace", "log")

# B = 1, start rollout(kind): (instance, kind, tenure, iters) -> (start, best, at move, evaluations)
ANCHORS = {("ta01", "SPT", 8, 300): (1462, 1314, 245, 4900), ("ta01", "SPT", 3, 64): (1462, 1361, 50, 1149),
           ("ta41", "SPT", 8, 200): (2499, 2325, 170, 5503)}
# the swap walk's anchors (tabu_cases.ANCHORS) that the block walk is held against, with as many moves as the swap walk spent
# re-timings (its evaluations and its moves, less the one of the start that both walks make): key -> (moves, the block walk's best)
EARNS = {("ta01", "SPT", 8, 300): (4394, 1258), ("ta41", "SPT", 8, 200): (8307, 2276)}


def build_emu_block():
    """jss_block.hip, unmodified, compiled with g++ against the SIMT emulator's hip_runtime.h: a library of its own"""
    deps = [BLOCK_SRC, os.path.join(K.EMU, "hip", "hip_runtime.h"), os.path.join(ROOT, "include", "jss_block.h"),
            os.path.join(ROOT, "include", "jss_tabu.h"), os.path.join(ROOT, "include", "jss_order.h"),
            os.path.join(ROOT, "jssenv_amd", "csrc", "jss_abi_checks.hpp")]
    if not os.path.isfile(EMU_LIB) or any(os.path.getmtime(d) > os.path.getmtime(EMU_LIB) for d in deps):
        tmp = EMU_LIB + f".tmp{os.getpid()}"
        subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
                               "-Wno-unknown-pragmas", "-I" + K.EMU, "-I" + os.path.join(ROOT, "include"), BLOCK_SRC, "-o", tmp])
        os.replace(tmp, EMU_LIB)
    return EMU_LIB


def emu_backend():
    """tabu_cases' emulator backend (the env kernels, jss_order.hip, jss_tabu.hip) with the emulated block library as its `block_lib`"""
    be = T.emu_backend()
    be.block_lib = _abi.bind_block(C.CDLL(build_emu_block()))
    return be


twin_backend = K.twin_backend


# ---- the hand instances ----------------------------------------------------------------------------------------------------------
# A batch of the same layout as order_cases' (the last env never reset), 4 x 3, for what the walks of order_cases' batches may not
# meet (what_the_cases_cover counts it): four jobs that all open on machine 0, which from the order by job index is one critical
# block of four operations, with short followers so that far moves survive the screen.
HAND = {
    "chain": (lambda be: BatchedJssEnv(K.inst("chain", [[0, 1, 2], [0, 2, 1], [0, 1, 2], [0, 2, 1]],
                                              [[9, 1, 1], [2, 1, 1], [3, 1, 1], [8, 2, 1]]), batch=3, _backend=be, seed=17), 3),
}
CASES = dict(K.CASES, **HAND)
_HAND_STATES = {}


def make_env(be, name):
    if name in K.CASES:
        return K.make_env(be, name)
    make, B = HAND[name]
    env = make(be)
    which = np.ones(B, np.uint8)
    which[B - 1] = 0
    env.reset(which=which)
    return env


def case_state(name):
    """order_cases.case_state for its cases; for a hand batch the same keys the runs need: env 0 ordered by job index on every
    machine, env 1 by job index descending, the env never reset a copy of env 0's"""
    if name in K.CASES:
        return K.case_state(name)
    if name not in _HAND_STATES:
        be = twin_backend()
        env = make_env(be, name)
        B = HAND[name][1]
        jobs = np.arange(env.jmax, dtype=np.int32)[:, None] * np.ones((1, env.mmax), np.int32)
        rank = np.stack([jobs, env.jmax - 1 - jobs, jobs]).astype(np.int32)
        _HAND_STATES[name] = dict(env=env, host=K.host_tables(env), rank=np.ascontiguousarray(rank), B=B)
    return _HAND_STATES[name]


def env_on(be, name):
    return case_state(name)["env"] if be is twin_backend() else make_env(be, name)


# ---- the runs ------------------------------------------------------------------------------------------------------------------
# Per case: (iters, tenure, target, reach); tenure and target as in tabu_cases.RUNS.  The small cases run the tenures 0, 2 and 64
# with the reaches 0, 1 and 2, the others one launch with a tenure per walker, at the move counts that keep a reference at a few
# seconds.
TENURES = T.TENURES
SMALL = ("1x2", "3x2", "repeats", "per-env", "chain")
RUNS = {
    "1x2": [(6, 0, None, 0), (6, 2, None, 1), (6, 64, None, 2), (6, "each", None, 0), (6, 2, "best", 0), (0, 2, None, 0)],
    "3x2": [(20, 0, None, 0), (20, 2, None, 1), (20, 64, None, 2), (20, "each", None, 0), (20, 2, "best", 0), (20, "bad", "never", 0),
            (0, 64, "best", 0)],
    "repeats": [(24, 0, None, 0), (24, 2, None, 1), (24, 64, None, 2), (24, "each", "best", 0), (0, 0, None, 0)],
    "per-env": [(16, 0, None, 0), (16, 2, None, 1), (16, 64, None, 2), (16, "each", None, 0), (16, "each", "best", 0)],
    "table-of-env": [(10, "each", None, 0), (10, "each", None, 2)],
    "by-shape": [(6, "each", None, 0)],
    "J65": [(40, "each", None, 0), (40, "each", None, 1)],
    "ta01": [(40, "each", None, 0), (40, 2, "best", 0), (40, "each", None, 2), (40, 64, None, 1)],
    "100x20": [(3, "each", None, 0)],
    "chain": [(12, 0, None, 0), (12, 2, None, 1), (12, 64, None, 2), (12, 3, "best", 0)],
}
_REFS = {}
_EVENTS = {}


def tenure_of_run(name, tenure):
    B = CASES[name][1]
    if tenure == "each":
        return np.array([TENURES[i % len(TENURES)] for i in range(B)], np.int32)
    if tenure == "bad":
        return np.array([65, -1] + [TENURES[i % len(TENURES)] for i in range(2, B)], np.int32)
    return int(tenure)


def runs_of(name):
    return list(range(len(RUNS[name]))) + (["hand"] if name == "3x2" else [])


def reference(name, run):
    """(best_makespan, best_rank, last_rank, info, trace, move_log) of the mirror for run `run` of case `name`, with the rank tensor,
    the tenure, the target and the reach the backends are to be given; made once"""
    key = (name, run)
    if key in _REFS:
        return _REFS[key]
    st = case_state(name)
    rank = T.cyclic_and_unfinished() if run == "hand" else st["rank"]
    iters, tenure, target, reach = (12, 2, None, 0) if run == "hand" else RUNS[name][run]
    tenure = tenure_of_run(name, tenure)
    host = st["host"]
    if target == "best":
        free = search.block_reference(host["env_const"], host["ops"], rank, iters, tenure, None, reach, fill=FILL)
        starts = search.order_eval_reference(host["env_const"], host["ops"], rank)[0]
        target = np.where(np.arange(st["B"]) % 2 == 1, starts, free[0]).astype(np.int32)
    elif target == "never":
        target = np.zeros(st["B"], np.int32)
    log = []
    ref = search.block_reference(host["env_const"], host["ops"], rank, iters, tenure, target, reach, fill=FILL, log=log)
    _REFS[key] = dict(rank=rank, iters=iters, tenure=tenure, target=target, reach=reach, ref=ref)
    _EVENTS[key] = log
    return _REFS[key]


def call_block(be, env, rank, iters, tenure, target=None, reach=0, want=OUTPUTS, desc=None):
    """jss_block_search through the backend's library: (rc, best_makespan, best_rank, last_rank, info, trace, move_log) as host
    arrays (None where not asked for); the outputs are prefilled (FILL), so what a call leaves alone can be told from what it writes"""
    lib = search.block_library(be)
    B = env.batch
    with be.on_device():
        dev = lambda x: None if x is None else be.from_numpy(np.asarray(x, np.int32))   # noqa: E731
        full = lambda shape: be.from_numpy(np.full(shape, FILL, np.int32))   # noqa: E731
        rk = dev(rank)
        ten = dev(tenure) if np.ndim(tenure) else None
        tgt = dev(target)
        mk, best = full(B), full((B, env.jmax, env.mmax))
        last = full((B, env.jmax, env.mmax)) if "last" in want else None
        info = full((B, _abi.BLOCK_NI)) if "info" in want else None
        trace = full((B, max(iters, 1))) if "trace" in want else None
        moved = full((B, max(iters, 1), 2)) if "log" in want else None
        p = be.ptr
        arg = _abi.JssBlock(iters, 0 if ten is not None else int(tenure), reach, p(rk), p(ten), p(tgt), p(mk), p(best), p(last), p(info),
                            p(trace), p(moved))
        rc = lib.jss_block_search(C.byref(env._desc if desc is None else desc), C.byref(env._state), C.byref(arg), be.stream())
        be.sync()
    host = lambda x: None if x is None else np.asarray(be.numpy(x))   # noqa: E731
    trace = None if trace is None else host(trace).reshape(-1)[:B * iters].reshape(B, iters)   # (rows of `iters` words)
    moved = None if moved is None else host(moved).reshape(-1)[:B * iters * 2].reshape(B, iters, 2)
    return rc, host(mk), host(best), host(last), host(info), trace, moved


def same(got, ref, what):
    """a call's outputs against the mirror's (best_makespan, best_rank, last_rank, info, trace, move_log), those asked for"""
    assert got[0] == 0, (what, got[0])
    assert got[1].dtype == np.int32 and np.array_equal(got[1], ref[0]), (what, "best_makespan", got[1], ref[0])
    assert np.array_equal(got[2], ref[1]), (what, "best_rank")
    for k, label in ((3, "last_rank"), (4, "info"), (5, "trace"), (6, "move_log")):
        if got[k] is not None:
            assert np.array_equal(got[k], ref[k - 1]), (what, label, got[k], ref[k - 1])


def case_against_mirror(be, name):
    """every run of the case against the mirror, with all optional outputs; on the small cases' first run the optional outputs in
    every combination; refused rows keep their fill; the batch untouched"""
    st = case_state(name)
    env = env_on(be, name)
    before = rows_of(env)
    for run in runs_of(name):
        r = reference(name, run)
        same(call_block(be, env, r["rank"], r["iters"], r["tenure"], r["target"], r["reach"]), r["ref"], (name, run))
    r = reference(name, 0)
    for mask in (range(16) if name in SMALL else ()):
        want = tuple(w for bit, w in enumerate(OUTPUTS) if mask >> bit & 1)
        same(call_block(be, env, r["rank"], r["iters"], r["tenure"], r["target"], r["reach"], want=want), r["ref"], (name, want))
    ref = r["ref"]
    dead = ref[0] < 0
    assert dead[st["B"] - 1] and ref[0][st["B"] - 1] == -1 and not dead[0]                 # the env never reset; a walk
    for k in (1, 2, 4, 5):
        assert (ref[k][dead] == FILL).all() and not (ref[k][~dead] == FILL).any(), (name, k)
    assert (ref[3][dead, 1:] == 0).all() and np.array_equal(ref[3][dead, 0], ref[0][dead])
    after = rows_of(env)
    for k in before:
        assert np.array_equal(before[k], after[k]), (name, k)


def case_hand_rows(be):
    """a cyclic rank (-2) and an unfinished solution (-1) next to a walk: their rows keep the fill"""
    r = reference("3x2", "hand")
    got = call_block(be, K.env_on(be, "3x2"), r["rank"], r["iters"], r["tenure"], r["target"], r["reach"])
    same(got, r["ref"], "hand")
    assert got[1][0] > 0 and got[1][1:].tolist() == [-2, -1, -1]
    assert got[4][1:].tolist() == [[-2] + [0] * 7, [-1] + [0] * 7, [-1] + [0] * 7]
    for k in (2, 3, 5, 6):
        assert (got[k][1:] == FILL).all() and not (got[k][0] == FILL).any()


def what_the_cases_cover():
    """over all runs of all cases the references hold: an F and a B move of distance >= 2 taken; a candidate screened for each of
    the three reasons, the job's own operation in the way on "repeats"; a tabu move taken by aspiration and a forced one; the stops
    0, 1, and 2 at move 0 and in mid-walk; a candidate that reach cut; a refused and a cyclic row, a refused tenure"""
    seen = {k: 0 for k in ("F far", "B far", "job", "job on repeats", "successor", "predecessor", "aspired", "forced", "reach", "stop0",
                           "stop1", "stop2_at_0", "stop2_mid", "refused", "cyclic", "bad_tenure")}
    for name in RUNS:
        for run in runs_of(name):
            r = reference(name, run)
            info, mk = r["ref"][3], r["ref"][0]
            for _, _, kind in _EVENTS[(name, run)]:
                seen[kind] += 1
                if kind == "job" and name == "repeats":
                    seen["job on repeats"] += 1
            seen["stop1"] += int((info[:, 0] == 1).sum())
            seen["stop2_at_0"] += int(((info[:, 0] == 2) & (info[:, 1] == 0)).sum())
            seen["stop2_mid"] += int(((info[:, 0] == 2) & (info[:, 1] > 0)).sum())
            seen["stop0"] += int(((info[:, 0] == 0) & (mk >= 0)).sum())
            seen["refused"] += int((mk == -1).sum())
            seen["cyclic"] += int((mk == -2).sum())
            if np.ndim(r["tenure"]):
                seen["bad_tenure"] += int((((r["tenure"] < 0) | (r["tenure"] > 64)) & (mk == -1))[:-1].sum())
    return seen


# ---- replay: a walk checked without the mirror -------------------------------------------------------------------------------------
def apply_move(order, x, y):
    """the machine's order (a list of flat indices) with x carried right behind y, or right before y: whichever side y is on"""
    at, to = order.index(x), order.index(y)
    order.insert(to, order.pop(at))


def case_replay(be, instance, kind, iters, tenure, reach=0):
    """a walk from a finished `kind` rollout, replayed on the host from its move log: see the asserts"""
    env = K.rolled_out(be, instance, kind)
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    host = K.host_tables(env)
    J, M = int(host["env_const"][0, _abi.C_JOBS]), int(host["env_const"][0, _abi.C_MACHINES])
    mach, dur = (host["ops"][0, :J, :M] >> 16) & 63, host["ops"][0, :J, :M] & 0xFFFF
    mmax = env.mmax
    start = int(n(env.evaluate_order())[0])
    mk, best_rank, info, trace, last_rank, moved = (n(x) for x in env.tabu_blocks(None, iters, tenure, None, reach, trace=True, last=True, log=True))
    stop, moves, best_move, evaluations, screened, far, hits, zero = (int(x) for x in info[0])
    assert stop == 0 and moves == iters and evaluations >= moves and zero == 0 and 0 <= hits <= moves and 0 <= far <= moves
    assert trace.shape == (1, iters) and (trace > 0).all() and moved.shape == (1, iters, 2)
    # iters = 0: the plain evaluation, best_rank the normalised order: the replay's start
    mk0, rank0, info0 = (n(x) for x in env.tabu_blocks(None, 0, tenure, None, reach))
    assert mk0[0] == start and info0[0].tolist() == [0] * 8 and n(env.evaluate_order(rank0))[0] == start
    assert np.array_equal(n(env.evaluate_order(rank0, start=True)[1]), n(env.evaluate_order(start=True)[1]))
    orders = {int(m): sorted((int(j) * mmax + int(k) for j, k in np.argwhere(mach == m)), key=lambda e: rank0[0].reshape(-1)[e])
              for m in np.unique(mach)}

    def positions():
        pos = np.full((1, env.jmax, env.mmax), -1, np.int32)
        for order in orders.values():
            for at, e in enumerate(order):
                pos[0, e // mmax, e % mmax] = at
        return pos

    distances = []
    for t in range(iters):
        x, y = (int(v) for v in moved[0, t])
        assert mach.reshape(-1)[x // mmax * M + x % mmax] == mach.reshape(-1)[y // mmax * M + y % mmax] and x // mmax != y // mmax
        if reach == 1:                                               # a block-end swap: one of the pairs of this order
            _, pa, pb, found = (n(v) for v in env.evaluate_order(positions(), pairs=128))
            pairs = {frozenset((int(a), int(b))) for a, b in zip(pa[0, :found[0]], pb[0, :found[0]])}
            assert found[0] <= 128 and frozenset((x, y)) in pairs, t
        order = orders[int(mach.reshape(-1)[x // mmax * M + x % mmax])]
        distances.append(abs(order.index(x) - order.index(y)))
        apply_move(order, x, y)
        assert n(env.evaluate_order(positions()))[0] == trace[0, t], t
        if t + 1 == best_move:
            assert np.array_equal(positions(), best_rank)
    assert np.array_equal(positions(), last_rank)
    assert far == sum(d >= 2 for d in distances) and (reach == 0 or max(distances) <= reach)
    # either rank reproduces its schedule; the best one's start times are a feasible schedule of that length
    again, times = (n(x) for x in env.evaluate_order(best_rank, start=True))
    assert again[0] == mk[0] and K.feasible(times[0], mach, dur) == mk[0]
    # positions: on every machine 0 ... count - 1, -1 in the padding
    for r in (best_rank[0], last_rank[0]):
        assert (r[J:] == -1).all() and (r[:, M:] == -1).all()
        for m in np.unique(mach):
            assert sorted(r[:J, :M][mach == m].tolist()) == list(range(int((mach == m).sum())))
    # the best is the lowest makespan the walk saw, found at the first move that reached it
    seen = np.concatenate(([start], trace[0]))
    assert mk[0] == seen.min() and best_move == int(np.argmax(seen == seen.min()))
    # a prefix of the walk is the shorter walk
    half = [n(x) for x in env.tabu_blocks(None, iters // 2, tenure, None, reach, trace=True, log=True)]
    assert np.array_equal(half[3][0], trace[0, :iters // 2]) and half[0][0] == seen[:iters // 2 + 1].min()
    assert np.array_equal(half[4][0], moved[0, :iters // 2])


# ---- the anchors -----------------------------------------------------------------------------------------------------------------
def case_anchor(be, key, mirror=False):
    """B = 1 from rollout(kind): the listed start, best, move and evaluations; with `mirror` the NumPy mirror gives them too"""
    name, kind, tenure, iters = key
    env = K.rolled_out(be, name, kind)
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    start = int(n(env.evaluate_order())[0])
    mk, _, info = (n(x) for x in env.tabu_blocks(None, iters, tenure))
    assert (start, int(mk[0]), int(info[0, 2]), int(info[0, 3])) == ANCHORS[key] and info[0, :2].tolist() == [0, iters]
    if mirror:
        host = K.host_tables(env)
        ref = search.block_reference(host["env_const"], host["ops"], n(env.solution), iters, tenure)
        assert (int(ref[0][0]), int(ref[3][0, 2]), int(ref[3][0, 3])) == ANCHORS[key][1:]
        assert np.array_equal(ref[3], info)


_EARNED = {}


def case_earns_its_keep(be, key):
    """from SPT with the swap walk's tenure, with as many moves as the swap walk's anchor spent re-timings, the block walk's best is
    no worse than the swap walk's; the twin's figures are kept, and every other backend gives the same bits"""
    name, kind, tenure, iters = key
    swap_start, swap_best, _, swap_evaluations = T.ANCHORS[key]
    moves, listed = EARNS[key]
    assert moves == swap_evaluations + iters                         # its neighbours and its moves: the start is re-timed by both
    env = K.rolled_out(be, name, kind)
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    mk, rank, info = (n(x) for x in env.tabu_blocks(None, moves, tenure))
    print(key, "block walk:", int(mk[0]), info[0].tolist(), "swap walk:", swap_best)
    assert info[0, 0] == 0 and info[0, 1] == moves and n(env.evaluate_order(rank))[0] == mk[0]
    assert mk[0] <= swap_best
    assert mk[0] == listed
    if be is twin_backend():
        _EARNED[key] = (int(mk[0]), info[0].tolist())
    elif key in _EARNED:
        assert (int(mk[0]), info[0].tolist()) == _EARNED[key]


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def definition_loop(be, instances, kind, walkers, iters, tenure, explore, seed, target, reach):
    """search.tabu_search(moves="block") written with the public calls: returns (makespan, walker, rank, start, optimal,
    best_makespan, info)"""
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
    mk, best_rank, info = (n(x) for x in env.tabu_blocks(None, iters, ten, tgt, reach))
    makespan, walker = [], []
    for g in range(G):
        low = min((int(mk[g * W + w]), w) for w in range(W) if mk[g * W + w] >= 0)
        makespan.append(low[0]), walker.append(low[1])
    winner = np.array([g * W + w for g, w in enumerate(walker)], np.int32)
    again, start = (n(x) for x in env.evaluate_order(best_rank, winner, start=True))
    assert again.tolist() == makespan
    optimal = [bool(info[i, 0] == 1 or (tgt is not None and mk[i] <= tgt[i])) for i in winner]
    return np.array(makespan), np.array(walker), best_rank[winner], start, np.array(optimal), mk, info


def case_driver(be, instances, kind="SPT", walkers=4, iters=30, tenure=(5, 12), explore=0.1, seed=0, target="lower_bound", reach=0):
    want = definition_loop(be, instances, kind, walkers, iters, tenure, explore, seed, target, reach)
    res = search.tabu_search(instances, kind, walkers, iters, tenure, explore, seed, target, _backend=be, moves="block", reach=reach)
    for g, w, label in zip((res.makespan, res.walker, res.rank, res.start, res.optimal, res.best_makespan, res.info), want,
                           ("makespan", "walker", "rank", "start", "optimal", "best_makespan", "info")):
        assert np.array_equal(g, w), label
    G = len(res.makespan)
    assert np.array_equal(res.makespan, res.best_makespan.reshape(G, walkers).min(axis=1))   # the group's best walker
    assert res.makespan.dtype == np.int32 and res.env.batch == G * walkers and res.info.shape == (G * walkers, _abi.BLOCK_NI)
    return res


def case_driver_swap_is_unchanged(be):
    """moves="swap", given or left out, and the positional form: tabu_cases' definition loop of the swap walk"""
    want = T.definition_loop(be, ["ta01", "ta02"], "SPT", 3, 12, (5, 12), 0.1, 0, "lower_bound")
    for res in (search.tabu_search(["ta01", "ta02"], "SPT", 3, 12, (5, 12), 0.1, 0, "lower_bound", None, be),
                search.tabu_search(["ta01", "ta02"], "SPT", 3, 12, _backend=be, moves="swap"),
                search.tabu_search(["ta01", "ta02"], walkers=3, iters=12, _backend=be, moves="swap", reach=0)):
        for g, w in zip((res.makespan, res.walker, res.rank, res.start, res.optimal, res.best_makespan, res.info), want):
            assert np.array_equal(g, w)
        assert res.info.shape == (6, _abi.TABU_NI)


# ---- ABI errors ------------------------------------------------------------------------------------------------------------------
def case_abi_errors(be):
    """every code of jss_block_search, before anything runs: the outputs keep their fill"""
    lib = search.block_library(be)
    env = K.env_on(be, "3x2")
    st = K.case_state("3x2")
    B = env.batch
    with be.on_device():
        rank = be.from_numpy(st["rank"])
        ten, tgt = be.from_numpy(np.full(B, 2, np.int32)), be.from_numpy(np.zeros(B, np.int32))
        out = {k: be.from_numpy(np.full(s, FILL, np.int32)) for k, s in (("best_makespan", B), ("best_rank", (B, env.jmax, env.mmax)),
                                                                         ("last_rank", (B, env.jmax, env.mmax)),
                                                                         ("info", (B, _abi.BLOCK_NI)), ("trace", (B, 5)),
                                                                         ("move_log", (B, 5, 2)))}
    p = be.ptr

    def call(desc=None, state=True, arg=True, **fields):
        d = _abi.JssDesc.from_buffer_copy(env._desc)
        for k, v in ({} if desc in (None, "null") else desc).items():
            setattr(d, k, v)
        t = _abi.JssBlock(5, 2, 0, p(rank), p(ten), p(tgt), p(out["best_makespan"]), p(out["best_rank"]), p(out["last_rank"]),
                          p(out["info"]), p(out["trace"]), p(out["move_log"]))
        for k, v in fields.items():
            setattr(t, k, v)
        rc = lib.jss_block_search(C.byref(d) if desc != "null" else None, C.byref(env._state) if state else None,
                                  C.byref(t) if arg else None, be.stream())
        be.sync()
        return rc

    assert call(desc="null") == _abi.E_NULL and call(state=False) == _abi.E_NULL and call(arg=False) == _abi.E_NULL
    assert call(rank=None) == _abi.E_NULL and call(best_makespan=None) == _abi.E_NULL and call(best_rank=None) == _abi.E_NULL
    assert call(desc={"ops": None}) == _abi.E_NULL
    assert call(iters=-1) == _abi.E_SHAPE and call(iters=65537) == _abi.E_SHAPE
    assert call(tenure=-1, tenure_of=None) == _abi.E_SHAPE and call(tenure=65, tenure_of=None) == _abi.E_SHAPE
    assert call(reach=-1) == _abi.E_SHAPE and call(reach=65536) == _abi.E_SHAPE
    assert call(desc={"jmax": 0}) == _abi.E_SHAPE and call(desc={"mmax": 65}) == _abi.E_SHAPE and call(desc={"batch": -1}) == _abi.E_SHAPE
    assert call(desc={"kernel": 64}) == _abi.E_KIND
    # a row of more than 3568 entries does not fit one walker's 64 KB of LDS: both libraries say so; 128 x 27 fits (not run)
    assert call(desc={"jmax": 128, "mmax": 64}) == _abi.E_LDS and call(desc={"jmax": 128, "mmax": 28}) == _abi.E_LDS
    assert call(desc={"jmax": 128, "mmax": 27, "batch": 0}) == 0 and call(desc={"batch": 0}) == 0      # batch == 0 launches nothing
    for k, v in out.items():
        assert (np.asarray(be.numpy(v)) == FILL).all(), k
    # tenure is not looked at where tenure_of is given; the optional pointers may all be NULL; iters and reach at their bounds
    assert call(tenure=99) == 0 and call(iters=0, tenure_of=None, target=None, last_rank=None, info=None, trace=None, move_log=None) == 0
    assert call(tenure=64, tenure_of=None, reach=65535) == 0 and call(tenure=0, tenure_of=None, iters=1) == 0
    assert not (np.asarray(be.numpy(out["best_makespan"])) == FILL).any()


# ---- the built library ------------------------------------------------------------------------------------------------------------
def block_kernel_rows():
    """[(name, vgprs, sgprs, spilled vgprs, spilled sgprs, scratch bytes, static LDS bytes)] of libjss_block_hip.so"""
    import re
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import LLVM, kernel_resources
    from jssenv_amd.build import build_block_extension
    so = build_block_extension()                                      # (built here if build() has not run)
    rows = kernel_resources(so)
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "block.co")
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", so, fat], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    lds = [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", notes)]
    assert len(lds) == len(rows)
    return [r + (b,) for r, b in zip(rows, lds)]
