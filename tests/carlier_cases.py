"""Backend-agnostic cases of jss_machine_solve and jss_bottleneck_exact (include/jss_carlier.h), BatchedJssEnv.solve_machines /
bottleneck_exact and search.bottleneck_search(nodes=...), run against the host-core twin, the kernel source
(jssenv_amd/csrc/jss_carlier.hip) under the SIMT emulator and the HIP library libjss_carlier_hip.so.

The references are search.solve_reference and search.bottleneck_exact_reference (NumPy, written from the header's definition).
The batches, rank tables, masks, candidate lists and biases are machine_cases'; a case's references are made once per budget."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np

import order_cases as K
import machine_cases as S
from clone_cases import rows_of
from jssenv_amd import BatchedJssEnv, _abi, search

ROOT = K.ROOT
CARLIER_SRC = os.path.join(ROOT, "jssenv_amd", "csrc", "jss_carlier.hip")
EMU_LIB = os.path.join(K.EMU, "libjss_carlier_emu.so")
FILL = K.FILL
FILL64 = np.uint64(np.int64(FILL).astype(np.uint64))
SOLVE_OUT = ("length", "lower_bound", "bottleneck", "opt", "low", "nodes_used", "proved", "head", "tail", "rank_out")
BUILD_OUT = S.BUILD_OUT
BUDGETS = (1, 2, 3, 256)

# The textbook case of the header (Carlier 1982): 7 jobs x 3 operations on machines (1, 0, 2) with durations (r, p, q); nothing is
# fixed, so the heads and tails of machine 0's operations are r and q.
HAND_R, HAND_P, HAND_Q = (11, 14, 12, 21, 31, 1, 31), (5, 6, 7, 4, 3, 6, 2), (8, 27, 25, 22, 9, 18, 1)
HAND_SCHRAGE = [11, 16, 22, 29, 33, 1, 36]
HAND_BEST = [29, 19, 12, 25, 34, 1, 37]

# prototype values of the header's definition, unbiased builds with a budget of 4096: (instance, reopt) -> makespan; for ta01
# also (nodes in total, most nodes of one problem); (reopt, budget) -> ta01's makespan; ta01's empty selection per machine
ANCHOR_EXACT = {("ta01", 0): 1512, ("ta01", 1): 1345, ("ta01", 3): 1352, ("ta11", 0): 1805, ("ta11", 1): 1702, ("ta41", 0): 2736,
                ("ta41", 1): 2487, ("ta51", 0): 3662, ("ta61", 0): 3917, ("ta71", 0): 7131}
ANCHOR_NODES = {("ta01", 0): (20, 2), ("ta01", 1): (264, 18), ("ta01", 3): (627, 9), ("ta11", 0): (43, 8), ("ta11", 1): (350, 23),
                ("ta41", 0): (47, 13), ("ta41", 1): (818, 33), ("ta71", 0): (303, 62)}
ANCHOR_PROBLEMS = {0: lambda m: m, 1: lambda m: m + m * (m - 1) // 2, 3: lambda m: m + 3 * m * (m - 1) // 2}
ANCHOR_BUDGET = {(0, 2): 1512, (1, 2): 1406, (1, 4): 1366, (1, 8): 1345}
TA01_OPT = [964, 1168, 963, 963, 963, 973, 1051, 963, 963, 963, 976, 963, 990, 1013, 1050]
TA01_NODES = [3, 1, 4, 1, 5, 2, 1, 2, 3, 5, 1, 4, 1, 1, 1]
GPU_ANCHORS = S.GPU_ANCHORS


def build_emu_carlier():
    """jss_carlier.hip, unmodified, compiled with g++ against the SIMT emulator's hip_runtime.h: a library of its own"""
    deps = [CARLIER_SRC, os.path.join(K.EMU, "hip", "hip_runtime.h"), os.path.join(ROOT, "jssenv_amd", "csrc", "jss_abi_checks.hpp"),
            os.path.join(ROOT, "include", "jss_carlier.h"), os.path.join(ROOT, "include", "jss_machine.h")]
    if not os.path.isfile(EMU_LIB) or any(os.path.getmtime(d) > os.path.getmtime(EMU_LIB) for d in deps):
        tmp = EMU_LIB + f".tmp{os.getpid()}"
        subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
                               "-Wno-unknown-pragmas", "-I" + K.EMU, "-I" + os.path.join(ROOT, "include"), CARLIER_SRC, "-o", tmp])
        os.replace(tmp, EMU_LIB)
    return EMU_LIB


def emu_backend():
    """machine_cases' emulator backend with the emulated Carlier library as its `carlier_lib`"""
    be = S.emu_backend()
    be.carlier_lib = _abi.bind_carlier(C.CDLL(build_emu_carlier()))
    return be


twin_backend = K.twin_backend
_REFS = {}


def tables_of(name):
    st = S.case_state(name)
    env = st["env"]
    return st, st["host"]["env_const"].reshape(-1, _abi.NC), st["host"]["ops"].reshape(-1, env.jmax, env.mmax)


def reopts_of(name, nodes):
    """the rounds a case's exact builds are run with: the mirror takes seconds per build at 15 x 15 and beyond, and a round over
    64 machines of three operations each is 2 016 relaxations that find nothing to search"""
    return S.reopts_of(name) if name in S.SMALL else (0, 1) if nodes == 256 and name != "m64" else (0,)


def solve_ref(name, nodes):
    key = (name, "solve", nodes)
    if key not in _REFS:
        st, const, ops = tables_of(name)
        _REFS[key] = search.solve_reference(const, ops, st["ranks"], st["masks"], st["par"], nodes, fill=FILL)
    return _REFS[key]


def exact_ref(name, nodes, reopt, resumed=False):
    key = (name, "exact", nodes, reopt, resumed)
    if key not in _REFS:
        st, const, ops = tables_of(name)
        kw = dict(rank=st["start_rank"], fixed=st["sub_of"]) if resumed else {}
        _REFS[key] = search.bottleneck_exact_reference(const, ops, st["bpar"], st["bias"], reopt, nodes, fill=FILL, **kw)
    return _REFS[key]


def call_solve(be, env, rank=None, fixed=None, parents=None, nodes=256, want=SOLVE_OUT[1:], n=None, desc=None, null=(), stride=None, alias=False):
    """jss_machine_solve through the backend's library: (rc, {output: host array}); the outputs are prefilled (FILL)"""
    lib = search.carlier_library(be)
    n = (env.batch if parents is None else len(parents)) if n is None else n
    rows = max(n, 1)
    with be.on_device():
        dev = lambda x: None if x is None else be.from_numpy(np.asarray(x, np.int32))   # noqa: E731
        full = lambda *shape: be.from_numpy(np.full(shape, FILL, np.int32))   # noqa: E731
        r, par, fx = dev(rank), dev(parents), S._masks_on(be, fixed)
        shapes = dict(length=(rows,), lower_bound=(rows,), bottleneck=(rows,), opt=(rows, env.mmax), low=(rows, env.mmax),
                      nodes_used=(rows, env.mmax), head=(rows, env.jmax, env.mmax), tail=(rows, env.jmax, env.mmax),
                      rank_out=(rows, env.jmax, env.mmax))
        out = {k: None for k in SOLVE_OUT}
        for k in SOLVE_OUT:
            if k == "proved":
                out[k] = be.from_numpy(np.full(rows, FILL, np.int64)) if k in want else None
            elif k == "length" or k in want:
                out[k] = full(*shapes[k])
        p = be.ptr
        if stride is None:
            stride = env.jmax * env.mmax if rank is not None and np.ndim(rank) == 3 else 0
        arg = _abi.JssMachineSolve(n, stride, nodes, 0, p(par), None if "rank" in null else p(r), p(fx),
                                   None if "length" in null else p(out["length"]), *(p(out[k]) for k in SOLVE_OUT[1:9]),
                                   p(r) if alias else p(out["rank_out"]))
        rc = lib.jss_machine_solve(C.byref(env._desc) if desc is None else desc, None if "state" in null else C.byref(env._state),
                                   None if "arg" in null else C.byref(arg), be.stream())
        be.sync()
    host = {k: None if v is None else np.asarray(be.numpy(v)) for k, v in out.items()}
    if host["proved"] is not None:
        host["proved"] = host["proved"].view(np.uint64)
    return rc, host


def call_exact(be, env, parents=None, bias=None, reopt=1, nodes=256, rank=None, fixed=None, want=("info", "order"), n=None, desc=None, null=(),
               alias=False):
    """jss_bottleneck_exact through the backend's library: (rc, {output: host array}), prefilled like call_solve's"""
    lib = search.carlier_library(be)
    n = (env.batch if parents is None else len(parents)) if n is None else n
    rows = max(n, 1)
    with be.on_device():
        dev = lambda x: None if x is None else be.from_numpy(np.asarray(x, np.int32))   # noqa: E731
        full = lambda *shape: be.from_numpy(np.full(shape, FILL, np.int32))   # noqa: E731
        r, par, fx, bs = dev(rank), dev(parents), S._masks_on(be, fixed), dev(bias)
        out = dict(makespan=full(rows), rank=full(rows, env.jmax, env.mmax), info=full(rows, _abi.EXACT_NI) if "info" in want else None,
                   order=full(rows, env.mmax) if "order" in want else None)
        p = be.ptr
        arg = _abi.JssBottleneckExact(n, reopt, nodes, 0, p(par), p(r), p(fx), p(bs), None if "makespan" in null else p(out["makespan"]),
                                      None if "rank" in null else p(r) if alias else p(out["rank"]), p(out["info"]), p(out["order"]))
        rc = lib.jss_bottleneck_exact(C.byref(env._desc) if desc is None else desc, None if "state" in null else C.byref(env._state),
                                      None if "arg" in null else C.byref(arg), be.stream())
        be.sync()
    return rc, {k: None if v is None else np.asarray(be.numpy(v)) for k, v in out.items()}


def same(got, ref, names, what, idx=None):
    rc, out = got
    assert rc == 0, (what, rc)
    for k, want in zip(names, ref):
        if out[k] is not None:
            want = want if idx is None else want[idx]
            assert out[k].dtype == want.dtype and np.array_equal(out[k][:len(want)], want), (what, k, out[k][:len(want)], want)


def picks(st, light):
    """all candidates; light == 2: env 0's and the refused parents"""
    par, bpar, B = st["par"], st["bpar"], st["B"]
    if light == 2:
        return np.flatnonzero((par == 0) | (par < 0) | (par >= B - 1)), np.flatnonzero((bpar == 0) | (bpar < 0) | (bpar >= B - 1))
    return np.arange(par.size), np.arange(bpar.size)


# ---- 1. against the mirror --------------------------------------------------------------------------------------------------------
def case_against_mirror(be, name, light=0):
    """jss_machine_solve on machine_cases' candidate list and jss_bottleneck_exact on its biased candidates, at every budget of
    BUDGETS, bit for bit; the optional outputs on their own, the shared table, n == 0, going on from a partial selection; refused
    and cyclic rows keep their fill; the batch is untouched.  `light` is for the emulator: 1 runs the budgets 1 and 256 and
    leaves out the combinations of optional outputs; 2 (the larger shapes) runs env 0's candidates and the refused parents
    through one solve call and one reopt-0 build, at the budget 3"""
    st = S.case_state(name)
    env = S.env_on(be, name)
    before = rows_of(env)
    par, masks, ranks, bpar, bias = st["par"], st["masks"], st["ranks"], st["bpar"], st["bias"]
    pick, bpick = picks(st, light)
    for nodes in (BUDGETS if not light else (1, 256) if light == 1 else (3,)):
        ref = solve_ref(name, nodes)
        same(call_solve(be, env, ranks[pick], masks[pick], par[pick], nodes), ref, SOLVE_OUT, (name, "candidates", nodes), pick)
        dead = ref[0] < 0
        assert np.array_equal(ref[0] == -1, st["refused"])
        for k, rows in zip(SOLVE_OUT[1:], ref[1:]):
            fill = FILL64 if k == "proved" else FILL
            assert (rows[dead] == fill).all() and not (rows[~dead] == fill).any(), (name, k)
        if light == 2 and env.mmax > 32:
            same(call_exact(be, env, bpar[bpick], bias[bpick], 0, nodes, st["start_rank"][bpick], st["sub_of"][bpick]),
                 exact_ref(name, nodes, 0, True), BUILD_OUT, (name, "resumed, reopt 0", nodes), bpick)
            continue
        for reopt in ((0,) if light == 2 else reopts_of(name, nodes)):
            ref = exact_ref(name, nodes, reopt)
            same(call_exact(be, env, bpar[bpick], bias[bpick], reopt, nodes), ref, BUILD_OUT, (name, "build", nodes, reopt), bpick)
            assert np.array_equal(ref[0] == -1, st["brefused"])
            for rows in ref[1:]:
                assert (rows[ref[0] < 0] == FILL).all() and not (rows[ref[0] >= 0] == FILL).any(), name
    if light < 2:
        nodes = 3
        ref = solve_ref(name, nodes)
        for k in (SOLVE_OUT[1:] if not light else ("proved", "rank_out")):
            same(call_solve(be, env, ranks, masks, par, nodes, want=(k,)), ref, SOLVE_OUT, (name, "only", k))
        same(call_solve(be, env, ranks, masks, par, nodes, want=()), ref, SOLVE_OUT, (name, "length alone"))
        got = call_solve(be, env, ranks, masks, par, nodes, n=0)
        assert got[0] == 0 and all((x == FILL).all() or (x == FILL64).all() for x in got[1].values())
        if name in S.SMALL:
            const, ops = tables_of(name)[1:]
            same(call_solve(be, env, st["base"], masks, par, nodes), search.solve_reference(const, ops, st["base"], masks, par, nodes, fill=FILL),
                 SOLVE_OUT, (name, "shared"))
            same(call_solve(be, env, nodes=nodes), search.solve_reference(const, ops, None, None, None, nodes, fill=FILL), SOLVE_OUT, (name, "rows"))
            same(call_exact(be, env, bpar, bias, 1, nodes, st["start_rank"], st["sub_of"]), exact_ref(name, nodes, 1, True), BUILD_OUT, (name, "resumed"))
            same(call_exact(be, env, bpar, None, 1, nodes),
                 search.bottleneck_exact_reference(const, ops, bpar, None, 1, nodes, fill=FILL), BUILD_OUT, (name, "no bias"))
            same(call_exact(be, env, bpar, bias, 1, nodes, want=()), exact_ref(name, nodes, 1), BUILD_OUT, (name, "no optional outputs"))
        got = call_exact(be, env, bpar, bias, 1, nodes, n=0)
        assert got[0] == 0 and all((x == FILL).all() for x in got[1].values())
    after = rows_of(env)
    for k in before:
        assert np.array_equal(before[k], after[k]), (name, k)


# ---- 2. a budget of one node is the existing library -------------------------------------------------------------------------------
def case_budget_one(be, name, light=0):
    """nodes == 1: jss_bottleneck_exact gives jss_bottleneck_build's makespan, rank, order and info[:4], jss_machine_solve
    jss_machine_relax's outputs with opt == schrage and low == jps -- both called on this backend"""
    st = S.case_state(name)
    env = S.env_on(be, name)
    pick, bpick = picks(st, light)
    par, masks, ranks, bpar, bias = st["par"][pick], st["masks"][pick], st["ranks"][pick], st["bpar"][bpick], st["bias"][bpick]
    rc, old = S.call_relax(be, env, ranks, masks, par)
    rc1, new = call_solve(be, env, ranks, masks, par, 1)
    assert rc == 0 and rc1 == 0
    for a, b in (("length", "length"), ("lower_bound", "lower_bound"), ("bottleneck", "bottleneck"), ("schrage", "opt"), ("jps", "low"),
                 ("head", "head"), ("tail", "tail"), ("rank_out", "rank_out")):
        assert np.array_equal(old[a], new[b]), (name, a)
    live = new["length"] >= 0
    assert ((new["nodes_used"][live] == 1) == (new["opt"][live] >= 0)).all() and (new["nodes_used"][~live] == FILL).all()
    # (proved at one node: the root was solved, or its bound closed it; then Schrage's value is the preemptive bound's)
    for c in np.flatnonzero(live):
        for m in range(env.mmax):
            if int(new["proved"][c]) >> m & 1:
                assert new["opt"][c, m] >= 0 and new["opt"][c, m] == new["low"][c, m] == old["jps"][c, m], (name, c, m)
    for reopt in ((0,) if light == 2 else S.reopts_of(name)):
        for kw in (dict(), dict(rank=st["start_rank"][bpick], fixed=st["sub_of"][bpick])):
            rc, old = S.call_build(be, env, bpar, bias, reopt, **kw)
            rc1, new = call_exact(be, env, bpar, bias, reopt, 1, **kw)
            assert rc == 0 and rc1 == 0
            for k in ("makespan", "rank", "order"):
                assert np.array_equal(old[k], new[k]), (name, reopt, k)
            assert np.array_equal(old["info"], new["info"][:, :4]), (name, reopt)
            done = new["makespan"] >= 0
            assert (new["info"][done, 7] == 0).all() and (new["info"][done, 5] <= 1).all()
            if light:
                break


def case_cyclic_build(be):
    """machine_cases' build on durations of 0 that turns cyclic: -2 at a budget of one node as from the existing library, and at
    every budget what the mirror gives; the rows keep their fill"""
    inst = S.D.inst_with_zeros("cyclic", S.CYCLIC_MACHINE, S.CYCLIC_DURATION)
    env = BatchedJssEnv(inst, batch=1, _backend=be)
    env.reset()
    host = K.host_tables(env)
    old = S.call_build(be, env, None, None, S.CYCLIC_REOPT)
    new = call_exact(be, env, None, None, S.CYCLIC_REOPT, 1)
    assert old[1]["makespan"].tolist() == [-2] == new[1]["makespan"].tolist() and all((x == FILL).all() for k, x in new[1].items() if k != "makespan")
    for nodes in BUDGETS:
        ref = search.bottleneck_exact_reference(host["env_const"], host["ops"].reshape(-1, env.jmax, env.mmax), None, None, S.CYCLIC_REOPT, nodes, fill=FILL)
        same(call_exact(be, env, None, None, S.CYCLIC_REOPT, nodes), ref, BUILD_OUT, ("cyclic build", nodes))


# ---- 3. the hand case ------------------------------------------------------------------------------------------------------------------
def hand_instance():
    return K.inst("carlier7", [[1, 0, 2]] * 7, list(zip(HAND_R, HAND_P, HAND_Q)))


def case_hand(be, mirror=False):
    """the header's textbook case through the public calls, at budgets of 1, 2 and 100 nodes.  The second node finds the optimum;
    it is the last one a budget of 2 pays for, so the proof -- both its children are closed by Jackson's bound -- needs a budget
    of 3"""
    env = BatchedJssEnv(hand_instance(), batch=1, _backend=be)
    env.reset()
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    jps, sch, head, tail = (n(x)[0] for x in env.relax_machines(jps=True, schrage=True, head=True, tail=True)[3:])
    assert head[:, 1].tolist() == list(HAND_R) and tail[:, 1].tolist() == list(HAND_Q) and (jps[0], sch[0]) == (51, 55)
    for nodes, (opt, low, used, proved, starts) in {1: (55, 51, 1, 0, HAND_SCHRAGE), 2: (52, 51, 2, 0, HAND_BEST), 3: (52, 52, 2, 1, HAND_BEST),
                                                      100: (52, 52, 2, 1, HAND_BEST)}.items():
        out = [n(x)[0] for x in env.solve_machines(nodes=nodes, opt=True, low=True, nodes_used=True, proved=True, rank_out=True)]
        print("hand case, budget", nodes, "opt", out[3], "low", out[4], "nodes", out[5], "proved", out[6])
        assert (out[3][0], out[4][0], out[5][0], int(out[6]) & 1) == (opt, low, used, proved), (nodes, out)
        assert out[7][:, 1].tolist() == starts and out[0] >= low and out[1] == max(r + p + q for r, p, q in zip(HAND_R, HAND_P, HAND_Q))
        if mirror:
            assert search.carlier_reference(HAND_R, HAND_P, HAND_Q, nodes) == (opt, bool(proved), low, used, starts)
    mk, rank, info = (n(x) for x in env.bottleneck_exact(reopt=0, nodes=100))
    assert mk[0] >= 52 and n(env.evaluate_order(rank))[0] == mk[0] and info[0, 6] == 0


# ---- 4. brute force --------------------------------------------------------------------------------------------------------------------
def brute_optimum(r, p, q):
    """the least max(s + p + q) over every order of the operations, each started as early as its order allows"""
    n = len(r)
    perms = np.array(list(itertools.permutations(range(n))))
    r, p, q = (np.asarray(x, np.int64) for x in (r, p, q))
    t, value = np.zeros(len(perms), np.int64), np.zeros(len(perms), np.int64)
    for k in range(n):
        i = perms[:, k]
        t = np.maximum(t, r[i]) + p[i]
        value = np.maximum(value, t + q[i])
    return int(value.min())


def check_optimum(opt, r, p, q):
    assert opt == brute_optimum(r, p, q), (opt, r, p, q)


def tiny_instance(rng, w):
    """a seeded tiny instance with at most 7 operations on a machine, durations 1-20: 4 to 7 jobs on 2 or 3 machines; every third
    one has 2 to 4 jobs of 3 operations whose machines may repeat"""
    while True:
        J, M = int(rng.integers(4, 8)), int(rng.integers(2, 4))
        if w % 3 == 0:
            J, M = int(rng.integers(2, 5)), 3
            machine = rng.integers(0, M, (J, M))
        else:
            machine = np.stack([rng.permutation(M) for _ in range(J)])
        if np.bincount(machine.reshape(-1)).max() <= 7:
            return K.inst("tiny", machine, rng.integers(1, 21, (J, M))), machine


def case_brute_force(be, count, seed=17):
    """`count` seeded tiny instances; per instance every selection on the way of an exact build, machine after machine fixed in
    its order: every proved opt is the minimum over all permutations, low never exceeds the best completion (where that is cheap
    to enumerate).  Returns (one-machine problems checked, instances on which some opt < schrage, selections bounded)"""
    rng = np.random.default_rng(seed)
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    checked = improved = bounded = 0
    for w in range(count):
        better = False
        inst, machine = tiny_instance(rng, w)
        J, M = machine.shape
        env = BatchedJssEnv(inst, batch=1, _backend=be)
        env.reset()
        dur = (K.host_tables(env)["ops"].reshape(-1, env.jmax, env.mmax)[0] & 0xFFFF)[:J, :M]
        mk, rank, info, order = (n(x) for x in env.bottleneck_exact(reopt=0, nodes=4096, order=True))
        assert mk[0] >= 0 and info[0, 6] == 0
        mask, part, selections = 0, np.zeros((J, M), np.int32), [(None, 0)]
        for m in order[0][order[0] >= 0].tolist()[:-1]:
            mask, part = mask | 1 << m, np.where(machine == m, rank[0, :J, :M], part).astype(np.int32)
            selections.append((part[None], mask))
        for table, mask in selections:
            part = None if table is None else table[0]
            sch = n(env.relax_machines(table, mask, schrage=True)[3])[0]
            lower, length, neck, opt, low, used, proved, head, tail = (n(x)[0] for x in env.solve_machines(
                table, mask, nodes=4096, opt=True, low=True, nodes_used=True, proved=True, head=True, tail=True))
            assert length >= 0
            for m in range(M):
                its = [(j, k) for j in range(J) for k in range(M) if machine[j, k] == m]
                if mask >> m & 1 or not its:
                    assert opt[m] == -1 and not int(proved) >> m & 1
                    continue
                assert int(proved) >> m & 1 and low[m] == opt[m] <= sch[m]
                check_optimum(int(opt[m]), *([int(x[j, k]) for j, k in its] for x in (head, dur, tail)))
                checked, better = checked + 1, better or bool(opt[m] < sch[m])
            if J * M <= 9:
                best = S.best_completion(be, inst, np.zeros((J, M), np.int32) if table is None else part, mask, machine)
                if best is not None:
                    assert lower <= best, (w, mask, lower, best)
                    bounded += 1
        improved += better
    return checked, improved, bounded


# ---- 5. properties -----------------------------------------------------------------------------------------------------------------------
def check_properties(be, env, rng, what, positive=True):
    """env 0: along an exact build's own order of machines, at every budget: jps <= low <= opt <= schrage; proved => low == opt;
    more budget never a worse opt or a weaker low; rank_out fed back with a machine's bit set is acyclic, or a build made to fix
    that machine first counts a replaced sequence; the build's rank re-times to its makespan"""
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    zero = np.zeros(1, np.int32)
    mk, order_rank, info, fixed_order = (n(x) for x in env.bottleneck_exact(zero, rng.integers(0, 20, (1, env.mmax)), int(rng.integers(0, 3)),
                                                                            int(rng.choice(BUDGETS)), order=True))
    if not positive and mk[0] < 0:
        return
    retimed = n(env.evaluate_order(np.tile(order_rank, (env.batch, 1, 1)), zero))
    assert mk[0] >= 0 and retimed[0] == mk[0] and mk[0] >= info[0, 3] and info[0, 5] <= info[0, 4], what
    rank, mask = order_rank, 0
    for step, m_next in enumerate(fixed_order[0][fixed_order[0] >= 0].tolist()):
        jps, sch = (n(x)[0] for x in env.relax_machines(rank, mask, zero, jps=True, schrage=True)[3:])
        last_opt, last_low = sch, jps
        for nodes in BUDGETS + (4096,):
            lower, length, neck, opt, low, used, proved, rank_out = (n(x)[0] for x in env.solve_machines(
                rank, mask, zero, nodes, opt=True, low=True, nodes_used=True, proved=True, rank_out=True))
            free = opt >= 0
            assert np.array_equal(free, jps >= 0) and (jps <= low).all() and (low <= opt).all() and (opt <= sch).all(), (what, step, nodes)
            assert (opt <= last_opt).all() and (low >= last_low).all() and ((used >= 1) == free).all() and (used <= nodes).all(), (what, step, nodes)
            done = np.array([bool(int(proved) >> m & 1) for m in range(env.mmax)])
            assert not (done & ~free).any() and (low[done] == opt[done]).all() and (low[free & ~done] == jps[free & ~done]).all(), (what, step, nodes)
            assert lower == max(length, low.max()) and (neck < 0 or low[neck] == low.max()), (what, step, nodes)
            last_opt, last_low = opt, low
            for m in np.flatnonzero(free) if nodes in (2, 4096) else ():
                if n(env.relax_machines(rank_out[None], mask | 1 << int(m), zero)[1])[0] == -2:
                    bias = np.zeros((1, env.mmax), np.int32)
                    bias[0, m] = 2 ** 30
                    row = rank if rank.ndim == 3 else rank[None]
                    forced = n(env.bottleneck_exact(zero, bias, 0, nodes, row, np.array([mask], np.uint64), order=True)[2])[0]
                    assert not positive or forced[7] >= 1, (what, step, nodes, m)
        assert done[free].all()                                        # (4096 nodes close every problem of these sizes)
        mask |= 1 << m_next


def case_properties(be, name):
    check_properties(be, S.env_on(be, name), np.random.default_rng(5), name, positive=name != "zeros")


def case_seeded_properties(be, count, seed=23):
    rng = np.random.default_rng(seed)
    for w in range(count):
        inst, _ = tiny_instance(rng, w)
        env = BatchedJssEnv(inst, batch=1, _backend=be)
        env.reset()
        check_properties(be, env, rng, w)


# ---- 6. anchors ----------------------------------------------------------------------------------------------------------------------------
def case_anchor(be, name, reopts=(0, 1, 3), mirror=False):
    """B = 1, unbiased, a budget of 4096 nodes: the prototype's makespans, node counts and problem counts; nothing left open"""
    env = BatchedJssEnv(name, batch=1, _backend=be)
    env.reset()
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    used = len(set(((K.host_tables(env)["ops"].reshape(-1, env.jmax, env.mmax)[0] >> 16) & 63).reshape(-1).tolist()))
    for reopt in reopts:
        if (name, reopt) not in ANCHOR_EXACT:
            continue
        mk, rank, info = (n(x) for x in env.bottleneck_exact(reopt=reopt, nodes=4096))
        print(name, "reopt", reopt, "makespan", mk, "info", info)
        assert mk.tolist() == [ANCHOR_EXACT[(name, reopt)]] and info[0, 3] == S.ANCHOR_BOUND.get(name, info[0, 3])
        assert info[0, 6] == 0 and info[0, 7] == 0 and info[0, 0] == used and info[0, 0] + info[0, 1] == ANCHOR_PROBLEMS[reopt](used)
        if (name, reopt) in ANCHOR_NODES:
            assert tuple(info[0, 4:6].tolist()) == ANCHOR_NODES[(name, reopt)]
        assert np.array_equal(n(env.evaluate_order(rank)), mk)
        if mirror and env.jmax * env.mmax <= 400 and reopt <= 1:
            host = K.host_tables(env)
            ref = search.bottleneck_exact_reference(host["env_const"], host["ops"].reshape(-1, env.jmax, env.mmax), reopt=reopt, nodes=4096)
            assert np.array_equal(ref[0], mk) and np.array_equal(ref[1], rank) and np.array_equal(ref[2], info)


def case_anchor_ta01(be, mirror=False):
    """ta01: the budgets 2, 4 and 8, and the empty selection machine by machine"""
    env = BatchedJssEnv("ta01", batch=1, _backend=be)
    env.reset()
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    for (reopt, nodes), want in ANCHOR_BUDGET.items():
        mk, _, info = (n(x) for x in env.bottleneck_exact(reopt=reopt, nodes=nodes))
        print("ta01 reopt", reopt, "budget", nodes, "makespan", mk, "info", info)
        assert mk.tolist() == [want] and info[0, 5] <= nodes
    lower, length, neck, opt, low, used, proved = (n(x)[0] for x in env.solve_machines(nodes=4096, opt=True, low=True, nodes_used=True, proved=True))
    print("ta01 empty selection: opt", opt, "nodes", used, "proved", proved)
    assert opt.tolist() == TA01_OPT and low.tolist() == TA01_OPT and used.tolist() == TA01_NODES and int(proved) == 2 ** 15 - 1
    assert (lower, length, neck) == (1168, 963, 1)
    if mirror:
        host = K.host_tables(env)
        ref = search.solve_reference(host["env_const"], host["ops"].reshape(-1, 15, 15), nodes=4096)
        assert ref[3][0].tolist() == TA01_OPT and ref[5][0].tolist() == TA01_NODES and int(ref[6][0]) == 2 ** 15 - 1


# ---- 7. refusals and errors ------------------------------------------------------------------------------------------------------------------
def case_refused_rows(be):
    """machine_cases' refused rows -- a parent out of range, the env never reset, a mask bit at M, a negative rank on a fixed
    machine: -1; a cyclic rank: -2 -- keep what they held, from both entry points"""
    env = S.env_on(be, "3x2")
    st = S.case_state("3x2")
    host = st["host"]
    base = st["base"]
    neg = base.copy()
    neg[0, 0] = -3
    cyc = np.array([[1, 0], [1, 1], [1, 0]], np.int32)
    par = np.array([0, 4, 3, 1, 0, 0, -1, 2], np.int32)
    masks = np.array([3, 0, 0, 4, 1, 2, 0, 3], np.uint64)
    ranks = np.stack([base, base, base, base, neg, neg, base, cyc])
    got = call_solve(be, env, ranks, masks, par, 5)
    same(got, search.solve_reference(host["env_const"], host["ops"].reshape(-1, 3, 2), ranks, masks, par, 5, fill=FILL), SOLVE_OUT, "refused rows")
    assert got[1]["length"].tolist()[1:5] == [-1] * 4 and got[1]["length"][6] == -1 and got[1]["length"][7] == -2 and got[1]["length"][0] >= 0
    for k in SOLVE_OUT[1:]:
        fill = FILL64 if k == "proved" else FILL
        assert (got[1][k][[1, 2, 3, 4, 6, 7]] == fill).all() and not (got[1][k][[0, 5]] == fill).any(), k
    got = call_exact(be, env, par, None, 1, 5, ranks, masks)
    same(got, search.bottleneck_exact_reference(host["env_const"], host["ops"].reshape(-1, 3, 2), par, None, 1, 5, ranks, masks, fill=FILL), BUILD_OUT,
         "refused builds")
    assert got[1]["makespan"][[1, 2, 3, 4, 6]].tolist() == [-1] * 5 and got[1]["makespan"][7] == -2 and got[1]["makespan"][5] >= 0
    for k in BUILD_OUT[1:]:
        assert (got[1][k][[1, 2, 3, 4, 6, 7]] == FILL).all(), k
    fresh = BatchedJssEnv("ta01", batch=2, _backend=be)
    for call in (fresh.solve_machines, fresh.bottleneck_exact):
        try:
            call()
        except RuntimeError:
            pass
        else:
            raise AssertionError("before reset() the call must raise")


def case_abi_errors(be):
    """every code of both entry points, before anything runs: the outputs keep their fill"""
    env = S.env_on(be, "3x2")
    st = S.case_state("3x2")
    B, ranks, masks, par = env.batch, st["ranks"], st["masks"], st["par"]

    def desc_of(desc):
        if desc is None or desc == "null":
            return None if desc is None else C.POINTER(_abi.JssDesc)()
        d = _abi.JssDesc.from_buffer_copy(env._desc)
        for k, v in desc.items():
            setattr(d, k, v)
        return C.byref(d)

    def untouched(got, kw):
        if got[0] and kw.get("n", 1):
            assert all(x is None or (x == FILL).all() or (x == FILL64).all() for x in got[1].values()), kw
        return got[0]

    def solve(desc=None, rank=ranks, fixed=masks, parents=par, nodes=7, **kw):
        return untouched(call_solve(be, env, rank, fixed, parents, nodes, desc=desc_of(desc), **kw), kw)

    def build(desc=None, parents=par, bias=None, reopt=1, nodes=7, rank=None, fixed=None, **kw):
        return untouched(call_exact(be, env, parents, bias, reopt, nodes, rank, fixed, desc=desc_of(desc), **kw), kw)

    for call in (solve, build):
        assert call(desc="null") == _abi.E_NULL and call(null=("state",)) == _abi.E_NULL and call(null=("arg",)) == _abi.E_NULL
        assert call(desc={"ops": None}) == _abi.E_NULL
        assert call(n=-1) == _abi.E_SHAPE and call(parents=None, n=B + 1) == _abi.E_SHAPE and call(parents=None, n=B - 1) == _abi.E_SHAPE
        assert call(desc={"jmax": 0}) == _abi.E_SHAPE and call(desc={"mmax": 65}) == _abi.E_SHAPE and call(desc={"batch": -1}) == _abi.E_SHAPE
        assert call(desc={"kernel": 64}) == _abi.E_KIND
        assert call(nodes=0) == _abi.E_SHAPE and call(nodes=-1) == _abi.E_SHAPE and call(nodes=_abi.CARLIER_MAX_NODES + 1) == _abi.E_SHAPE
        assert call(nodes=1) == 0 and call(nodes=_abi.CARLIER_MAX_NODES) == 0 and call(n=0) == 0 and call() == 0
    assert solve(null=("length",)) == _abi.E_NULL and solve(null=("rank",)) == _abi.E_NULL and solve(alias=True) == _abi.E_NULL
    assert solve(stride=5) == _abi.E_SHAPE and solve(desc={"jmax": env.jmax + 1}) == _abi.E_SHAPE
    assert solve(rank=None, fixed=None) == 0 and solve(fixed=None) == 0 and solve(want=()) == 0
    assert build(null=("makespan",)) == _abi.E_NULL and build(null=("rank",)) == _abi.E_NULL
    assert build(rank=ranks) == _abi.E_NULL and build(fixed=masks) == _abi.E_NULL and build(rank=ranks, fixed=masks, alias=True) == _abi.E_NULL
    assert build(reopt=-1) == _abi.E_SHAPE and build(reopt=_abi.BOTTLENECK_MAX_REOPT + 1) == _abi.E_SHAPE
    assert build(reopt=0) == 0 and build(reopt=_abi.BOTTLENECK_MAX_REOPT) == 0 and build(want=()) == 0
    # a row of more than 2272 entries does not fit one candidate's 64 KB of LDS: both libraries say so; 100 x 20 and 128 x 17 fit
    # (not run)
    shared = st["base"]
    assert solve(desc={"jmax": 128, "mmax": 18}, rank=shared) == _abi.E_LDS and build(desc={"jmax": 128, "mmax": 18}) == _abi.E_LDS
    assert solve(desc={"jmax": 128, "mmax": 17}, rank=shared, n=0) == 0 and build(desc={"jmax": 128, "mmax": 17}, n=0) == 0
    assert solve(desc={"jmax": 100, "mmax": 20}, rank=shared, n=0) == 0 and build(desc={"jmax": 100, "mmax": 20}, n=0) == 0


# ---- 8. the built library ----------------------------------------------------------------------------------------------------------------
def carlier_kernel_rows():
    """[(name, vgprs, sgprs, spilled vgprs, spilled sgprs, scratch bytes, static LDS bytes)] of libjss_carlier_hip.so"""
    import re
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import LLVM, kernel_resources
    from jssenv_amd.build import build_carlier_extension
    so = build_carlier_extension()                                    # (built here if build() has not run)
    rows = kernel_resources(so)
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "carlier.co")
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", so, fat], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    by_name = {}
    for k in notes.split("- .agpr_count")[1:]:
        by_name[re.search(r"\.name:\s+(\S+)", k).group(1)] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", k).group(1))
    assert len(by_name) == len(rows)
    lds = {next(r[0] for r in rows if r[0].split("(")[0] in name): size for name, size in by_name.items()}
    return [r + (lds[r[0]],) for r in rows]
