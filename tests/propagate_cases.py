"""Backend-agnostic cases of jss_propagate (include/jss_propagate.h), BatchedJssEnv.propagate and search.destructive_bound, run
against the host-core twin, the kernel source (jssenv_amd/csrc/jss_propagate.hip) under the SIMT emulator and the HIP library
libjss_propagate_hip.so.

The reference is search.propagate_reference (NumPy, the plain restatement of the header's definition).  The batches are
machine_cases'; a case's candidates -- partial selections, trial makespans, hypotheses, window tables -- are made once from the
case itself, and its references once per variant.  Where the mirror is too slow (its task intervals are O(n^4) per machine and
pass) the emulator and the device are held to the twin, and the twin to the mirror on a reduced set."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np

import order_cases as K
import machine_cases as S
import carlier_cases as X
import decode_cases as D
from clone_cases import rows_of
from jssenv_amd import BatchedJssEnv, _abi, search

ROOT = K.ROOT
PROPAGATE_SRC = os.path.join(ROOT, "jssenv_amd", "csrc", "jss_propagate.hip")
EMU_LIB = os.path.join(K.EMU, "libjss_propagate_emu.so")
FILL = K.FILL
PROP_OUT = ("status", "passes_used", "est", "lct")
BUDGETS = (1, 2, 256)
SLOW = ("one-machine", "J128")                       # 160 and 128 operations on one machine: one pass of the mirror, one candidate
NOT_MIRRORED = SLOW + ("m64",)                       # ... and 64 machines, which the mirror walks in Python every pass
MIRRORED = tuple(name for name in S.CASES if name not in NOT_MIRRORED)    # the cases whose every variant the mirror computes

FT06_MACHINE = [[2, 0, 1, 3, 5, 4], [1, 2, 4, 5, 0, 3], [2, 3, 5, 0, 1, 4], [1, 0, 2, 3, 4, 5], [2, 1, 4, 5, 0, 3], [1, 3, 5, 0, 4, 2]]
FT06_DURATION = [[1, 3, 6, 7, 3, 6], [8, 5, 10, 10, 10, 4], [5, 4, 8, 9, 1, 7], [5, 5, 5, 3, 8, 9], [9, 3, 5, 4, 3, 1], [3, 3, 9, 10, 4, 1]]
FT06_OPT = 55
# the statuses are firm (a pass does not depend on its order); the pass counts are the mirror's
FT06_STATUS = {47: 1, 48: 1, 49: 1, 50: 1, 51: 1, 52: 1, 53: 1, 54: 0, 55: 0, 56: 0}
TA01_STATUS = {1189: 1, 1190: 0}


def ft06():
    return K.inst("ft06", FT06_MACHINE, FT06_DURATION)


def build_emu_propagate():
    """jss_propagate.hip, unmodified, compiled with g++ against the SIMT emulator's hip_runtime.h: a library of its own"""
    deps = [PROPAGATE_SRC, os.path.join(K.EMU, "hip", "hip_runtime.h"), os.path.join(ROOT, "jssenv_amd", "csrc", "jss_abi_checks.hpp"),
            os.path.join(ROOT, "include", "jss_propagate.h"), os.path.join(ROOT, "include", "jss_machine.h")]
    if not os.path.isfile(EMU_LIB) or any(os.path.getmtime(d) > os.path.getmtime(EMU_LIB) for d in deps):
        tmp = EMU_LIB + f".tmp{os.getpid()}"
        subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
                               "-Wno-unknown-pragmas", "-I" + K.EMU, "-I" + os.path.join(ROOT, "include"), PROPAGATE_SRC, "-o", tmp])
        os.replace(tmp, EMU_LIB)
    return EMU_LIB


def emu_backend():
    """carlier_cases' emulator backend with the emulated propagation library as its `propagate_lib`"""
    be = X.emu_backend()
    be.propagate_lib = _abi.bind_propagate(C.CDLL(build_emu_propagate()))
    return be


twin_backend = K.twin_backend
_STATES, _REFS = {}, {}


def call_propagate(be, env, ub, rank=None, fixed=None, parents=None, est=None, lct=None, hyp=None, passes=256, want=PROP_OUT[1:], n=None,
                   desc=None, null=(), stride=None, win_stride=None, alias=None):
    """jss_propagate through the backend's library: (rc, {output: host array}); the outputs are prefilled (FILL), so what a call
    leaves alone can be told from what it writes"""
    lib = search.propagate_library(be)
    n = (env.batch if parents is None else len(parents)) if n is None else n
    rows = max(n, 1)
    with be.on_device():
        dev = lambda x: None if x is None else be.from_numpy(np.asarray(x, np.int32))   # noqa: E731
        full = lambda *shape: be.from_numpy(np.full(shape, FILL, np.int32))   # noqa: E731
        r, par, fx, u, e_in, l_in = dev(rank), dev(parents), S._masks_on(be, fixed), dev(np.full(rows, ub) if np.ndim(ub) == 0 else ub), dev(est), dev(lct)
        h = [None] * 3 if hyp is None else [dev(x) for x in hyp]
        shapes = dict(status=(rows,), passes_used=(rows,), est=(rows, env.jmax, env.mmax), lct=(rows, env.jmax, env.mmax))
        out = {k: full(*shapes[k]) if k == "status" or k in want else None for k in PROP_OUT}
        p = be.ptr
        region = env.jmax * env.mmax
        if stride is None:
            stride = region if rank is not None and np.ndim(rank) == 3 else 0
        if win_stride is None:
            win_stride = region if est is not None and np.ndim(est) == 3 else 0
        arg = _abi.JssPropagate(n, stride, win_stride, passes, p(par), None if "rank" in null else p(r), p(fx), None if "ub" in null else p(u),
                                None if "est_in" in null else p(e_in), None if "lct_in" in null else p(l_in),
                                *(None if f"hyp{i}" in null else p(h[i]) for i in range(3)), None if "status" in null else p(out["status"]),
                                p(out["passes_used"]), p(e_in) if alias == "est" else p(out["est"]), p(l_in) if alias == "lct" else p(out["lct"]))
        rc = lib.jss_propagate(C.byref(env._desc) if desc is None else desc, None if "state" in null else C.byref(env._state),
                               None if "arg" in null else C.byref(arg), be.stream())
        be.sync()
    return rc, {k: None if v is None else np.asarray(be.numpy(v)) for k, v in out.items()}


def same(got, ref, what, idx=None):
    rc, out = got
    assert rc == 0, (what, rc)
    for k, want in zip(PROP_OUT, ref):
        if out[k] is not None:
            want = want if idx is None else want[idx]
            assert out[k].dtype == np.int32 and np.array_equal(out[k][:len(want)], want), (what, k, out[k][:len(want)], want)


def tables_of(name):
    st = S.case_state(name)
    env = st["env"]
    return st, st["host"]["env_const"].reshape(-1, _abi.NC), st["host"]["ops"].reshape(-1, env.jmax, env.mmax)


def twin_ref(name, ub, rank, fixed, parents, est=None, lct=None, hyp=None, passes=256):
    env = S.case_state(name)["env"]
    rc, out = call_propagate(twin_backend(), env, ub, rank, fixed, parents, est, lct, hyp, passes)
    assert rc == 0
    return tuple(out[k] for k in PROP_OUT)


def mirror_ref(name, ub, rank, fixed, parents, est=None, lct=None, hyp=None, passes=256):
    _, const, ops = tables_of(name)
    return search.propagate_reference(const, ops, ub, rank, fixed, parents, est, lct, hyp, passes, fill=FILL)


def case_cands(name):
    """The case's candidates, all on env 0 but the refused ones, made once.  Three partial selections: nothing fixed; the
    bottleneck machine fixed by its Schrage starts; all used machines but the lowest fixed by the order of an unbiased shifting
    bottleneck build.  At each four trial makespans: L - 1, L, the first that propagation does not refute and the sum of all
    durations, L being relax_machines' bound of the selection.  Then machine_cases' cyclic ranks where it has some, the env never reset, a parent out of range and a negative
    makespan.  `hyp`: a random real operation per candidate with a random window, one candidate without (-1), one past the row
    (refused).  `shared`: the fixpoint of the empty selection at the sum of the durations; `own`: that table moved a little per
    candidate, one of them with an entry out of range (refused)."""
    if name in _STATES:
        return _STATES[name]
    st, const, ops = tables_of(name)
    env, B, base = st["env"], st["B"], st["base"]
    jmax, mmax = env.jmax, env.mmax
    J, M, tab = (int(const[0, x]) for x in (_abi.C_JOBS, _abi.C_MACHINES, _abi.C_TABLE))
    mach, dur = ((ops[tab] >> 16) & 63)[:J, :M], (ops[tab] & 0xFFFF)[:J, :M]
    used = sorted(set(mach.reshape(-1).tolist()))
    total = int(dur.sum())
    neck = int(st["rows"][2][0])
    schrage = np.maximum(st["rows"][7][0], 0).astype(np.int32)
    built = st["built"][0]
    order = built[1][0].astype(np.int32) if built[0][0] >= 0 else base
    all_but_one = sum(1 << m for m in used[1:])
    par, masks, ranks, ubs = [], [], [], []
    for mask, rank in ((0, base), (1 << neck if neck >= 0 else 0, schrage), (all_but_one, np.maximum(order, 0))):
        rank = np.asarray(rank, np.int32)
        L = int(search.machine_reference(const, ops, rank[None], [mask], [0])[1][0])
        start = max(L, 0)
        while True:                                                   # (the twin scans: it is held to the mirror bit for bit)
            span = start + np.arange(8)
            status = twin_ref(name, span, np.stack([rank] * 8), np.full(8, mask, np.uint64), np.zeros(8, np.int32))[0]
            if (status != 1).any():
                first = int(span[np.flatnonzero(status != 1)[0]])
                break
            start += 8
        for ub in (L - 1, L, first, total):
            par.append(0), masks.append(mask), ranks.append(rank), ubs.append(max(ub, 0))
    cyclic = np.flatnonzero((st["par"] == 0) & (st["cands"][0] == -2))
    if cyclic.size:                                                   # (machine_cases' random ranks on env 0, where they close a cycle)
        par.append(0), masks.append(int(st["masks"][cyclic[0]])), ranks.append(st["ranks"][cyclic[0]]), ubs.append(total)
    for p, ub in ((B - 1, total), (-1, total), (0, -1)):
        par.append(p), masks.append(0), ranks.append(base), ubs.append(ub)
    par, masks, ranks, ubs = np.asarray(par, np.int32), np.asarray(masks, np.uint64), np.stack(ranks), np.asarray(ubs, np.int32)
    n = par.size
    rng = np.random.default_rng(len(name) * 104729 + n)
    real = np.flatnonzero((np.arange(jmax)[:, None] < J) & (np.arange(mmax)[None, :] < M))
    hyp_op = rng.choice(real, n).astype(np.int32)
    hyp_op[1], hyp_op[2] = -1, jmax * mmax
    cap = np.maximum(ubs, 0).astype(np.int64)
    hyp = (hyp_op, rng.integers(0, cap // 2 + 1).astype(np.int32), rng.integers(cap // 2, cap + 1).astype(np.int32))
    fix = twin_ref(name, total, base, None, np.zeros(1, np.int32))
    assert fix[0][0] == 0
    shared = (fix[2][0].copy(), fix[3][0].copy())
    own_e = np.stack([np.where(shared[0] >= 0, shared[0] + c % 3, -1) for c in range(n)]).astype(np.int32)
    own_l = np.stack([np.where(shared[1] >= 0, np.maximum(shared[1] - c % 2, 0), -1) for c in range(n)]).astype(np.int32)
    own_e[3, 0, 0] = -1                                               # (an entry of a real operation out of range: refused)
    _STATES[name] = dict(par=par, masks=masks, ranks=ranks, ubs=ubs, hyp=hyp, shared=shared, own=(own_e, own_l), n=n, total=total)
    return _STATES[name]


def variants(light=0):
    """(hypothesis?, tables: none / shared / own, budget)"""
    if light == 2:
        return [(False, "none", 2)]
    if light == 1:
        return [(False, "none", 1), (True, "own", 256), (True, "shared", 2), (False, "own", 1), (False, "none", 256)]
    return list(itertools.product((False, True), ("none", "shared", "own"), BUDGETS))


def args_of(name, variant):
    cs = case_cands(name)
    with_hyp, tables, passes = variant
    est, lct = (None, None) if tables == "none" else cs[tables]
    return cs["ubs"], cs["ranks"], cs["masks"], cs["par"], est, lct, cs["hyp"] if with_hyp else None, passes


def ref_of(name, variant):
    """the mirror's outputs for the variant where the mirror is quick, the twin's elsewhere"""
    key = (name, variant)
    if key not in _REFS:
        _REFS[key] = (mirror_ref if name in MIRRORED else twin_ref)(name, *args_of(name, variant))
    return _REFS[key]


# ---- 1. against the mirror --------------------------------------------------------------------------------------------------------
def case_against_mirror(be, name, light=0):
    """every variant of the case's candidates, bit for bit: status, passes_used, est and lct; the optional outputs on their own;
    n == 0; refused, cyclic and refuted rows keep their fill; the batch is untouched.  The cases the mirror computes run all
    eighteen variants, the three it does not five of them (every budget, both kinds of tables, with and without hypotheses).
    `light` is for the emulator: 2 (the shapes beyond S.SMALL) runs one call at a budget of two passes"""
    env = S.env_on(be, name)
    before = rows_of(env)
    for variant in variants(light or int(name not in MIRRORED)):       # (the larger shapes: five variants on every backend)
        ub, rank, fixed, par, est, lct, hyp, passes = args_of(name, variant)
        ref = ref_of(name, variant)
        same(call_propagate(be, env, ub, rank, fixed, par, est, lct, hyp, passes), ref, (name, variant))
        status = ref[0]
        assert status[-3:].tolist() == [-1, -1, -1] and status[0] >= 0
        kept = (status < 0) | (status == 1)
        assert (ref[2][kept] == FILL).all() and (ref[3][kept] == FILL).all() and not (ref[2][~kept] == FILL).any()
        assert (ref[1][status < 0] == FILL).all() and (ref[1][status >= 0] >= 0).all()
    if light < 2:
        variant = (True, "shared", 2)
        ub, rank, fixed, par, est, lct, hyp, passes = args_of(name, variant)
        ref = ref_of(name, variant)
        for k in PROP_OUT[1:]:
            same(call_propagate(be, env, ub, rank, fixed, par, est, lct, hyp, passes, want=(k,)), ref, (name, "only", k))
        same(call_propagate(be, env, ub, rank, fixed, par, est, lct, hyp, passes, want=()), ref, (name, "status alone"))
        got = call_propagate(be, env, ub, rank, fixed, par, est, lct, hyp, passes, n=0)
        assert got[0] == 0 and all((x == FILL).all() for x in got[1].values())
        # one shared rank table, candidate c env c
        rows = call_propagate(be, env, case_cands(name)["total"], S.case_state(name)["base"], None, None)
        assert rows[0] == 0 and rows[1]["status"][0] == 0 and rows[1]["status"][-1] == -1
    after = rows_of(env)
    for k in before:
        assert np.array_equal(before[k], after[k]), (name, k)


def case_twin_against_mirror_reduced(name):
    """where the mirror computes no variant in full ("one-machine", "J128", "m64"): the twin against it on the candidates of the
    empty selection without hypotheses or tables -- L - 1 and L at a budget of 2 passes for m64, L alone in one pass where a
    machine holds more than a hundred operations"""
    cs = case_cands(name)
    pick, passes = (np.arange(1, 2), 1) if name in SLOW else (np.arange(2), 2)
    args = (cs["ubs"][pick], cs["ranks"][pick], cs["masks"][pick], cs["par"][pick])
    got, ref = twin_ref(name, *args, passes=passes), mirror_ref(name, *args, passes=passes)
    for k, a, b in zip(PROP_OUT, got, ref):
        assert np.array_equal(a, b), (name, k, a, b)
    return got


# ---- 2. the rules are told apart ----------------------------------------------------------------------------------------------------
def rule_runs(const, ops, ub, rank=None, fixed=None, passes=256):
    """the mirror on one candidate with all rules and with every single rule switched off: {rule or None: outputs}"""
    runs = {None: search.propagate_reference(const, ops, [ub], rank, fixed, [0], passes=passes)}
    for rule in search.PROPAGATE_RULES:
        rules = tuple(r for r in search.PROPAGATE_RULES if r != rule)
        runs[rule] = search.propagate_reference(const, ops, [ub], rank, fixed, [0], passes=passes, rules=rules)
    return runs


def triple():
    """three jobs whose first operations, two units each, share machine 0 and whose last take one unit: at a makespan of 6 they
    have the one window [0, 5], which no pair and no operation outside a task interval narrows -- only the sum does not fit"""
    return K.inst("triple", [[0, 1]] * 3, [[2, 1]] * 3)


def rule_differences(names=("ft06", "triple", "hand", "3x2", "repeats")):
    """over the candidates of the small cases and ft06: which single rules change the outcome somewhere -- "overload": a candidate
    refuted with it and at a fixpoint without; "after", "before", "pairs": a fixpoint whose windows differ without the rule;
    "budget": a candidate that two passes leave at status 2 and 256 end"""
    found = set()
    for name in names:
        if name in ("ft06", "triple"):
            env = BatchedJssEnv(ft06() if name == "ft06" else triple(), batch=1, _backend=twin_backend())
            env.reset()
            host = K.host_tables(env)
            const, ops = host["env_const"].reshape(-1, _abi.NC), host["ops"].reshape(-1, env.jmax, env.mmax)
            cands = [(ub, None, None) for ub in ((53, 54, 55, 58) if name == "ft06" else (6, 7))]
        else:
            _, const, ops = tables_of(name)
            cs = case_cands(name)
            cands = [(int(cs["ubs"][c]), cs["ranks"][c][None], [int(cs["masks"][c])]) for c in range(cs["n"] - 3)]
        for ub, rank, fixed in cands:
            runs = rule_runs(const, ops, ub, rank, fixed)
            full = runs[None]
            if full[0][0] < 0:
                continue
            if full[0][0] == 1 and runs["overload"][0][0] == 0:
                found.add("overload")
            for rule in ("after", "before", "pairs"):
                if full[0][0] == 0 and runs[rule][0][0] == 0 and not (np.array_equal(full[2], runs[rule][2]) and np.array_equal(full[3], runs[rule][3])):
                    found.add(rule)
            if full[0][0] in (0, 1) and search.propagate_reference(const, ops, [ub], rank, fixed, [0], passes=2)[0][0] == 2:
                found.add("budget")
    return found


# ---- 3. the hand cases ------------------------------------------------------------------------------------------------------------------
def case_ft06(be, mirror=False):
    """ft06 (optimum 55) through the public calls: propagation alone refutes every makespan from 47 to 53 and leaves 54, 55 and 56
    at a fixpoint; the driver's scan gives 54, one shaving round refutes it, the bound is the optimum"""
    env = BatchedJssEnv(ft06(), batch=1, _backend=be)
    env.reset()
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    ubs = np.asarray(sorted(FT06_STATUS), np.int32)
    status, used, est, lct = (n(x) for x in env.propagate(ubs, parents=np.zeros(ubs.size, np.int32), windows=True))
    print("ft06: makespans", ubs.tolist(), "status", status.tolist(), "passes", used.tolist())
    assert status.tolist() == [FT06_STATUS[int(u)] for u in ubs] and n(env.solve_machines()[0])[0] == 52
    assert (est[status == 1] == -1).all() and (est[status == 0][:, :6, :6] >= 0).all()
    if mirror:
        host = K.host_tables(env)
        ref = search.propagate_reference(host["env_const"], host["ops"].reshape(-1, 6, 6), ubs, parents=np.zeros(ubs.size, np.int64))
        assert np.array_equal(ref[0], status) and np.array_equal(ref[1], used) and np.array_equal(ref[2], est) and np.array_equal(ref[3], lct)
    res = search.destructive_bound(ft06(), upper=FT06_OPT, _backend=be)
    print("ft06: bound", res.lower_bound, "scan", res.first_bound, "one machine", res.one_machine, "launches", res.launches, "propagations", res.propagations)
    assert (res.first_bound.tolist(), res.lower_bound.tolist(), res.one_machine.tolist(), res.proved_optimal.tolist()) == ([54], [55], [52], [True])
    assert res.launches.tolist() == [3]                               # the scan, the round that refutes 54, the windows at 55
    open_end = search.destructive_bound(ft06(), rounds=2, _backend=be)
    assert open_end.lower_bound.tolist() == [55] and not open_end.proved_optimal[0]      # 55 stays open after two rounds
    assert search.destructive_bound(ft06(), shave=False, _backend=be).lower_bound.tolist() == [54]
    return status, used


def case_ta01(be):
    """ta01: 1189 is refuted, 1190 ends at a fixpoint; the scan's bound is 1190 against 1168 from solve_machines"""
    env = BatchedJssEnv("ta01", batch=1, _backend=be)
    env.reset()
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    ubs = np.asarray(sorted(TA01_STATUS), np.int32)
    status, used = (n(x) for x in env.propagate(ubs, parents=np.zeros(2, np.int32)))
    print("ta01: makespans", ubs.tolist(), "status", status.tolist(), "passes", used.tolist())
    assert status.tolist() == [TA01_STATUS[int(u)] for u in ubs]
    res = search.destructive_bound("ta01", shave=False, _backend=be)
    assert (res.first_bound.tolist(), res.lower_bound.tolist(), res.one_machine.tolist(), res.launches.tolist()) == ([1190], [1190], [1168], [1])
    return status, used


# ---- 4. brute force -------------------------------------------------------------------------------------------------------------------
def tiny_instance(rng, w):
    """a seeded tiny instance, at most 4 x 3, durations 1 to 9; every third one lets machines repeat within a job"""
    J, M = int(rng.integers(2, 5)), int(rng.integers(2, 4))
    machine = rng.integers(0, M, (J, M)) if w % 3 == 0 else np.stack([rng.permutation(M) for _ in range(J)])
    return K.inst("tiny", machine, rng.integers(1, 10, (J, M))), np.asarray(machine), None


def brute_optimum(machine, dur):
    """every order of every machine's operations, enumerated completely: (the least makespan, the starts of one schedule that has
    it, each operation as early as its order allows)"""
    J, M = machine.shape
    flat_m, d = machine.reshape(-1), np.asarray(dur, np.int64).reshape(-1)
    groups = [np.flatnonzero(flat_m == m) for m in sorted(set(flat_m.tolist()))]
    combos = list(itertools.product(*(itertools.permutations(g.tolist()) for g in groups)))
    pred = np.full((len(combos), J * M), -1, np.int64)
    for c, perms in enumerate(combos):
        for perm in perms:
            for u, v in zip(perm[:-1], perm[1:]):
                pred[c, v] = u
    start = np.zeros((len(combos), J * M), np.int64)
    job_pred = np.where(np.arange(J * M) % M > 0, np.arange(J * M) - 1, -1)
    rows = np.arange(len(combos))[:, None]
    for it in range(J * M + 1):
        end = start + d
        by_job = np.where(job_pred >= 0, end[:, np.maximum(job_pred, 0)], 0)
        by_machine = np.where(pred >= 0, end[rows, np.maximum(pred, 0)], 0)
        new = np.maximum(by_job, by_machine)
        if it == J * M:
            acyclic = (new == start).all(axis=1)
        start = new
    mk = np.where(acyclic, (start + d).max(axis=1), np.iinfo(np.int64).max)
    best = int(mk.argmin())
    return int(mk[best]), start[best].reshape(J, M)


def inside(est, lct, start, dur):
    J, M = start.shape
    return bool((est[:J, :M] <= start).all() and (start + dur <= lct[:J, :M]).all())


def case_brute_force(be, count, seed=29, prop=None):
    """`count` seeded tiny instances, each enumerated completely: no makespan at or above the optimum is refuted, with or without
    a round of shaving hypotheses; at the optimum the starts of an optimal schedule lie inside the windows; destructive_bound
    never exceeds the optimum, and where it reaches it its final windows hold that schedule too.  Returns (instances, those
    whose scan's bound exceeds the one-machine bound, those where shaving raises it further).  `prop(env, ubs)` replaces the
    propagation (the companion test's broken one)"""
    rng = np.random.default_rng(seed)
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    scan_better = shave_better = 0
    for w in range(count):
        inst, machine, _ = tiny_instance(rng, w)
        J, M = machine.shape
        dur = np.asarray(inst.duration, np.int64)
        opt, start = brute_optimum(machine, dur)
        env = BatchedJssEnv(inst, batch=1, _backend=be)
        env.reset()
        ubs = np.asarray([opt, opt + 1, opt + 4], np.int32)
        if prop is not None:
            status, est, lct = prop(env, ubs)
            assert (status != 1).all(), (w, opt, status)
            continue
        status, _, est, lct = (n(x) for x in env.propagate(ubs, parents=np.zeros(3, np.int32), windows=True))
        assert (status != 1).all(), (w, opt, status)
        assert inside(est[0], lct[0], start, dur), (w, opt)
        # the halves of every window at the optimum: the half that holds the optimal start is never refuted
        flat = np.arange(J * M)
        ops = (flat // M * env.mmax + flat % M).astype(np.int32)
        e, l, d = est[0, :J, :M].reshape(-1), lct[0, :J, :M].reshape(-1), dur.reshape(-1)   # noqa: E741
        mid = (e + l - d) // 2
        low = start.reshape(-1) <= mid
        hyp = (ops, np.where(low, e, mid + 1).astype(np.int32), np.where(low, mid + d, l).astype(np.int32))
        halves = n(env.propagate(np.full(J * M, opt, np.int32), parents=np.zeros(J * M, np.int32), est=est[0], lct=lct[0], hyp=hyp)[0])
        assert (halves != 1).all(), (w, opt, halves)
        res = search.destructive_bound(inst, _backend=be)
        assert res.one_machine[0] <= res.first_bound[0] <= res.lower_bound[0] <= opt, (w, opt, res.lower_bound)
        if res.lower_bound[0] == opt:
            assert inside(res.est[0], res.lct[0], start, dur), (w, opt)
        capped = search.destructive_bound(inst, upper=opt, _backend=be)
        assert capped.lower_bound[0] == res.lower_bound[0] and capped.proved_optimal[0] == (res.lower_bound[0] == opt)
        scan_better += int(res.first_bound[0] > res.one_machine[0])
        shave_better += int(res.lower_bound[0] > res.first_bound[0])
    return count, scan_better, shave_better


def broken_propagation(env, ubs):
    """the mirror with the overload threshold off by one: a set that exactly fills its interval counts as overloaded"""
    host = K.host_tables(env)
    out = search.propagate_reference(host["env_const"], host["ops"].reshape(-1, env.jmax, env.mmax), ubs, parents=np.zeros(len(ubs), np.int64),
                                     _overload_slack=1)
    return out[0], out[2], out[3]


# ---- 5. properties -----------------------------------------------------------------------------------------------------------------------
def check_rules_hold(const_row, ops_row, mmax, rank, mask, est, lct):
    """rules 1 to 3 of the header, checked directly on the windows of a fixpoint"""
    J, M = int(const_row[_abi.C_JOBS]), int(const_row[_abi.C_MACHINES])
    mach, d = ((ops_row >> 16) & 63)[:J, :M], (ops_row & 0xFFFF)[:J, :M].astype(np.int64)
    e, l = est[:J, :M].astype(np.int64), lct[:J, :M].astype(np.int64)   # noqa: E741
    assert (e + d <= l).all()
    assert (e[:, 1:] >= (e + d)[:, :-1]).all() and (l[:, :-1] <= (l - d)[:, 1:]).all()
    for m in sorted(set(mach.reshape(-1).tolist())):
        its = [(j, k) for j in range(J) for k in range(M) if mach[j, k] == m]
        if mask >> m & 1:
            seq = sorted(its, key=lambda o: (rank[o[0]][o[1]], o))
            for u, v in zip(seq[:-1], seq[1:]):
                assert e[v] >= e[u] + d[u] and l[u] <= l[v] - d[v]
        else:
            for i in its:
                for j in its:
                    if i != j and d[i] > 0 and d[j] > 0 and e[i] + d[i] + d[j] > l[j]:
                        assert e[i] >= e[j] + d[j] and l[j] <= l[i] - d[i]


def case_properties(be, name):
    """env 0 of the case: the windows only narrow as ub falls; a fixpoint fed back returns itself in one pass; fixing a machine by
    the order of a known schedule never refutes that schedule's makespan, and every machine fixed leaves its starts inside the
    windows; the windows of a fixpoint obey rules 1 to 3"""
    st, const, ops = tables_of(name)
    env = S.env_on(be, name)
    cs = case_cands(name)
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    J, M, tab = (int(const[0, x]) for x in (_abi.C_JOBS, _abi.C_MACHINES, _abi.C_TABLE))
    total, zero = cs["total"], np.zeros(1, np.int32)
    # narrowing
    first = int(cs["ubs"][2])
    ubs = np.asarray(sorted([total, (total + first + 1) // 2, first + 1, first], reverse=True), np.int32)
    status, used, est, lct = (n(x) for x in env.propagate(ubs, parents=np.zeros(4, np.int32), windows=True, passes=4096))
    assert (status == 0).all(), (name, status)
    for a, b in zip(range(3), range(1, 4)):
        real = est[a] >= 0
        assert (est[b][real] >= est[a][real]).all() and (lct[b][real] <= lct[a][real]).all(), (name, a)
    for c in range(4):
        again = [n(x) for x in env.propagate(ubs[c:c + 1], parents=zero, est=est[c], lct=lct[c], windows=True)]
        assert again[0].tolist() == [0] and again[1].tolist() == [1] and np.array_equal(again[2][0], est[c]) and np.array_equal(again[3][0], lct[c])
        check_rules_hold(const[0], ops[tab], env.mmax, st["base"], 0, est[c], lct[c])
    # a known schedule: an unbiased build's order, its starts and its makespan
    built = st["built"][0]
    if built[0][0] < 0:
        return
    rank = built[1][0:1].astype(np.int32)
    mk, start = (n(x) for x in env.evaluate_order(np.tile(rank, (env.batch, 1, 1)), zero, start=True))
    assert mk[0] == built[0][0]
    dur = (ops[tab] & 0xFFFF)[:J, :M].astype(np.int64)
    used_machines = sorted(set(((ops[tab] >> 16) & 63)[:J, :M].reshape(-1).tolist()))
    masks = np.asarray([0] + [sum(1 << m for m in used_machines[:i + 1]) for i in range(len(used_machines))], np.uint64)[:9]
    c = masks.size
    status, _, est, lct = (n(x) for x in env.propagate(int(mk[0]), np.tile(rank, (c, 1, 1)), masks, np.zeros(c, np.int32), windows=True, passes=4096))
    assert (status == 0).all(), (name, status)
    for i in range(c):
        assert inside(est[i], lct[i], start[0, :J, :M].astype(np.int64), dur), (name, i)
        check_rules_hold(const[0], ops[tab], env.mmax, rank[0], int(masks[i]), est[i], lct[i])
    if masks[-1] == sum(1 << m for m in used_machines) and (dur > 0).all():
        assert n(env.propagate(int(mk[0]) - 1, rank, masks[-1:], zero)[0]).tolist() == [1]      # every machine fixed: its length decides


# ---- 6. refusals and errors ------------------------------------------------------------------------------------------------------------
def case_refused_rows(be):
    """refused rows -- a parent out of range, the env never reset, a mask bit at M, a negative rank on a fixed machine, a makespan,
    a hypothesis or a window entry out of range: -1; a cyclic rank: -2 -- and refuted ones keep what they held"""
    env = S.env_on(be, "3x2")
    st = S.case_state("3x2")
    host = st["host"]
    base = st["base"]
    neg = base.copy()
    neg[0, 0] = -3
    cyc = np.array([[1, 0], [1, 1], [1, 0]], np.int32)
    par = np.array([0, 4, 3, 1, 0, 0, -1, 2, 0, 0, 0, 0, 0], np.int32)
    masks = np.array([3, 0, 0, 4, 1, 2, 0, 3, 0, 0, 0, 0, 0], np.uint64)
    ranks = np.stack([base, base, base, base, neg, neg, base, cyc, base, base, base, base, base])
    ubs = np.array([30, 30, 30, 30, 30, 30, 30, 30, -1, _abi.PROPAGATE_MAX_TIME + 1, 30, 30, 3], np.int32)
    hyp = (np.array([-1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 6, 1, -5], np.int32), np.zeros(13, np.int32), np.full(13, 30, np.int32))
    hyp[1][11] = -1
    got = call_propagate(be, env, ubs, ranks, masks, par, hyp=hyp, passes=50)
    ref = search.propagate_reference(host["env_const"], host["ops"].reshape(-1, 3, 2), ubs, ranks, masks, par, hyp=hyp, passes=50, fill=FILL)
    same(got, ref, "refused rows")
    assert got[1]["status"].tolist() == [0, -1, -1, -1, -1, 0, -1, -2, -1, -1, -1, -1, 1]
    for k in PROP_OUT[1:]:
        assert (got[1][k][[1, 2, 3, 4, 6, 7, 8, 9, 10, 11]] == FILL).all() and not (got[1][k][[0, 5]] == FILL).any(), k
    assert got[1]["passes_used"][12] == 0 and (got[1]["est"][12] == FILL).all() and (got[1]["lct"][12] == FILL).all()
    bad = np.stack([np.zeros((3, 2), np.int32)] * 2)
    bad[1, 2, 1] = _abi.PROPAGATE_MAX_TIME + 1
    wide = np.full((2, 3, 2), 40, np.int32)
    got = call_propagate(be, env, 30, None, None, np.zeros(2, np.int32), est=bad, lct=wide)
    assert got[1]["status"].tolist() == [0, -1] and (got[1]["est"][1] == FILL).all()
    fresh = BatchedJssEnv("ta01", batch=2, _backend=be)
    try:
        fresh.propagate(1300)
    except RuntimeError:
        pass
    else:
        raise AssertionError("before reset() the call must raise")


def case_abi_errors(be):
    """every code of the entry point, before anything runs: the outputs keep their fill"""
    env = S.env_on(be, "3x2")
    st = S.case_state("3x2")
    B, ranks, masks, par = env.batch, st["ranks"], st["masks"], st["par"]
    n = par.size
    tables = np.zeros((n, 3, 2), np.int32), np.full((n, 3, 2), 40, np.int32)
    hyp = (np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, 40, np.int32))

    def desc_of(desc):
        if desc is None or desc == "null":
            return None if desc is None else C.POINTER(_abi.JssDesc)()
        d = _abi.JssDesc.from_buffer_copy(env._desc)
        for k, v in desc.items():
            setattr(d, k, v)
        return C.byref(d)

    def call(desc=None, ub=40, rank=ranks, fixed=masks, parents=par, est=None, lct=None, hyp=None, passes=7, **kw):
        got = call_propagate(be, env, ub, rank, fixed, parents, est, lct, hyp, passes, desc=desc_of(desc), **kw)
        if got[0] and kw.get("n", 1):
            assert all(x is None or (x == FILL).all() for x in got[1].values()), kw
        return got[0]

    assert call(desc="null") == _abi.E_NULL and call(null=("state",)) == _abi.E_NULL and call(null=("arg",)) == _abi.E_NULL
    assert call(desc={"ops": None}) == _abi.E_NULL
    assert call(null=("status",)) == _abi.E_NULL and call(null=("ub",)) == _abi.E_NULL and call(null=("rank",)) == _abi.E_NULL
    assert call(est=tables[0], lct=tables[1], null=("est_in",)) == _abi.E_NULL and call(est=tables[0], lct=tables[1], null=("lct_in",)) == _abi.E_NULL
    for i in range(3):
        assert call(hyp=hyp, null=(f"hyp{i}",)) == _abi.E_NULL
        assert call(hyp=hyp, null=tuple(f"hyp{k}" for k in range(3) if k != i)) == _abi.E_NULL
    assert call(est=tables[0], lct=tables[1], alias="est") == _abi.E_NULL and call(est=tables[0], lct=tables[1], alias="lct") == _abi.E_NULL
    assert call(n=-1) == _abi.E_SHAPE and call(parents=None, n=B + 1) == _abi.E_SHAPE and call(parents=None, n=B - 1) == _abi.E_SHAPE
    assert call(desc={"jmax": 0}) == _abi.E_SHAPE and call(desc={"mmax": 65}) == _abi.E_SHAPE and call(desc={"batch": -1}) == _abi.E_SHAPE
    assert call(desc={"kernel": 64}) == _abi.E_KIND
    assert call(passes=0) == _abi.E_SHAPE and call(passes=-1) == _abi.E_SHAPE and call(passes=_abi.PROPAGATE_MAX_PASSES + 1) == _abi.E_SHAPE
    assert call(stride=5) == _abi.E_SHAPE and call(win_stride=5) == _abi.E_SHAPE and call(desc={"jmax": env.jmax + 1}) == _abi.E_SHAPE
    assert call(passes=1) == 0 and call(passes=_abi.PROPAGATE_MAX_PASSES) == 0 and call(n=0) == 0 and call() == 0
    assert call(rank=None, fixed=None) == 0 and call(fixed=None) == 0 and call(want=()) == 0
    assert call(est=tables[0], lct=tables[1], hyp=hyp) == 0 and call(est=tables[0][0], lct=tables[1][0]) == 0
    # a row of more than 2144 entries does not fit one candidate's 64 KB of LDS: both libraries say so; 100 x 20 and 128 x 16 fit
    # (not run)
    shared = st["base"]
    assert call(desc={"jmax": 128, "mmax": 17}, rank=shared) == _abi.E_LDS
    assert call(desc={"jmax": 128, "mmax": 16}, rank=shared, n=0) == 0 and call(desc={"jmax": 100, "mmax": 20}, rank=shared, n=0) == 0


# ---- 7. the built library ------------------------------------------------------------------------------------------------------------------
def propagate_kernel_rows():
    """[(name, vgprs, sgprs, spilled vgprs, spilled sgprs, scratch bytes, static LDS bytes)] of libjss_propagate_hip.so"""
    import re
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import LLVM, kernel_resources
    from jssenv_amd.build import build_propagate_extension
    so = build_propagate_extension()                                  # (built here if build() has not run)
    rows = kernel_resources(so)
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "propagate.co")
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


# ---- 8. the drivers --------------------------------------------------------------------------------------------------------------------------
DRIVER_FIELDS = ("lower_bound", "first_bound", "one_machine", "est", "lct", "launches", "propagations", "proved_optimal")


def small_instances():
    return dict(ft06=ft06(), hand=D.hand_instance(), **{"3x2": K.inst("three", [[0, 1], [0, 1], [1, 0]], [[2, 3], [4, 1], [5, 2]])})


def case_driver(be, names=("ft06", "3x2", "hand")):
    """destructive_bound on the backend is destructive_reference, field for field: one instance, a list of them, with and without
    an upper bound and shaving; two runs are identical"""
    insts = small_instances()
    for name in names:
        for kw in (dict(), dict(shave=False), dict(upper=FT06_OPT if name == "ft06" else 11), dict(rounds=1, span=3)):
            got, ref = search.destructive_bound(insts[name], _backend=be, **kw), search.destructive_reference(insts[name], **kw)
            for f in DRIVER_FIELDS:
                assert np.array_equal(getattr(got, f), getattr(ref, f)), (name, kw, f, getattr(got, f), getattr(ref, f))
    several = [insts[k] for k in names]
    got, again, ref = (search.destructive_bound(several, _backend=be), search.destructive_bound(several, _backend=be),
                       search.destructive_reference(several))
    for f in DRIVER_FIELDS:
        assert np.array_equal(getattr(got, f), getattr(ref, f)) and np.array_equal(getattr(got, f), getattr(again, f)), f
    return got
