"""Backend-agnostic cases of jss_machine_relax and jss_bottleneck_build (include/jss_machine.h), BatchedJssEnv.relax_machines /
bottleneck and search.bottleneck_search, run against the host-core twin, the kernel source (jssenv_amd/csrc/jss_machine.hip) under
the SIMT emulator and the HIP library libjss_machine_hip.so.

The references are search.machine_reference and search.bottleneck_reference (NumPy, written from the header's definition).  A
case's batch, rank tables, masks and candidate list are made once, on the twin, and its references once; another backend builds
the same batch (only env_const and the instance tables are read, which a reset writes identically everywhere) and is compared
with them bit for bit."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np

import order_cases as K
import decode_cases as D
from clone_cases import rows_of
from jssenv_amd import BatchedJssEnv, _abi, search
from jssenv_amd import instances as I

ROOT = K.ROOT
MACHINE_SRC = os.path.join(ROOT, "jssenv_amd", "csrc", "jss_machine.hip")
EMU_LIB = os.path.join(K.EMU, "libjss_machine_emu.so")
FILL = K.FILL                       # what the outputs hold before a call: the rows of refused and cyclic candidates keep it
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
U64 = 2 ** 64 - 1
RELAX_OUT = ("length", "lower_bound", "bottleneck", "jps", "schrage", "head", "tail", "rank_out")
BUILD_OUT = ("makespan", "rank", "info", "order")

# The hand case: decode_cases' 3 jobs x 3 machines.  Nothing fixed: the heads are the sums of the durations before an operation
# in its job, the tails the sums behind it, the length the longest job.  Machine 0 holds (0,1) r5 p2 q3, (1,1) r1 p3 q3 and (2,2)
# r6 p1 q0: (1,1) runs 1-4, (0,1) 5-7 (released alone at 5; (2,2), released at 6, has the smaller q), (2,2) 7-8: max(4+3, 7+3,
# 8+0) = 10, preemptive or not.  Machine 1 holds (0,0) r0 p5 q5, (1,2) r4 p3 q0, (2,1) r3 p3 q1: (0,0) 0-5, (2,1) 5-8, (1,2) 8-11:
# max(10, 9, 11) = 11.  Machine 2 holds (0,2) r7 p3 q0, (1,0) r0 p1 q6, (2,0) r0 p3 q4: (1,0) 0-1, (2,0) 1-4, (0,2) 7-10: 10.
# With machine 0 fixed in that order -- (1,1), (0,1), (2,2), the Schrage starts 1, 5, 7 as ranks -- head(2,2) = head(0,1) + 2 = 7,
# tail(1,1) = d(0,1) + tail(0,1) = 2 + 3 = 5 and tail(1,0) = d(1,1) + tail(1,1) = 8; nothing else moves.
HAND_FREE = dict(length=10, lower_bound=11, bottleneck=1, jps=[10, 11, 10], schrage=[10, 11, 10],
                 head=[[0, 5, 7], [0, 1, 4], [0, 3, 6]], tail=[[5, 3, 0], [6, 3, 0], [4, 1, 0]],
                 rank_out=[[0, 5, 7], [0, 1, 8], [1, 5, 7]])
HAND_M0 = dict(length=10, lower_bound=11, bottleneck=1, jps=[-1, 11, 10], schrage=[-1, 11, 10],
               head=[[0, 5, 7], [0, 1, 4], [0, 3, 7]], tail=[[5, 3, 0], [8, 5, 0], [4, 1, 0]],
               rank_out=[[0, 5, 7], [0, 1, 8], [1, 5, 7]])
HAND_BUILD = dict(makespan=11, rank=[[0, 5, 7], [0, 1, 8], [1, 5, 8]], order=[1, 0, 2], info={0: [3, 0, 0, 11], 1: [3, 3, 0, 11], 2: [3, 6, 0, 11]})
# durations of 0 whose Schrage starts tie: the unbiased build turns cyclic (found by a seeded search over tiny instances)
CYCLIC_MACHINE = [[1, 0, 2], [0, 2, 1], [1, 2, 0]]
CYCLIC_DURATION = [[1, 0, 0], [0, 2, 0], [0, 0, 0]]
CYCLIC_REOPT = 0

# prototype values of the header's definitions: the bound of the empty selection; unbiased builds, (reopt, instance) -> makespan
ANCHOR_BOUND = dict(ta01=1168, ta02=1143, ta11=1254, ta21=1435, ta41=1850, ta61=2868, ta71=5464)
ANCHOR_BUILD = {(0, "ta01"): 1633, (0, "ta02"): 1794, (0, "ta11"): 1928, (0, "ta21"): 2300, (0, "ta41"): 2894, (0, "ta61"): 4300,
                (0, "ta71"): 7625, (1, "ta01"): 1475, (1, "ta02"): 1444, (1, "ta11"): 1592, (1, "ta21"): 2030, (1, "ta41"): 2542,
                (3, "ta01"): 1402}
ANCHOR_INFO = {(1, "ta01"): (15, 105, 28, 1168), (3, "ta01"): (15, 315, 32, 1168)}
GPU_ANCHORS = ("ta01", "ta41")


def build_emu_machine():
    """jss_machine.hip, unmodified, compiled with g++ against the SIMT emulator's hip_runtime.h: a library of its own"""
    deps = [MACHINE_SRC, os.path.join(K.EMU, "hip", "hip_runtime.h"), os.path.join(ROOT, "jssenv_amd", "csrc", "jss_abi_checks.hpp"),
            os.path.join(ROOT, "include", "jss_machine.h")]
    if not os.path.isfile(EMU_LIB) or any(os.path.getmtime(d) > os.path.getmtime(EMU_LIB) for d in deps):
        tmp = EMU_LIB + f".tmp{os.getpid()}"
        subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
                               "-Wno-unknown-pragmas", "-I" + K.EMU, "-I" + os.path.join(ROOT, "include"), MACHINE_SRC, "-o", tmp])
        os.replace(tmp, EMU_LIB)
    return EMU_LIB


def emu_backend():
    """order_cases' emulator backend (the env kernels, jss_order.hip) with the emulated machine library as its `machine_lib`"""
    be = K.emu_backend()
    be.machine_lib = _abi.bind_machine(C.CDLL(build_emu_machine()))
    return be


twin_backend = K.twin_backend


# ---- the batches -----------------------------------------------------------------------------------------------------------------
def _taillard(jobs, machines, seed):
    return I.taillard_instance(jobs, machines, 5000 + seed, 6000 + seed, name=f"syn{jobs}x{machines}")


def _all_on_one(jobs, ops):
    """every operation on machine 0: one machine holds jobs * ops operations, the others none"""
    rng = np.random.default_rng(jobs * 100 + ops)
    return K.inst(f"one{jobs}x{ops}", np.zeros((jobs, ops), np.int32), rng.integers(1, 30, (jobs, ops)))


# name -> (constructor on a backend, envs).  The last env of every batch is never reset.  "M1": as in decode_cases, the envs of a
# 5 x 2 batch get M = 1 written into their env_const after the reset.  "one-machine": 160 operations on machine 0 (positions
# strided over the lanes), machines 1 to 3 unused.  "m64": 64 machines, so that bit 63 of a mask is a machine.
OWN = {
    "hand": (lambda be: BatchedJssEnv(D.hand_instance(), batch=3, _backend=be, seed=41), 3),
    "zeros": (lambda be: BatchedJssEnv(D.zeros_instance(), batch=3, _backend=be, seed=42), 3),
    "J1": (lambda be: BatchedJssEnv(K.inst("one4", [[2, 0, 3, 1]], [[4, 9, 2, 6]]), batch=3, _backend=be, seed=43), 3),
    "M1": (lambda be: BatchedJssEnv(K.inst("five2", [[0, 1]] * 5, [[3, 1], [5, 1], [2, 1], [7, 1], [4, 1]]), batch=3, _backend=be, seed=44), 3),
    "J64": (lambda be: BatchedJssEnv(_taillard(64, 3, 1), batch=2, _backend=be, seed=45), 2),
    "J128": (lambda be: BatchedJssEnv(_taillard(128, 2, 2), batch=2, _backend=be, seed=46), 2),
    "one-machine": (lambda be: BatchedJssEnv(_all_on_one(40, 4), batch=2, _backend=be, seed=47), 2),
    "m64": (lambda be: BatchedJssEnv(_taillard(3, 64, 3), batch=2, _backend=be, seed=48), 2),
}
REUSED = ("3x2", "repeats", "ta01", "J65", "table-of-env")
CASES = dict({name: K.CASES[name] for name in REUSED}, **OWN)
SMALL = ("hand", "zeros", "J1", "M1", "3x2", "repeats")           # what the emulator runs in full
_STATES = {}


def make_env(be, name):
    """the case's batch on `be`: every env but the last reset"""
    make, B = CASES[name]
    env = make(be)
    which = np.ones(B, np.uint8)
    which[B - 1] = 0
    env.reset(which=which)
    if name == "M1":
        env.env_const[:B - 1, _abi.C_MACHINES] = 1
        env.synchronize()
    return env


def reopts_of(name):
    """the re-optimisation rounds a case's builds are run with"""
    return (0, 1, 2) if name in SMALL else (0, 1)


def base_rank(jmax, mmax):
    """an order that is acyclic on every instance and for every subset of machines: by operation index, then by job"""
    return (np.arange(mmax)[None, :] * jmax + np.arange(jmax)[:, None]).astype(np.int32)


def case_state(name):
    """The case's batch on the twin and what is derived from it, made once.  `relax`: per reset env the candidates (mask, rank)
    = (nothing fixed, base), (all fixed, base), (a random subset, base), (the subset, random ranks -- often cyclic), (all fixed,
    random ranks), (the subset, base with negative ranks on the free machines: ignored), (all fixed, base with one negative
    rank: refused), (a bit at M: refused, where M < 64); then the env never reset and parents out of range.  `build`: per reset
    env an unbiased candidate, one with small biases, one with biases near INT32_MAX (the sum needs 64 bits); then the refused
    parents; and the same candidates going on from the base order of a random subset."""
    if name in _STATES:
        return _STATES[name]
    B = CASES[name][1]
    env = make_env(twin_backend(), name)
    host = K.host_tables(env)
    jmax, mmax = env.jmax, env.mmax
    const = host["env_const"].reshape(-1, _abi.NC)
    ops = host["ops"].reshape(-1, jmax, mmax)
    rng = np.random.default_rng(len(name) * 7919 + B)
    base = base_rank(jmax, mmax)
    par, masks, ranks, refused = [], [], [], []
    bpar, bias, brefused, sub_of = [], [], [], []
    for i in range(B - 1):
        J, M, tab = (int(const[i, x]) for x in (_abi.C_JOBS, _abi.C_MACHINES, _abi.C_TABLE))
        mach = (ops[tab] >> 16) & 63
        full = (1 << M) - 1
        sub = int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2)) & full
        if name == "m64":
            sub |= 1 << 63
        rnd = rng.integers(0, 4, (jmax, mmax)).astype(np.int32)
        free_neg = np.where((sub >> mach.astype(np.uint64).astype(object) & 1).astype(bool), base, -5).astype(np.int32)
        fixed_neg = base.copy()
        fixed_neg[int(rng.integers(0, J)), int(rng.integers(0, M))] = -1
        for mask, rank, bad in ((0, base, 0), (full, base, 0), (sub, base, 0), (sub, rnd, 0), (full, rnd, 0), (sub, free_neg, 0), (full, fixed_neg, 1)):
            par.append(i), masks.append(mask), ranks.append(rank), refused.append(bool(bad))
        if M < 64:
            par.append(i), masks.append(1 << M), ranks.append(base), refused.append(True)
        kinds = (np.zeros(mmax, np.int64), rng.integers(0, 60, mmax), rng.integers(I32_MAX - 50, I32_MAX, mmax, dtype=np.int64))
        for b in (kinds if name in SMALL else kinds[i % 3:i % 3 + 1]):        # (the mirror takes a second per build at 15 x 15)
            bpar.append(i), bias.append(b), brefused.append(False), sub_of.append(sub)
    for p in (B - 1, -1, B, I32_MAX, I32_MIN):
        par.append(p), masks.append(0), ranks.append(base), refused.append(True)
        bpar.append(p), bias.append(np.zeros(mmax, np.int64)), brefused.append(True), sub_of.append(0)
    par, masks, ranks = np.asarray(par, np.int64).astype(np.int32), np.asarray(masks, np.uint64), np.stack(ranks)
    bpar, bias, sub_of = np.asarray(bpar, np.int64).astype(np.int32), np.stack(bias).astype(np.int32), np.asarray(sub_of, np.uint64)
    ref = lambda rank, fixed, parents: search.machine_reference(const, ops, rank, fixed, parents, fill=FILL)   # noqa: E731
    build = lambda reopt, b, **kw: search.bottleneck_reference(const, ops, bpar, b, reopt, fill=FILL, **kw)   # noqa: E731
    start_rank = np.stack([base] * bpar.size)
    st = dict(env=env, host=host, B=B, par=par, masks=masks, ranks=ranks, refused=np.asarray(refused), base=base,
              rows=ref(None, None, None), cands=ref(ranks, masks, par), shared=ref(base, masks, par),
              bpar=bpar, bias=bias, brefused=np.asarray(brefused), sub_of=sub_of, start_rank=start_rank,
              built={r: build(r, bias) for r in reopts_of(name)}, plain=build(1, None) if name in SMALL else None,
              resumed=build(1, bias, rank=start_rank, fixed=sub_of), resumed0=build(0, bias, rank=start_rank, fixed=sub_of))
    _STATES[name] = st
    return st


def env_on(be, name):
    return case_state(name)["env"] if be is twin_backend() else make_env(be, name)


def _masks_on(be, masks):
    return None if masks is None else be.from_numpy(np.asarray(masks, np.uint64).view(np.int64))


def call_relax(be, env, rank=None, fixed=None, parents=None, want=RELAX_OUT[1:], n=None, desc=None, null=(), stride=None, alias=False):
    """jss_machine_relax through the backend's library: (rc, {output: host array}); the outputs are prefilled (FILL), so what a
    call leaves alone can be told from what it writes"""
    lib = search.machine_library(be)
    n = (env.batch if parents is None else len(parents)) if n is None else n
    rows = max(n, 1)
    with be.on_device():
        dev = lambda x: None if x is None else be.from_numpy(np.asarray(x, np.int32))   # noqa: E731
        full = lambda *shape: be.from_numpy(np.full(shape, FILL, np.int32))   # noqa: E731
        r, par, fx = dev(rank), dev(parents), _masks_on(be, fixed)
        shapes = dict(length=(rows,), lower_bound=(rows,), bottleneck=(rows,), jps=(rows, env.mmax), schrage=(rows, env.mmax),
                      head=(rows, env.jmax, env.mmax), tail=(rows, env.jmax, env.mmax), rank_out=(rows, env.jmax, env.mmax))
        out = {k: full(*shapes[k]) if k == "length" or k in want else None for k in RELAX_OUT}
        p = be.ptr
        if stride is None:
            stride = env.jmax * env.mmax if rank is not None and np.ndim(rank) == 3 else 0
        arg = _abi.JssMachineRelax(n, stride, p(par), None if "rank" in null else p(r), p(fx), None if "length" in null else p(out["length"]),
                                   *(p(out[k]) for k in RELAX_OUT[1:7]), p(r) if alias else p(out["rank_out"]))
        rc = lib.jss_machine_relax(C.byref(env._desc) if desc is None else desc, None if "state" in null else C.byref(env._state),
                                   None if "arg" in null else C.byref(arg), be.stream())
        be.sync()
    return rc, {k: None if v is None else np.asarray(be.numpy(v)) for k, v in out.items()}


def call_build(be, env, parents=None, bias=None, reopt=1, rank=None, fixed=None, want=("info", "order"), n=None, desc=None, null=(), alias=False):
    """jss_bottleneck_build through the backend's library: (rc, {output: host array}), prefilled like call_relax's"""
    lib = search.machine_library(be)
    n = (env.batch if parents is None else len(parents)) if n is None else n
    rows = max(n, 1)
    with be.on_device():
        dev = lambda x: None if x is None else be.from_numpy(np.asarray(x, np.int32))   # noqa: E731
        full = lambda *shape: be.from_numpy(np.full(shape, FILL, np.int32))   # noqa: E731
        r, par, fx, bs = dev(rank), dev(parents), _masks_on(be, fixed), dev(bias)
        out = dict(makespan=full(rows), rank=full(rows, env.jmax, env.mmax), info=full(rows, _abi.BOTTLENECK_NI) if "info" in want else None,
                   order=full(rows, env.mmax) if "order" in want else None)
        p = be.ptr
        arg = _abi.JssBottleneck(n, reopt, p(par), p(r), p(fx), p(bs), None if "makespan" in null else p(out["makespan"]),
                                 None if "rank" in null else p(r) if alias else p(out["rank"]), p(out["info"]), p(out["order"]))
        rc = lib.jss_bottleneck_build(C.byref(env._desc) if desc is None else desc, None if "state" in null else C.byref(env._state),
                                      None if "arg" in null else C.byref(arg), be.stream())
        be.sync()
    return rc, {k: None if v is None else np.asarray(be.numpy(v)) for k, v in out.items()}


def same(got, ref, names, what):
    rc, out = got
    assert rc == 0, (what, rc)
    n = ref[0].size
    for k, want in zip(names, ref):
        if out[k] is not None:
            assert out[k].dtype == np.int32 and np.array_equal(out[k][:n], want), (what, k, out[k][:n], want)


def case_against_mirror(be, name, light=0):
    """jss_machine_relax: per-candidate tables on the candidate list, the rows with nothing fixed, the shared table, every
    optional output on its own, n == 0; jss_bottleneck_build: the biased candidates at every reopt of the case, without a bias,
    going on from a partial selection, without the optional outputs.  Refused and cyclic rows keep their fill; the batch is
    untouched.  `light` is for the emulator, which takes a fifth of a millisecond per decision: 1 leaves out most of the
    combinations of optional outputs; 2 (the larger shapes) runs env 0's candidates and the refused parents through one relax
    call and one reopt-0 build -- which goes on from the partial selection where the case has more than 32 machines"""
    st = case_state(name)
    env = env_on(be, name)
    before = rows_of(env)
    par, masks, ranks = st["par"], st["masks"], st["ranks"]
    pick = np.flatnonzero((par == 0) | (par < 0) | (par >= st["B"] - 1)) if light == 2 else np.arange(par.size)
    of = lambda ref, idx: tuple(r[idx] for r in ref)   # noqa: E731
    same(call_relax(be, env, ranks[pick], masks[pick], par[pick]), of(st["cands"], pick), RELAX_OUT, (name, "candidates"))
    length = st["cands"][0]
    assert np.array_equal(length == -1, st["refused"]) and not st["refused"][0] and length[0] >= 0
    dead = length < 0
    for k, rows in zip(RELAX_OUT[1:], st["cands"][1:]):
        assert (rows[dead] == FILL).all() and not (rows[~dead] == FILL).any(), (name, k)
    if light < 2:
        same(call_relax(be, env), st["rows"], RELAX_OUT, (name, "rows"))
        same(call_relax(be, env, st["base"], masks, par), st["shared"], RELAX_OUT, (name, "shared"))
        for k in (RELAX_OUT[1:] if not light else ("jps", "rank_out")):
            same(call_relax(be, env, ranks, masks, par, want=(k,)), st["cands"], RELAX_OUT, (name, "only", k))
        same(call_relax(be, env, ranks, masks, par, want=()), st["cands"], RELAX_OUT, (name, "length alone"))
        got = call_relax(be, env, ranks, masks, par, n=0)
        assert got[0] == 0 and all((x == FILL).all() for x in got[1].values())
    bpar, bias = st["bpar"], st["bias"]
    pick = np.flatnonzero((bpar == 0) | (bpar < 0) | (bpar >= st["B"] - 1)) if light == 2 else np.arange(bpar.size)
    if light == 2 and env.mmax > 32:
        same(call_build(be, env, bpar[pick], bias[pick], 0, st["start_rank"][pick], st["sub_of"][pick]), of(st["resumed0"], pick), BUILD_OUT,
             (name, "resumed, reopt 0"))
    else:
        for reopt in ((0,) if light == 2 else reopts_of(name)):
            same(call_build(be, env, bpar[pick], bias[pick], reopt), of(st["built"][reopt], pick), BUILD_OUT, (name, "build", reopt))
    mk = st["built"][0][0]
    assert np.array_equal(mk == -1, st["brefused"])
    dead = mk < 0
    for k, rows in zip(BUILD_OUT[1:], st["built"][0][1:]):
        assert (rows[dead] == FILL).all() and not (rows[~dead] == FILL).any(), (name, k)
    if light < 2:
        if st["plain"] is not None and not light:
            same(call_build(be, env, bpar, None, 1), st["plain"], BUILD_OUT, (name, "no bias"))
        same(call_build(be, env, bpar, bias, 1, st["start_rank"], st["sub_of"]), st["resumed"], BUILD_OUT, (name, "resumed"))
        same(call_build(be, env, bpar, bias, 1, want=()), st["built"][1], BUILD_OUT, (name, "no optional outputs"))
        got = call_build(be, env, bpar, bias, 1, n=0)
        assert got[0] == 0 and all((x == FILL).all() for x in got[1].values())
    after = rows_of(env)
    for k in before:
        assert np.array_equal(before[k], after[k]), (name, k)


def what_the_cases_cover():
    """the shapes and paths the issue lists, read off the cases' states"""
    shape = lambda name: (case_state(name)["env"].jmax, case_state(name)["env"].mmax)   # noqa: E731
    assert {name: shape(name) for name in OWN} == {"hand": (3, 3), "zeros": (4, 3), "J1": (1, 4), "M1": (5, 2), "J64": (64, 3),
                                                    "J128": (128, 2), "one-machine": (40, 4), "m64": (3, 64)}
    assert shape("J65") == (65, 4) and shape("repeats") == (3, 4)
    assert case_state("M1")["host"]["env_const"].reshape(-1, _abi.NC)[:2, _abi.C_MACHINES].tolist() == [1, 1]
    one = case_state("one-machine")["rows"]
    assert (one[3][0, 1:] == -1).all() and one[3][0, 0] > 0 and one[2][0] == 0        # 160 operations on machine 0, three machines unused
    assert (case_state("repeats")["rows"][3][0] == -1).sum() == 1                      # a machine the instance never uses
    assert (case_state("m64")["masks"] >> np.uint64(63)).any()
    assert (case_state("zeros")["host"]["ops"] & 0xFFFF == 0).sum() >= 6
    for name in CASES:
        length = case_state(name)["cands"][0]
        assert (length >= 0).sum() >= 4 and (length == -1).sum() >= 6, name
    assert any((case_state(name)["cands"][0] == -2).any() for name in ("hand", "3x2", "repeats", "ta01"))    # a cyclic rank
    assert len(set(case_state("table-of-env")["par"][case_state("table-of-env")["cands"][0] >= 0].tolist())) >= 3   # mixed parents


def case_hand(be, mirror=False):
    """the hand case through the public calls: nothing fixed, machine 0 fixed with the first answer's rank_out, the builds"""
    env = env_on(be, "hand")
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    order = ("lower_bound", "length", "bottleneck", "jps", "schrage", "head", "tail", "rank_out")
    free = [n(x) for x in env.relax_machines(jps=True, schrage=True, head=True, tail=True, rank_out=True)]
    for k, got in zip(order, free):
        assert got[0].tolist() == HAND_FREE[k] and got[1].tolist() == HAND_FREE[k], (k, got[0])
        assert (got[2] == -1).all()                                    # (the env never reset)
    m0 = [n(x) for x in env.relax_machines(free[7], 1, jps=True, schrage=True, head=True, tail=True, rank_out=True)]
    for k, got in zip(order, m0):
        assert got[0].tolist() == HAND_M0[k], (k, got[0])
    for reopt, info in HAND_BUILD["info"].items():
        mk, rank, nf, fixed_order = (n(x) for x in env.bottleneck(reopt=reopt, order=True))
        assert mk.tolist() == [11, 11, -1] and rank[0].tolist() == HAND_BUILD["rank"] and nf[0].tolist() == info, (reopt, mk, nf)
        assert fixed_order[0].tolist() == HAND_BUILD["order"] and n(env.evaluate_order(rank)).tolist() == [11, 11, -1]
    if mirror:
        host = K.host_tables(env)
        ref = search.machine_reference(host["env_const"], host["ops"].reshape(-1, 3, 3))
        for k, got in zip(RELAX_OUT, ref):
            assert got[0].tolist() == HAND_FREE[k], k


def case_cyclic_build(be):
    """durations of 0: the unbiased build of this instance turns cyclic (-2), and its rows keep their fill"""
    inst = D.inst_with_zeros("cyclic", CYCLIC_MACHINE, CYCLIC_DURATION)
    env = BatchedJssEnv(inst, batch=1, _backend=be)
    env.reset()
    host = K.host_tables(env)
    ref = search.bottleneck_reference(host["env_const"], host["ops"].reshape(-1, env.jmax, env.mmax), None, None, CYCLIC_REOPT, fill=FILL)
    assert ref[0].tolist() == [-2] and all((x == FILL).all() for x in ref[1:])
    same(call_build(be, env, None, None, CYCLIC_REOPT), ref, BUILD_OUT, "cyclic build")


def case_anchor(be, name, reopts=(0, 1), mirror=False):
    """B = 1: the bound of the empty selection and the unbiased builds of the listed instance"""
    env = BatchedJssEnv(name, batch=1, _backend=be)
    env.reset()
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    lower, length, neck = (n(x) for x in env.relax_machines())
    print(name, "lower_bound", lower, "length", length, "bottleneck", neck)
    assert lower.tolist() == [ANCHOR_BOUND[name]] and length[0] <= lower[0] and neck[0] >= 0
    if getattr(be, "bound_lib", None) is not None or hasattr(be.lib, "jss_bound"):
        assert lower[0] >= n(env.lower_bound())[0]
    for reopt in reopts:
        if (reopt, name) not in ANCHOR_BUILD:
            continue
        mk, rank, info = (n(x) for x in env.bottleneck(reopt=reopt))
        print(name, "reopt", reopt, "makespan", mk, "info", info)
        assert mk.tolist() == [ANCHOR_BUILD[(reopt, name)]] and info[0, 3] == ANCHOR_BOUND[name]
        if (reopt, name) in ANCHOR_INFO:
            assert tuple(info[0].tolist()) == ANCHOR_INFO[(reopt, name)]
        assert np.array_equal(n(env.evaluate_order(rank)), mk)
        if mirror and env.jmax * env.mmax <= 400:
            host = K.host_tables(env)
            ref = search.bottleneck_reference(host["env_const"], host["ops"].reshape(-1, env.jmax, env.mmax), reopt=reopt)
            assert np.array_equal(ref[0], mk) and np.array_equal(ref[1], rank) and np.array_equal(ref[2], info)


# ---- properties ------------------------------------------------------------------------------------------------------------------
def subset_bound(r, p, q):
    """brute force: the largest min r + sum p + min q over the non-empty subsets"""
    idx = range(len(r))
    return max(min(r[i] for i in s) + sum(p[i] for i in s) + min(q[i] for i in s)
               for size in range(1, len(r) + 1) for s in itertools.combinations(idx, size))


def best_completion(be, inst, rank, mask, mach, limit=3000):
    """brute force: the shortest schedule over every order of the free machines' operations, the fixed machines as ranked, each
    order one env's row of evaluate_order; None where that is more than `limit` orders"""
    J, M = mach.shape
    free = [m for m in sorted(set(mach.reshape(-1).tolist())) if not mask >> m & 1]
    ops_of = {m: [(j, k) for j in range(J) for k in range(M) if mach[j, k] == m] for m in free}
    count = 1
    for m in free:
        count *= int(np.prod(np.arange(1, len(ops_of[m]) + 1)))
    if count > limit:
        return None
    tables = []
    for perms in itertools.product(*(itertools.permutations(ops_of[m]) for m in free)):
        t = np.array(rank, np.int32)
        for perm in perms:
            for pos, (j, k) in enumerate(perm):
                t[j, k] = pos
        tables.append(t)
    env = BatchedJssEnv(inst, batch=len(tables), _backend=be)
    env.reset()
    mk = np.asarray(be.numpy(env.evaluate_order(np.stack(tables))))
    return int(mk[mk >= 0].min()) if (mk >= 0).any() else None


def check_properties(be, env, rng, what, inst=None):
    """env 0 of a positive-duration batch: see the asserts.  Returns (one-machine problems checked by brute force, selections
    whose bound was checked against the best completion)"""
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    host = K.host_tables(env)
    const = host["env_const"].reshape(-1, _abi.NC)
    J, M, tab = (int(const[0, x]) for x in (_abi.C_JOBS, _abi.C_MACHINES, _abi.C_TABLE))
    ops = host["ops"].reshape(-1, env.jmax, env.mmax)[tab, :J, :M]
    mach, dur = (ops >> 16) & 63, ops & 0xFFFF
    zero = np.zeros(1, np.int32)
    retime = lambda rank, **kw: env.evaluate_order(np.tile(n(rank), (env.batch, 1, 1)), zero, **kw)   # noqa: E731
    # a build: never cyclic on positive durations, a complete order that re-times to its makespan, fixed machine by machine
    mk, order_rank, info, fixed_order = (n(x) for x in env.bottleneck(zero, rng.integers(0, 20, (1, env.mmax)), int(rng.integers(0, 3)), order=True))
    used = sorted(set(mach.reshape(-1).tolist()))
    assert mk[0] >= 0 and n(retime(order_rank))[0] == mk[0] and info[0, 0] == len(used) and mk[0] >= info[0, 3], what
    assert sorted(fixed_order[0][:len(used)].tolist()) == used and (fixed_order[0][len(used):] == -1).all()
    solved, bounded = 0, 0
    rank, mask = order_rank, 0
    for step in range(len(used) + 1):
        lower, length, neck, jps, sch, head, tail, rank_out = (n(x) for x in env.relax_machines(rank, mask, zero, True, True, True, True, True))
        assert length[0] >= 0 and lower[0] == max(length[0], jps[0].max()), (what, step)
        assert step or lower[0] <= mk[0], what                         # (the empty selection's bound holds for every schedule)
        for m in range(env.mmax):
            its = [(j, k) for j in range(J) for k in range(M) if mach[j, k] == m]
            if mask >> m & 1 or not its:
                assert jps[0, m] == -1 and sch[0, m] == -1
                continue
            r, p, q = ([int(x[0, j, k]) for j, k in its] for x in (head, dur[None], tail))
            assert jps[0, m] <= sch[0, m] < jps[0, m] + max(max(p), 1), (what, m)          # Carlier: Schrage is within p_max of the bound
            if inst is not None and len(its) <= 8:
                assert jps[0, m] == subset_bound(r, p, q), (what, m)
                solved += 1
        if inst is not None and J * M <= 9:
            best = best_completion(be, inst, rank[0], mask, mach)
            if best is not None:
                assert lower[0] <= best, (what, step, lower, best)
                bounded += 1
        if neck[0] < 0:
            # every used machine fixed: jss_order_eval's makespan, starts and tails
            again, start, tails = (n(x) for x in retime(rank, start=True, tail=True))
            assert again[0] == length[0] == lower[0] and np.array_equal(start, head) and np.array_equal(tails, tail), what
            break
        # rank_out fed back with the bottleneck's bit set: an acyclic selection
        assert jps[0, neck[0]] == jps[0].max()
        rank, mask = rank_out, mask | 1 << int(neck[0])
        assert n(env.relax_machines(rank, mask, zero)[1])[0] >= 0, (what, step)
    assert step == len(used)
    return solved, bounded


def case_seeded_properties(be, count, seed=11):
    """`count` seeded tiny instances: 2-4 jobs, 2-4 operations each on machines that may repeat or stay unused, durations 1-9"""
    rng = np.random.default_rng(seed)
    solved = bounded = 0
    for w in range(count):
        J, M = int(rng.integers(2, 5)), int(rng.integers(2, 5))
        if w % 3 == 0:
            J, M = min(J, 3), min(M, 3)
        machine = np.stack([rng.permutation(M) for _ in range(J)]) if rng.random() < 0.5 else rng.integers(0, M, (J, M))
        inst = K.inst("tiny", machine, rng.integers(1, 10, (J, M)))
        env = BatchedJssEnv(inst, batch=1, _backend=be)
        env.reset()
        a, b = check_properties(be, env, rng, w, inst)
        solved, bounded = solved + a, bounded + b
    return solved, bounded


def case_properties(be, name):
    env = env_on(be, name)
    return check_properties(be, env, np.random.default_rng(3), name)


# ---- refusals and errors -----------------------------------------------------------------------------------------------------------
def case_refused_rows(be):
    """next to relaxations and builds: a parent out of range, the env never reset, a mask bit at M, a negative rank on a fixed
    machine -- -1, the other rows as they were; a negative rank on a free machine is not read; a cyclic rank is -2"""
    env = env_on(be, "3x2")
    st = case_state("3x2")
    host = st["host"]
    base = st["base"]
    neg = base.copy()
    neg[0, 0] = -3                                                     # (machine 0)
    cyc = np.array([[1, 0], [1, 1], [1, 0]], np.int32)                 # job 2 before job 0 on machine 0, its last stop, and behind it on machine 1
    par = np.array([0, 4, 3, 1, 0, 0, -1, 2], np.int32)                # (B = 4, env 3 never reset)
    masks = np.array([3, 0, 0, 4, 1, 2, 0, 3], np.uint64)
    ranks = np.stack([base, base, base, base, neg, neg, base, cyc])
    got = call_relax(be, env, ranks, masks, par)
    ref = search.machine_reference(host["env_const"], host["ops"].reshape(-1, 3, 2), ranks, masks, par, fill=FILL)
    same(got, ref, RELAX_OUT, "refused rows")
    assert got[1]["length"][[1, 2, 3, 4, 6]].tolist() == [-1] * 5 and got[1]["length"][0] >= 0 and got[1]["length"][5] >= 0
    assert got[1]["length"][7] == -2
    for k in RELAX_OUT[1:]:
        assert (got[1][k][[1, 2, 3, 4, 6, 7]] == FILL).all() and not (got[1][k][[0, 5]] == FILL).any(), k
    got = call_build(be, env, par, None, 1, ranks, masks)
    ref = search.bottleneck_reference(host["env_const"], host["ops"].reshape(-1, 3, 2), par, None, 1, ranks, masks, fill=FILL)
    same(got, ref, BUILD_OUT, "refused builds")
    assert got[1]["makespan"][[1, 2, 3, 4, 6]].tolist() == [-1] * 5 and got[1]["makespan"][7] == -2 and got[1]["makespan"][5] >= 0
    fresh = BatchedJssEnv("ta01", batch=2, _backend=be)
    for call in (fresh.relax_machines, fresh.bottleneck):
        try:
            call()
        except RuntimeError:
            pass
        else:
            raise AssertionError("before reset() the call must raise")


def case_abi_errors(be):
    """every code of both entry points, before anything runs: the outputs keep their fill"""
    env = env_on(be, "3x2")
    st = case_state("3x2")
    B, ranks, masks, par = env.batch, st["ranks"], st["masks"], st["par"]

    def desc_of(desc):
        if desc is None or desc == "null":
            return None if desc is None else C.POINTER(_abi.JssDesc)()
        d = _abi.JssDesc.from_buffer_copy(env._desc)
        for k, v in desc.items():
            setattr(d, k, v)
        return C.byref(d)

    def relax(desc=None, rank=ranks, fixed=masks, parents=par, **kw):
        got = call_relax(be, env, rank, fixed, parents, desc=desc_of(desc), **kw)
        if got[0] and kw.get("n", 1):
            assert all(x is None or (x == FILL).all() for x in got[1].values()), (desc, kw)
        return got[0]

    def build(desc=None, parents=par, bias=None, reopt=1, rank=None, fixed=None, **kw):
        got = call_build(be, env, parents, bias, reopt, rank, fixed, desc=desc_of(desc), **kw)
        if got[0] and kw.get("n", 1):
            assert all(x is None or (x == FILL).all() for x in got[1].values()), (desc, kw)
        return got[0]

    for call in (relax, build):
        assert call(desc="null") == _abi.E_NULL and call(null=("state",)) == _abi.E_NULL and call(null=("arg",)) == _abi.E_NULL
        assert call(desc={"ops": None}) == _abi.E_NULL
        assert call(n=-1) == _abi.E_SHAPE and call(parents=None, n=B + 1) == _abi.E_SHAPE and call(parents=None, n=B - 1) == _abi.E_SHAPE
        assert call(desc={"jmax": 0}) == _abi.E_SHAPE and call(desc={"mmax": 65}) == _abi.E_SHAPE and call(desc={"batch": -1}) == _abi.E_SHAPE
        assert call(desc={"kernel": 64}) == _abi.E_KIND
        assert call(n=0) == 0 and call() == 0
    assert relax(null=("length",)) == _abi.E_NULL and relax(null=("rank",)) == _abi.E_NULL and relax(alias=True) == _abi.E_NULL
    assert relax(stride=5) == _abi.E_SHAPE and relax(desc={"jmax": env.jmax + 1}) == _abi.E_SHAPE    # (the stride is that of another region)
    assert relax(rank=None, fixed=None) == 0 and relax(fixed=None) == 0 and relax(want=()) == 0
    assert build(null=("makespan",)) == _abi.E_NULL and build(null=("rank",)) == _abi.E_NULL
    assert build(rank=ranks) == _abi.E_NULL and build(fixed=masks) == _abi.E_NULL and build(rank=ranks, fixed=masks, alias=True) == _abi.E_NULL
    assert build(reopt=-1) == _abi.E_SHAPE and build(reopt=_abi.BOTTLENECK_MAX_REOPT + 1) == _abi.E_SHAPE
    assert build(reopt=0) == 0 and build(reopt=_abi.BOTTLENECK_MAX_REOPT) == 0 and build(want=()) == 0
    # a row of more than 2688 entries does not fit one candidate's 64 KB of LDS: both libraries say so; 128 x 21 fits (not run)
    shared = st["base"]
    assert relax(desc={"jmax": 128, "mmax": 22}, rank=shared) == _abi.E_LDS and build(desc={"jmax": 128, "mmax": 22}) == _abi.E_LDS
    assert relax(desc={"jmax": 128, "mmax": 21}, rank=shared, n=0) == 0 and build(desc={"jmax": 128, "mmax": 21}, n=0) == 0


# ---- the driver --------------------------------------------------------------------------------------------------------------------
def definition_loop(be, instances, walkers, reopt, spread, polish, tenure, seed, target):
    """search.bottleneck_search written with the public calls, on the host: returns (makespan, walker, rank, start, optimal,
    lower_bound, best_makespan)"""
    names = instances if isinstance(instances, list) else [instances]
    G, W = len(names), walkers
    n = lambda x: np.asarray(be.numpy(x)).copy()   # noqa: E731

    def batch(per_group):
        if G == 1:
            return BatchedJssEnv(names[0], batch=per_group, seed=seed, _backend=be)
        return BatchedJssEnv(names, batch=G * per_group, table_of_env=np.repeat(np.arange(G), per_group), order="interleaved", seed=seed,
                             _backend=be)

    env = batch(1)
    env.reset()
    bound = n(env.relax_machines()[0])
    tgt = bound if target == "one_machine" else n(env.lower_bound()) if target == "lower_bound" else None if target is None else \
        np.broadcast_to(np.asarray(target, np.int32), (G,))
    parents = np.repeat(np.arange(G), W).astype(np.int32)
    bias = np.random.default_rng(seed).integers(0, spread + 1, (G * W, env.mmax)).astype(np.int32)
    bias[::W] = 0
    mk, rank, info = (n(x) for x in env.bottleneck(parents, bias, reopt))
    if polish:
        crowd = batch(W)
        crowd.reset()
        mk, rank, _ = (n(x) for x in crowd.tabu_blocks(rank, polish, tenure))
    walker = np.array([min((int(mk[g * W + w]), w) for w in range(W) if mk[g * W + w] >= 0)[1] for g in range(G)], np.int32)
    winner = np.arange(G, dtype=np.int32) * W + walker
    again, start = (n(x) for x in env.evaluate_order(rank[winner], np.arange(G, dtype=np.int32), start=True))
    assert np.array_equal(again, mk[winner])
    optimal = np.zeros(G, bool) if tgt is None else mk[winner] <= tgt
    return mk[winner], walker, rank[winner], start, optimal, bound, mk


FIELDS = ("makespan", "walker", "rank", "start", "optimal", "lower_bound", "best_makespan")


def case_driver(be, instances, walkers=8, reopt=1, spread=40, polish=0, tenure=8, seed=0, target="one_machine"):
    want = definition_loop(be, instances, walkers, reopt, spread, polish, tenure, seed, target)
    res = search.bottleneck_search(instances, walkers, reopt, spread, polish, tenure, seed, target, _backend=be)
    for label, w in zip(FIELDS, want):
        assert np.array_equal(getattr(res, label), w), (label, getattr(res, label), w)
    assert (res.makespan >= res.lower_bound).all() and res.info.shape == (len(res.best_makespan), _abi.BOTTLENECK_NI)
    return res


# ---- the built library ------------------------------------------------------------------------------------------------------------
def machine_kernel_rows():
    """[(name, vgprs, sgprs, spilled vgprs, spilled sgprs, scratch bytes, static LDS bytes)] of libjss_machine_hip.so"""
    import re
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import LLVM, kernel_resources
    from jssenv_amd.build import build_machine_extension
    so = build_machine_extension()                                    # (built here if build() has not run)
    rows = kernel_resources(so)
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "machine.co")
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", so, fat], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    by_name = {}
    for k in notes.split("- .agpr_count")[1:]:
        by_name[re.search(r"\.name:\s+(\S+)", k).group(1)] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", k).group(1))
    assert len(by_name) == len(rows)
    lds = {next(r[0] for r in rows if r[0].split("(")[0] in name): size for name, size in by_name.items()}   # (mangled names hold the plain ones)
    return [r + (lds[r[0]],) for r in rows]
