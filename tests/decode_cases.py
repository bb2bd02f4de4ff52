"""Backend-agnostic cases of jss_decode_keys and jss_keys_evolve (include/jss_decode.h), BatchedJssEnv.decode_keys / evolve_keys and
search.brkga_search, run against the host-core twin, the kernel source (jssenv_amd/csrc/jss_decode.hip) under the SIMT emulator and
the HIP library libjss_decode_hip.so.

The references are search.decode_reference and search.evolve_reference (NumPy, written from the header's definition).  A case's
batch, key tables and candidate list are made once, on the twin, and its references once; another backend builds the same batch
(only env_const and the instance tables are read, which a reset writes identically everywhere) and is compared with them bit for
bit."""
import ctypes as C
import os
import subprocess

import numpy as np

import order_cases as K
from clone_cases import rows_of
from jssenv_amd import BatchedJssEnv, _abi, dispatching, search
from jssenv_amd import instances as I

ROOT = K.ROOT
DECODE_SRC = os.path.join(ROOT, "jssenv_amd", "csrc", "jss_decode.hip")
EMU_LIB = os.path.join(K.EMU, "libjss_decode_emu.so")
FILL = K.FILL                       # what the outputs hold before a call: the rows of refused candidates keep it
DELTAS = (0, 32768, 65536)
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1

# the hand case: 3 jobs x 3 machines; delta (in 1 / 65536) -> (start, makespan, info)
HAND_MACHINE = [[1, 0, 2], [2, 0, 1], [2, 1, 0]]
HAND_DURATION = [[5, 2, 3], [1, 3, 3], [3, 3, 1]]
HAND_KEYS = [[3, 8, 4], [5, 1, 3], [9, 5, 0]]
HAND_RESULTS = {65536: ([[6, 11, 13], [3, 4, 11], [0, 3, 7]], 16, (4, 2, 1, 0)),
                32768: ([[0, 5, 7], [3, 7, 10], [0, 5, 10]], 13, (2, 2, 1, 0)),
                0: ([[0, 7, 9], [3, 4, 8], [0, 5, 9]], 12, (1, 2, 0, 0))}
# a tiny instance with several durations of 0, among them a whole job and two operations in a row on one machine
ZEROS_MACHINE = [[0, 1, 2], [1, 0, 2], [2, 2, 0], [0, 2, 1]]
ZEROS_DURATION = [[0, 3, 0], [2, 0, 0], [0, 0, 0], [4, 0, 1]]
ZEROS_KEYS = [[1, 5, 2], [7, 7, 0], [3, 3, 9], [1, 2, 8]]

# instance, table of dispatching.rule_keys -> makespans at delta 1, 0.5, 0; the info rows of ta01 SPT
ANCHORS = {("ta01", "SPT"): (1966, 1605, 1462), ("ta01", "MWR"): (1589, 1521, 1491), ("ta11", "MWR"): (1796, 1654, 1685),
           ("ta41", "SPT"): (3561, 2938, 2499)}
ANCHOR_INFO = {("ta01", "SPT"): ((115, 4, 66, 0), (75, 5, 23, 0), (51, 4, 0, 0))}


def build_emu_decode():
    """jss_decode.hip, unmodified, compiled with g++ against the SIMT emulator's hip_runtime.h: a library of its own"""
    deps = [DECODE_SRC, os.path.join(K.EMU, "hip", "hip_runtime.h"), os.path.join(ROOT, "jssenv_amd", "csrc", "jss_abi_checks.hpp"),
            os.path.join(ROOT, "include", "jss_decode.h")]
    if not os.path.isfile(EMU_LIB) or any(os.path.getmtime(d) > os.path.getmtime(EMU_LIB) for d in deps):
        tmp = EMU_LIB + f".tmp{os.getpid()}"
        subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
                               "-Wno-unknown-pragmas", "-I" + K.EMU, "-I" + os.path.join(ROOT, "include"), DECODE_SRC, "-o", tmp])
        os.replace(tmp, EMU_LIB)
    return EMU_LIB


def emu_backend():
    """order_cases' emulator backend (the env kernels, jss_order.hip) with the emulated decode library as its `decode_lib`"""
    be = K.emu_backend()
    be.decode_lib = _abi.bind_decode(C.CDLL(build_emu_decode()))
    return be


twin_backend = K.twin_backend


# ---- the batches -----------------------------------------------------------------------------------------------------------------
def inst_with_zeros(name, machine, duration):
    """an Instance whose durations may be 0.  Instance refuses them because the step kernels need d >= 1; a decode reads the op
    table only and nothing steps these envs, so the zeros are written into the arrays behind a valid instance"""
    duration = np.asarray(duration, np.int32)
    inst = K.inst(name, machine, np.maximum(duration, 1))
    inst.duration[...] = duration
    return inst


def hand_instance():
    return K.inst("hand", HAND_MACHINE, HAND_DURATION)


def zeros_instance():
    return inst_with_zeros("zeros", ZEROS_MACHINE, ZEROS_DURATION)


def _taillard(jobs, machines, seed):
    return I.taillard_instance(jobs, machines, 3000 + seed, 4000 + seed, name=f"syn{jobs}x{machines}")


def _flat(jobs, machines, duration):
    """every duration the same, the machines of job j rotated by j"""
    machine = (np.arange(machines)[None, :] + np.arange(jobs)[:, None]) % machines
    return K.inst(f"flat{jobs}x{machines}", machine, np.full((jobs, machines), duration))


# name -> (constructor on a backend, envs).  The last env of every batch is never reset, except in "many".  "M1": the package
# builds no instance with one machine (the reference refuses it, and so do the desc checks), so the envs of a 5 x 2 batch get
# M = 1 written into their env_const after the reset -- the decoder reads J, M and the table from there, and nothing steps them.
OWN = {
    "hand": (lambda be: BatchedJssEnv(hand_instance(), batch=3, _backend=be, seed=31), 3),
    "zeros": (lambda be: BatchedJssEnv(zeros_instance(), batch=3, _backend=be, seed=32), 3),
    "ties": (lambda be: BatchedJssEnv(_flat(5, 4, 3), batch=3, _backend=be, seed=33), 3),
    "J1": (lambda be: BatchedJssEnv(K.inst("one4", [[2, 0, 3, 1]], [[4, 9, 2, 6]]), batch=3, _backend=be, seed=34), 3),
    "M1": (lambda be: BatchedJssEnv(K.inst("five2", [[0, 1]] * 5, [[3, 1], [5, 1], [2, 1], [7, 1], [4, 1]]), batch=3, _backend=be, seed=35), 3),
    "J64": (lambda be: BatchedJssEnv(_taillard(64, 3, 1), batch=3, _backend=be, seed=36), 3),
    "J128": (lambda be: BatchedJssEnv(_taillard(128, 2, 2), batch=3, _backend=be, seed=37), 3),
    "extreme": (lambda be: BatchedJssEnv(_taillard(6, 4, 3), batch=3, _backend=be, seed=38), 3),
    "many": (lambda be: BatchedJssEnv(_taillard(6, 4, 4), batch=1, _backend=be, seed=39), 1),
}
REUSED = ("1x2", "3x2", "repeats", "per-env", "ta01", "J65", "table-of-env")
CASES = dict({name: K.CASES[name] for name in REUSED}, **OWN)
POSITIVE = tuple(name for name in CASES if name != "zeros")            # the cases whose durations are all >= 1
_STATES = {}


def make_env(be, name):
    """the case's batch on `be`: every env but the last reset ("many": its one env)"""
    make, B = CASES[name]
    env = make(be)
    which = np.ones(B, np.uint8)
    if name != "many":
        which[B - 1] = 0
    env.reset(which=which)
    if name == "M1":
        env.env_const[:B - 1, _abi.C_MACHINES] = 1
        env.synchronize()
    return env


def case_state(name):
    """The case's batch on the twin and what is derived from it, made once: `shared`, one key table; `tables`, one per
    candidate; the candidate list -- every reset env three times, the env never reset, parents out of range -- with a delta of
    each kind per candidate, a -1 and a 65537 among them; and the references of every call of case_against_mirror."""
    if name in _STATES:
        return _STATES[name]
    B = CASES[name][1]
    env = make_env(twin_backend(), name)
    host = K.host_tables(env)
    jmax, mmax = env.jmax, env.mmax
    rng = np.random.default_rng(len(name) * 104729 + B)
    if name == "many":
        par = np.zeros(70, np.int32)
        delta_of = np.array([DELTAS[c % 3] for c in range(70)], np.int32)
        refused = np.zeros(70, bool)
    else:
        par = [i for i in range(B - 1) for _ in range(3)] + [B - 1, -1, B, 0, 0, I32_MAX, I32_MIN]
        if len(par) % 4 == 0:
            par.append(0)
        par = np.asarray(par, np.int64).astype(np.int32)
        delta_of = np.array([DELTAS[(c + c // 3) % 3] for c in range(par.size)], np.int32)
        bad_delta = 3 * (B - 1) + 3
        delta_of[bad_delta], delta_of[bad_delta + 1] = -1, 65537
        refused = (par < 0) | (par >= B - 1)
        refused[bad_delta] = refused[bad_delta + 1] = True
    n = par.size

    def draw(shape):
        if name == "ties":
            return np.full(shape, 7, np.int32)
        if name == "extreme":
            return rng.choice(np.array([I32_MIN, I32_MAX, -1, I32_MIN + 1, 0], np.int64), shape).astype(np.int32)
        if name == "hand":
            return np.broadcast_to(np.asarray(HAND_KEYS, np.int32), shape).copy()
        if name == "zeros" and len(shape) == 2:
            return np.asarray(ZEROS_KEYS, np.int32)
        return rng.integers(-50, 50, shape).astype(np.int32) if rng.random() < 0.5 else rng.integers(I32_MIN, I32_MAX, shape, dtype=np.int64).astype(np.int32)

    shared, tables = draw((jmax, mmax)), draw((n, jmax, mmax))
    ref = lambda keys, parents, delta: search.decode_reference(host["env_const"], host["ops"], keys, parents, delta, fill=FILL)   # noqa: E731
    st = dict(env=env, host=host, B=B, par=par, delta_of=delta_of, refused=refused, shared=shared, tables=tables,
              rows={d: ref(shared, None, d) for d in DELTAS} if name != "many" else {},
              cands={d: ref(tables, par, d) for d in DELTAS}, mixed=ref(tables, par, delta_of),
              shared_cands=ref(shared, par, delta_of))
    _STATES[name] = st
    return st


def env_on(be, name):
    return case_state(name)["env"] if be is twin_backend() else make_env(be, name)


def call_decode(be, env, keys, parents=None, delta=65536, delta_of=None, want=("start", "info"), n=None, desc=None, null=()):
    """jss_decode_keys through the backend's library: (rc, makespan, start, info) as host arrays (None where not asked for); the
    outputs are prefilled (FILL), so what a call leaves alone can be told from what it writes"""
    lib = search.decode_library(be)
    keys = np.asarray(keys, np.int32)
    n = (env.batch if parents is None else len(parents)) if n is None else n
    rows = max(n, 1)
    with be.on_device():
        dev = lambda x: None if x is None else be.from_numpy(np.asarray(x, np.int32))   # noqa: E731
        full = lambda shape: be.from_numpy(np.full(shape, FILL, np.int32))   # noqa: E731
        k, par, dl = dev(keys), dev(parents), dev(delta_of)
        mk = full(rows)
        st = full((rows, env.jmax, env.mmax)) if "start" in want else None
        nf = full((rows, _abi.DECODE_NI)) if "info" in want else None
        p = be.ptr
        arg = _abi.JssDecode(n, env.jmax * env.mmax if keys.ndim == 3 else 0, int(delta), p(par), None if "keys" in null else p(k), p(dl),
                             None if "makespan" in null else p(mk), p(st), p(nf))
        rc = lib.jss_decode_keys(C.byref(env._desc) if desc is None else desc, None if "state" in null else C.byref(env._state),
                                 None if "arg" in null else C.byref(arg), be.stream())
        be.sync()
    host = lambda x: None if x is None else np.asarray(be.numpy(x))   # noqa: E731
    return rc, host(mk), host(st), host(nf)


def same(got, ref, what):
    assert got[0] == 0, (what, got[0])
    n = ref[0].size
    assert got[1].dtype == np.int32 and np.array_equal(got[1][:n], ref[0]), (what, "makespan", got[1][:n], ref[0])
    for k, label in ((2, "start"), (3, "info")):
        if got[k] is not None:
            assert np.array_equal(got[k][:n], ref[k - 1]), (what, label)


def case_against_mirror(be, name, light=False):
    """the shared table on the rows and per-candidate tables on the candidate list at every delta, a per-candidate delta_of that
    mixes them (with a -1 and a 65537), the shared table on the candidate list, every combination of the optional outputs, n == 0;
    refused rows keep their fill; the batch and the key tables untouched.  `light` (the emulator, which takes seconds per call at
    15 x 15): the calls with a delta_of and the rows at delta 1 only"""
    st = case_state(name)
    env = env_on(be, name)
    before = rows_of(env)
    par, tables, shared = st["par"], st["tables"], st["shared"]
    for d in (DELTAS[2:] if light else DELTAS):
        if st["rows"]:
            same(call_decode(be, env, shared, None, d), st["rows"][d], (name, "rows", d))
        if not light:
            same(call_decode(be, env, tables, par, d), st["cands"][d], (name, "candidates", d))
    same(call_decode(be, env, tables, par, 65536, st["delta_of"]), st["mixed"], (name, "delta_of"))
    same(call_decode(be, env, shared, par, 0, st["delta_of"]), st["shared_cands"], (name, "shared, delta_of"))
    mk, start, info = st["mixed"]
    dead = mk < 0
    assert np.array_equal(dead, st["refused"]) and (mk[dead] == -1).all() and (mk[~dead] >= 0).all() and not dead[0]
    assert (start[dead] == FILL).all() and (info[dead] == FILL).all()
    assert not (start[~dead] == FILL).any() and not (info[~dead] == FILL).any()
    for mask in (() if light else range(4)):
        want = tuple(w for bit, w in enumerate(("start", "info")) if mask >> bit & 1)
        same(call_decode(be, env, tables, par, 65536, st["delta_of"], want=want), st["mixed"], (name, want))
    got = call_decode(be, env, tables, par, 65536, n=0)
    assert got[0] == 0 and all((x == FILL).all() for x in got[1:])
    after = rows_of(env)
    for k in before:
        assert np.array_equal(before[k], after[k]), (name, k)


def case_hand(be, mirror=False):
    """the hand case: the listed starts, makespans and info rows at the three deltas, through the public call"""
    env = env_on(be, "hand")
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    for d, (start, makespan, info) in HAND_RESULTS.items():
        mk, st, nf = (n(x) for x in env.decode_keys(np.asarray(HAND_KEYS, np.int32), None, d / 65536, start=True, info=True))
        assert mk.tolist() == [makespan, makespan, -1] and st[0].tolist() == start and nf[0].tolist() == list(info), (d, mk, st[0], nf[0])
        if mirror:
            host = K.host_tables(env)
            ref = search.decode_reference(host["env_const"], host["ops"], HAND_KEYS, None, d)
            assert ref[0][0] == makespan and ref[1][0].tolist() == start and ref[2][0].tolist() == list(info)


def case_anchor(be, key, mirror=False):
    """B = 3, the table of a stock rule at delta 1, 0.5, 0: the listed makespans (and info rows)"""
    env = BatchedJssEnv(key[0], batch=3, _backend=be)
    env.reset()
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    table = dispatching.rule_keys(*key)
    mk, start, info = (n(x) for x in env.decode_keys(table, None, np.array([1.0, 0.5, 0.0]), start=True, info=True))
    assert tuple(mk.tolist()) == ANCHORS[key], (key, mk)
    if key in ANCHOR_INFO:
        assert tuple(tuple(r) for r in info.tolist()) == ANCHOR_INFO[key], (key, info)
    assert np.array_equal(n(env.evaluate_order(start)), mk)
    if mirror:
        host = K.host_tables(env)
        ref = search.decode_reference(host["env_const"], host["ops"], table, None, [65536, 32768, 0])
        for got, want in zip((mk, start, info), ref):
            assert np.array_equal(got, want)


# ---- properties ------------------------------------------------------------------------------------------------------------------
def _on_machines(start, mach, dur):
    """machine -> its operations as (start, end, j, k), by start (then end: an operation of duration 0 first)"""
    J, M = mach.shape
    out = {}
    for j in range(J):
        for k in range(M):
            out.setdefault(int(mach[j, k]), []).append((int(start[j, k]), int(start[j, k] + dur[j, k]), j, k))
    return {m: sorted(v) for m, v in out.items()}


def feasible(start, mach, dur):
    """job order holds and no two operations overlap on a machine; returns the makespan"""
    J, M = mach.shape
    s = start[:J, :M].astype(np.int64)
    assert (s >= 0).all() and (s[:, 1:] >= (s + dur)[:, :-1]).all()
    for ops in _on_machines(s, mach, dur).values():
        assert all(b[0] >= a[1] for a, b in zip(ops[:-1], ops[1:]))
    return int((s + dur).max())


def no_delay(start, mach, dur):
    """brute force: no machine stands idle at a time at which an operation on it could start -- from its job predecessor's end
    to its own start the machine is busy without a gap (durations >= 1)"""
    J, M = mach.shape
    on = _on_machines(start, mach, dur)
    for j in range(J):
        for k in range(M):
            t, s = (int(start[j, k - 1] + dur[j, k - 1]) if k else 0), int(start[j, k])
            for a, b, _, _ in on[int(mach[j, k])]:
                if a <= t < b:
                    t = b
            if t < s:
                return False
    return True


def active(start, mach, dur):
    """brute force: no operation fits into an earlier idle gap of its machine at or after its job predecessor's end"""
    J, M = mach.shape
    on = _on_machines(start, mach, dur)
    for j in range(J):
        for k in range(M):
            ready, s, d = (int(start[j, k - 1] + dur[j, k - 1]) if k else 0), int(start[j, k]), int(dur[j, k])
            others = [(a, b) for a, b, jj, kk in on[int(mach[j, k])] if (jj, kk) != (j, k)]
            for t in range(ready, s):
                if all(t + d <= a or t >= b for a, b in others):
                    return False
    return True


def check_properties(be, env, keys, what):
    """one table per env (n == B): see the asserts.  Returns the delta = 1 info rows of the reset envs"""
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    host = K.host_tables(env)
    const = host["env_const"]
    out = {d: [n(x) for x in env.decode_keys(keys, None, d, start=True, info=True)] for d in (0.0, 0.5, 1.0)}
    alive = out[1.0][0] >= 0
    assert alive[0]
    for d, (mk, start, info) in out.items():
        # a valid rank: evaluate_order gives the same makespan and the same start times back (a semi-active schedule)
        again, begin = (n(x) for x in env.evaluate_order(start, start=True))
        assert np.array_equal(again[alive], mk[alive]) and np.array_equal(begin[alive], start[alive]), (what, d)
        for i in np.flatnonzero(alive):
            J, M, tab = (int(const[i, x]) for x in (_abi.C_JOBS, _abi.C_MACHINES, _abi.C_TABLE))
            ops = host["ops"].reshape(-1, env.jmax, env.mmax)[tab, :J, :M]
            mach, dur = (ops >> 16) & 63, ops & 0xFFFF
            assert feasible(start[i], mach, dur) == mk[i], (what, d, i)
            assert (start[i, J:] == -1).all() and (start[i, :, M:] == -1).all()
            assert info[i, 1] >= 1 and info[i, 0] <= J * M and info[i, 3] == 0
            if d == 0.0:
                assert info[i, 2] == 0 and no_delay(start[i], mach, dur), (what, i)
            if d == 1.0:
                assert active(start[i], mach, dur), (what, i)
    # the round trip: the start times of a delta = 1 decode, negated, are a key table that decodes to the same schedule
    mk, start, _ = out[1.0]
    back = [n(x) for x in env.decode_keys(dispatching.keys_from_schedule(start), None, 1.0, start=True)]
    assert np.array_equal(back[0][alive], mk[alive]) and np.array_equal(back[1][alive], start[alive]), what
    return out[1.0][2][alive]


def case_properties(be, name):
    st = case_state(name)
    env = env_on(be, name)
    keys = st["tables"][:st["B"]] if name != "many" else st["tables"][:1]
    return check_properties(be, env, keys, name)


def case_seeded_properties(be, count, seed=7):
    """`count` seeded tiny instances (2-5 jobs, 2-4 machines, durations 1-8, random keys), three envs each with a table of its
    own: returns the summed delta = 1 info rows"""
    rng = np.random.default_rng(seed)
    total = np.zeros(_abi.DECODE_NI, np.int64)
    for w in range(count):
        J, M = int(rng.integers(2, 6)), int(rng.integers(2, 5))
        machine = np.stack([rng.permutation(M) for _ in range(J)]) if rng.random() < 0.7 else rng.integers(0, M, (J, M))
        inst = K.inst("tiny", machine, rng.integers(1, 9, (J, M)))
        env = BatchedJssEnv(inst, batch=3, _backend=be)
        env.reset()
        keys = rng.integers(-4, 5, (3, J, M)).astype(np.int32) if w % 2 else rng.integers(I32_MIN, I32_MAX, (3, J, M), dtype=np.int64).astype(np.int32)
        total += check_properties(be, env, keys, w).sum(axis=0)
    return total


# ---- refusals and errors -----------------------------------------------------------------------------------------------------------
def case_refused_rows(be):
    """next to decodes: a parent out of range, the env never reset, a delta_of of -1 and one of 65537 -- makespan -1, the rows
    of start and info as they were"""
    env = env_on(be, "3x2")
    st = case_state("3x2")
    par = np.array([0, 4, 3, 1, 2, -1, 0], np.int32)                  # (B = 4, env 3 never reset)
    delta_of = np.array([65536, 0, 0, -1, 65537, 0, 0], np.int32)
    got = call_decode(be, env, st["tables"][:7], par, 65536, delta_of)
    ref = search.decode_reference(st["host"]["env_const"], st["host"]["ops"], st["tables"][:7], par, delta_of, fill=FILL)
    same(got, ref, "refused rows")
    assert got[1].tolist()[1:6] == [-1] * 5 and got[1][0] >= 0 and got[1][6] >= 0
    assert (got[2][1:6] == FILL).all() and (got[3][1:6] == FILL).all() and not (got[2][[0, 6]] == FILL).any()
    fresh = BatchedJssEnv("ta01", batch=2, _backend=be)
    try:
        fresh.decode_keys(np.zeros((15, 15), np.int32))
    except RuntimeError:
        pass
    else:
        raise AssertionError("decode_keys before reset() must raise")


def case_abi_errors(be):
    """every code of jss_decode_keys, before anything runs: the outputs keep their fill"""
    env = env_on(be, "3x2")
    st = case_state("3x2")
    B, tables, par = env.batch, st["tables"], st["par"]

    def call(desc=None, keys=tables, parents=par, delta=65536, **kw):
        d = _abi.JssDesc.from_buffer_copy(env._desc)
        for k, v in (desc or {}).items():
            setattr(d, k, v)
        got = call_decode(be, env, keys, parents, delta, desc=None if desc == "null" else C.byref(d), **kw)
        if got[0] and kw.get("n", 1):
            assert all(x is None or (x == FILL).all() for x in got[1:]), (desc, kw)
        return got[0]

    assert call_decode(be, env, tables, par, desc=C.POINTER(_abi.JssDesc)())[0] == _abi.E_NULL
    assert call(null=("state",)) == _abi.E_NULL and call(null=("arg",)) == _abi.E_NULL
    assert call(null=("keys",)) == _abi.E_NULL and call(null=("makespan",)) == _abi.E_NULL
    assert call(desc={"ops": None}) == _abi.E_NULL
    assert call(n=-1) == _abi.E_SHAPE and call(delta=-1) == _abi.E_SHAPE and call(delta=65537) == _abi.E_SHAPE
    assert call(parents=None, n=B + 1) == _abi.E_SHAPE and call(parents=None, n=B - 1) == _abi.E_SHAPE
    assert call(desc={"jmax": 0}) == _abi.E_SHAPE and call(desc={"mmax": 65}) == _abi.E_SHAPE and call(desc={"batch": -1}) == _abi.E_SHAPE
    assert call(desc={"jmax": env.jmax + 1}) == _abi.E_SHAPE            # (the stride is that of another region)
    assert call(desc={"kernel": 64}) == _abi.E_KIND
    # a row of more than 8160 entries does not fit one candidate's 64 KB of LDS: both libraries say so; 128 x 63 fits (not run)
    assert call(desc={"jmax": 128, "mmax": 64}, keys=st["shared"]) == _abi.E_LDS
    assert call(desc={"jmax": 128, "mmax": 63}, keys=st["shared"], n=0) == 0 and call(n=0) == 0
    # a stride that is neither 0 nor the region
    lib = search.decode_library(be)
    with be.on_device():
        k, mk = be.from_numpy(tables), be.from_numpy(np.full(B, FILL, np.int32))
        arg = _abi.JssDecode(B, 5, 65536, None, be.ptr(k), None, be.ptr(mk), None, None)
        assert lib.jss_decode_keys(C.byref(env._desc), C.byref(env._state), C.byref(arg), be.stream()) == _abi.E_SHAPE
        be.sync()
        assert (np.asarray(be.numpy(mk)) == FILL).all()
    assert call() == 0 and call(want=()) == 0                          # the optional pointers may be NULL


# ---- evolve --------------------------------------------------------------------------------------------------------------------------
# (G, P, region, elite, mutants, rho)
EVOLVE_SHAPES = [(3, 8, 12, 2, 2, 0.7), (1, 2, 1, 1, 0, 0.7), (2, 65, 225, 10, 10, 0.0), (2, 65, 225, 10, 10, 1.0), (2, 4096, 4, 1, 1, 0.7)]
_EVOLVE = {}


def evolve_inputs(shape):
    """keys and a fitness vector with ties and negative entries, and the mirror's answer, made once"""
    if shape not in _EVOLVE:
        G, P, region, ne, nm, rho = shape
        rng = np.random.default_rng(G * 1000 + P + region)
        keys = rng.integers(I32_MIN, I32_MAX, (G * P, region), dtype=np.int64).astype(np.int32)
        fitness = rng.integers(0, max(2, P // 2), G * P).astype(np.int32)       # (ties)
        fitness[rng.random(G * P) < 0.2] = -1
        fitness[rng.random(G * P) < 0.05] = -7
        seed, generation = 0x1234567887654321 + P, 3 + region
        ref = search.evolve_reference(keys, fitness, G, P, ne, nm, int(round(rho * 65536)), generation, seed)
        _EVOLVE[shape] = dict(keys=keys, fitness=fitness, seed=seed, generation=generation, ref=ref)
    return _EVOLVE[shape]


def call_evolve(be, G, P, region, ne, nm, rho_q16, generation, seed, fitness, keys, want_rank=True, alias=False, null=()):
    """jss_keys_evolve through the backend's library: (rc, keys_out, by_rank); the outputs are prefilled (FILL)"""
    lib = search.decode_library(be)
    rows = max(G * P, 1)
    with be.on_device():
        dev = lambda x: None if x is None else be.from_numpy(np.asarray(x, np.int32))   # noqa: E731
        fit, k = dev(fitness), dev(keys)
        out = be.from_numpy(np.full((rows, max(region, 1)), FILL, np.int32))
        by_rank = be.from_numpy(np.full(rows, FILL, np.int32)) if want_rank else None
        p = be.ptr
        arg = _abi.JssEvolve(G, P, region, ne, nm, rho_q16, generation, seed & (2 ** 64 - 1), p(fit), p(k),
                             None if "keys_out" in null else p(k) if alias else p(out), p(by_rank))
        rc = lib.jss_keys_evolve(None if "arg" in null else C.byref(arg), be.stream())
        be.sync()
    return rc, np.asarray(be.numpy(out)), None if by_rank is None else np.asarray(be.numpy(by_rank))


def case_evolve(be, shape):
    """against the mirror bit for bit, by_rank with keys_out; the elites are exact copies; without a by_rank the same keys"""
    G, P, region, ne, nm, rho = shape
    x = evolve_inputs(shape)
    q16 = int(round(rho * 65536))
    rc, out, by_rank = call_evolve(be, G, P, region, ne, nm, q16, x["generation"], x["seed"], x["fitness"], x["keys"])
    assert rc == 0 and np.array_equal(by_rank, x["ref"][1]) and np.array_equal(out, x["ref"][0]), shape
    fit = x["fitness"].reshape(G, P)
    for g in range(G):
        order = by_rank[g * P:(g + 1) * P]
        assert sorted(order.tolist()) == list(range(P))
        ranked = [(fit[g, p] < 0, fit[g, p], p) for p in order]
        assert ranked == sorted(ranked)
        for c in range(ne):
            assert np.array_equal(out[g * P + c], x["keys"][g * P + order[c]])
    rc, again, none = call_evolve(be, G, P, region, ne, nm, q16, x["generation"], x["seed"], x["fitness"], x["keys"], want_rank=False)
    assert rc == 0 and none is None and np.array_equal(again, out)
    return out, by_rank


def case_evolve_fresh(be):
    """the all-mutant form with NULL fitness and keys_in: the mirror's rows; another generation or seed, other mutants"""
    G, P, region = 2, 5, 9
    ref = search.evolve_reference(None, None, G, P, 0, P, 0, 0, 11, region=region)
    rc, out, by_rank = call_evolve(be, G, P, region, 0, P, 45875, 0, 11, None, None)
    assert rc == 0 and np.array_equal(out, ref[0]) and np.array_equal(by_rank, ref[1]) and by_rank.tolist() == list(range(P)) * G
    assert len({tuple(r) for r in out.tolist()}) == G * P               # every row its own
    rc, other_gen, _ = call_evolve(be, G, P, region, 0, P, 45875, 1, 11, None, None, want_rank=False)
    rc2, other_seed, _ = call_evolve(be, G, P, region, 0, P, 45875, 0, 12, None, None)
    assert rc == 0 and rc2 == 0 and not (other_gen == out).all(axis=1).any() and not (other_seed == out).all(axis=1).any()
    # the mutants of a generation with elites and children: another generation, other mutants
    x = evolve_inputs(EVOLVE_SHAPES[0])
    a = call_evolve(be, 3, 8, 12, 2, 2, 45875, 1, 5, x["fitness"], x["keys"])[1]
    b = call_evolve(be, 3, 8, 12, 2, 2, 45875, 2, 5, x["fitness"], x["keys"])[1]
    rows = [g * 8 + c for g in range(3) for c in (6, 7)]
    assert not (a[rows] == b[rows]).all(axis=1).any() and np.array_equal(a[[0, 1, 8, 9]], b[[0, 1, 8, 9]])


def case_evolve_errors(be):
    """every code of jss_keys_evolve, before anything runs: the outputs keep their fill"""
    x = evolve_inputs(EVOLVE_SHAPES[0])

    def call(G=3, P=8, region=12, ne=2, nm=2, rho=45875, fitness=x["fitness"], keys=x["keys"], **kw):
        rc, out, by_rank = call_evolve(be, G, P, region, ne, nm, rho, 1, 5, fitness, keys, **kw)
        if rc:
            assert (out == FILL).all() and (by_rank == FILL).all()
        return rc

    assert call(null=("arg",)) == _abi.E_NULL and call(null=("keys_out",)) == _abi.E_NULL
    assert call(fitness=None) == _abi.E_NULL and call(keys=None) == _abi.E_NULL and call(alias=True) == _abi.E_NULL
    assert call(P=0) == _abi.E_SHAPE and call(P=4097) == _abi.E_SHAPE and call(region=0) == _abi.E_SHAPE and call(G=-1) == _abi.E_SHAPE
    assert call(rho=-1) == _abi.E_SHAPE and call(rho=65537) == _abi.E_SHAPE
    assert call(ne=7, nm=2) == _abi.E_SHAPE and call(ne=0, nm=7) == _abi.E_SHAPE and call(ne=-1, nm=9) == _abi.E_SHAPE
    assert call(G=0) == 0 and call() == 0 and call(ne=8, nm=0) == 0 and call(rho=0) == 0 and call(rho=65536) == 0


# ---- the driver --------------------------------------------------------------------------------------------------------------------
def definition_loop(be, instances, population, generations, elite, mutants, rho, delta, seed_rules, polish, tenure, seed, target,
                    check_every):
    """search.brkga_search written with the public calls, on the host: returns (makespan, keys, start, rank, history,
    generations, optimal)"""
    names = instances if isinstance(instances, list) else [instances]
    G, P = len(names), population
    n = lambda x: np.asarray(be.numpy(x)).copy()   # noqa: E731

    def batch(per_group):
        if G == 1:
            return BatchedJssEnv(names[0], batch=per_group, seed=seed, _backend=be)
        return BatchedJssEnv(names, batch=G * per_group, table_of_env=np.repeat(np.arange(G), per_group), order="interleaved", seed=seed,
                             _backend=be)

    env = batch(1)
    env.reset()
    tgt = n(env.lower_bound()) if target == "lower_bound" else None if target is None else np.broadcast_to(np.asarray(target, np.int32), (G,))
    parents = np.repeat(np.arange(G), P).astype(np.int32)
    n_elite, n_mutant = max(1, int(round(elite * P))), int(round(mutants * P))
    keys = n(env.evolve_keys((G * P, env.jmax, env.mmax), None, P, 0, P, generation=0, seed=seed)[0])
    for g, name in enumerate(names):
        for r, rule in enumerate(seed_rules):
            table = dispatching.rule_keys(name, rule)
            keys[g * P + r] = 0
            keys[g * P + r, :table.shape[0], :table.shape[1]] = table

    def low(mk):
        return [min([int(x) for x in mk[g * P:(g + 1) * P] if x >= 0] or [2 ** 31 - 1]) for g in range(G)]

    history, t = [], 0
    while True:
        fitness = n(env.decode_keys(keys, parents, delta))
        history.append(low(fitness))
        if t == generations:
            break
        if tgt is not None and t and t % check_every == 0 and all(h <= x for h, x in zip(history[-1], tgt)):
            break
        t += 1
        keys = n(env.evolve_keys(keys, fitness, P, n_elite, n_mutant, rho, t, seed)[0])
    mk, start = (n(x) for x in env.decode_keys(keys, parents, delta, start=True))
    rank = start
    if polish:
        walkers = batch(P)
        walkers.reset()
        mk, rank, _ = (n(x) for x in walkers.tabu_blocks(start, polish, tenure))
    winner = np.array([min((int(mk[g * P + p]), g * P + p) for p in range(P) if mk[g * P + p] >= 0)[1] for g in range(G)], np.int32)
    if polish:
        again, begin = (n(x) for x in walkers.evaluate_order(rank, winner, start=True))
        assert np.array_equal(again, mk[winner])
        start_out = begin
    else:
        start_out = start[winner]
    optimal = np.zeros(G, bool) if tgt is None else mk[winner] <= tgt
    return mk[winner], keys[winner], start_out, rank[winner], np.array(history).T.reshape(G, -1), t, optimal


FIELDS = ("makespan", "keys", "start", "rank", "history", "generations", "optimal")


def case_driver(be, instances, population=16, generations=6, elite=0.15, mutants=0.15, rho=0.7, delta=0.5, seed_rules=("SPT", "MWR"),
                polish=0, tenure=8, seed=0, target="lower_bound", check_every=8):
    want = definition_loop(be, instances, population, generations, elite, mutants, rho, delta, seed_rules, polish, tenure, seed, target,
                           check_every)
    res = search.brkga_search(instances, population, generations, elite, mutants, rho, delta, seed_rules, polish, tenure, seed, target,
                              check_every, _backend=be)
    for label, w in zip(FIELDS, want):
        assert np.array_equal(getattr(res, label), w), (label, getattr(res, label), w)
    G = len(res.makespan)
    assert res.history.shape == (G, res.generations + 1) and res.history.dtype == np.int32
    assert (np.diff(res.history, axis=1) <= 0).all()                   # elites are copied: it never rises
    if not polish:
        assert np.array_equal(res.history[:, -1], res.makespan) and np.array_equal(res.rank, res.start)
    assert (res.makespan <= res.history[:, -1]).all()
    return res


# ---- the built library ------------------------------------------------------------------------------------------------------------
def decode_kernel_rows():
    """[(name, vgprs, sgprs, spilled vgprs, spilled sgprs, scratch bytes, static LDS bytes)] of libjss_decode_hip.so"""
    import re
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import LLVM, kernel_resources
    from jssenv_amd.build import build_decode_extension
    so = build_decode_extension()                                     # (built here if build() has not run)
    rows = kernel_resources(so)
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "decode.co")
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
