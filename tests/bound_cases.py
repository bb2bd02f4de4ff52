"""Backend-agnostic cases of jss_bound (include/jss_bound.h) and BatchedJssEnv.lower_bound, run against the host-core twin, the
kernel source (jssenv_amd/csrc/jss_bound.hip) under the SIMT emulator and the HIP library libjss_bound_hip.so.

The reference is search.lower_bound_reference (NumPy, written from the header's definition).  A case's states are made once, on
the twin (random rollouts of several lengths, one env done, one never reset), its reference once from the twin's host arrays;
another backend gets the states through load_state_dict and is compared with that reference bit for bit."""
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
BOUND_SRC = os.path.join(ROOT, "jssenv_amd", "csrc", "jss_bound.hip")
EMU_LIB = os.path.join(EMU, "libjss_bound_emu.so")
FILL = -77777                       # what est_start holds before a call: rows of refused candidates keep it
SIX = ["ta01", "ta02", "ta11", "ta41", "ta61", "ta71"]
ANCHORS = {"ta01": (1005, 963, 1462), "ta02": (953, 942, 1446), "ta11": (1254, 949, 1865), "ta41": (1850, 1232, 2499),
           "ta61": (2868, 1284, 3606), "ta71": (5464, 1341, 6232)}     # lower_bound, job_bound at reset; SPT makespan


def build_emu_bound():
    """jss_bound.hip, unmodified, compiled with g++ against the SIMT emulator's hip_runtime.h: a library of its own"""
    deps = [BOUND_SRC, os.path.join(EMU, "hip", "hip_runtime.h"), os.path.join(ROOT, "include", "jss_bound.h"),
            os.path.join(ROOT, "jssenv_amd", "csrc", "jss_abi_checks.hpp")]
    if not os.path.isfile(EMU_LIB) or any(os.path.getmtime(d) > os.path.getmtime(EMU_LIB) for d in deps):
        tmp = EMU_LIB + f".tmp{os.getpid()}"
        subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
                               "-Wno-unknown-pragmas", "-I" + EMU, "-I" + os.path.join(ROOT, "include"), BOUND_SRC, "-o", tmp])
        os.replace(tmp, EMU_LIB)
    return EMU_LIB


def emu_backend():
    """the emulator backend of the env kernels, with the emulated bound library attached as its `bound_lib`"""
    sys.path.insert(0, EMU)
    from emu_backend import EmuBackend
    be = EmuBackend(default_kernel="auto")
    be.bound_lib = _abi.bind_bound(C.CDLL(build_emu_bound()))
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


def hand_instance():
    """J0: (m0, 3), (m1, 2); J1: (m1, 4), (m0, 1)"""
    return inst("hand2x2", [[0, 1], [1, 0]], [[3, 2], [4, 1]])


def _wide(jobs, machines, seed):
    return I.taillard_instance(jobs, machines, 1000 + seed, 2000 + seed, name=f"syn{jobs}x{machines}")


# name -> (constructor on a backend, envs).  The shapes are the smallest at which the kernel takes another path: one job, an
# odd 3 x 3, 15 x 15 on the shared compact table, 64 / 65 / 128 jobs (one or two jobs per lane; 65 jobs in rows padded to 128),
# 64 machines (eight full chunks of a row), ragged batches in both deals, per-env tables in every record layout, a generated
# batch, machines that repeat within a job with one the instance never uses, the longest durations.
CASES = {
    "1x2": (lambda be: BatchedJssEnv(inst("one", [[1, 0]], [[4, 9]]), batch=3, _backend=be, seed=1), 3),
    "3x3": (lambda be: BatchedJssEnv(_wide(3, 3, 1), batch=5, _backend=be, seed=2), 5),
    "ta01": (lambda be: BatchedJssEnv("ta01", batch=6, _backend=be, seed=3), 6),
    "J64": (lambda be: BatchedJssEnv(_wide(64, 5, 2), batch=4, _backend=be, seed=4), 4),
    "J65": (lambda be: BatchedJssEnv(_wide(65, 4, 3), batch=4, _backend=be, seed=5), 4),
    "J128": (lambda be: BatchedJssEnv(_wide(128, 3, 4), batch=4, _backend=be, seed=6), 4),
    "J65-in-128": (lambda be: BatchedJssEnv([_wide(65, 4, 3), _wide(128, 3, 4)], batch=5, table_of_env=[0, 1, 0, 0, 1],
                                            _backend=be, seed=7), 5),
    "M64": (lambda be: BatchedJssEnv(_wide(4, 64, 5), batch=4, _backend=be, seed=8), 4),
    "ragged-by-shape": (lambda be: BatchedJssEnv(["ta01", "ta41", "ta72"], batch=6, order="by_shape", _backend=be, seed=9), 6),
    "ragged-interleaved": (lambda be: BatchedJssEnv(["ta01", "ta41", "ta72"], batch=6, order="interleaved", _backend=be, seed=9), 6),
    "per-env": (lambda be: BatchedJssEnv(I.synthetic_packed(5, 7, 6), batch=5, _backend=be, seed=10), 5),
    "per-env-medium": (lambda be: BatchedJssEnv(I.synthetic_packed(5, 20, 10), batch=5, records="medium", _backend=be, seed=11), 5),
    "per-env-full": (lambda be: BatchedJssEnv(I.synthetic_packed(5, 20, 10), batch=5, records="full", _backend=be, seed=11), 5),
    "generated": (lambda be: BatchedJssEnv.generated(9, 5, 5, fresh=True, _backend=be, seed=12, instance_seed=9), 5),
    "repeats": (lambda be: BatchedJssEnv(inst("repeats", [[0, 0, 1, 3], [1, 0, 0, 1], [3, 1, 1, 0]],
                                              [[3, 5, 2, 4], [6, 1, 1, 7], [2, 2, 9, 3]]), batch=5, _backend=be, seed=13), 5),
    "dur65535": (lambda be: BatchedJssEnv(inst("long", [[0, 1], [1, 0], [0, 1]], [[65535, 65535], [65535, 1], [1, 65535]]),
                                          batch=4, _backend=be, seed=14), 4),
}
_STATES = {}


def host_arrays(env):
    be = env.backend
    pk = env.packed
    return dict(env_header=be.numpy(env.env_header), env_const=be.numpy(env.env_const), solution=be.numpy(env.solution),
                ops=np.array(pk.ops, copy=True), rem=np.array(pk.rem, copy=True), mask=be.numpy(env.action_mask),
                done=be.numpy(env.done), makespan=be.numpy(env.makespan))


def reference(host, parents=None, actions=None, use_mask=False, est_fill=FILL):
    return search.lower_bound_reference(host["env_header"], host["env_const"], host["solution"], host["ops"], host["rem"], parents,
                                        actions, host["mask"] if use_mask else None, est_fill)


def case_state(name):
    """The case's batch on the twin and what is derived from it, made once: env B - 1 is never reset, env B - 2 is done, the
    others have taken 0, 5, J * M / 2 random steps (NOPEs included) in turn; the candidate list; the reference's answers."""
    if name in _STATES:
        return _STATES[name]
    make, B = CASES[name]
    be = twin_backend()
    env = make(be)
    which = np.ones(B, np.uint8)
    which[B - 1] = 0
    env.reset(which=which)
    ops = int(env.jmax * env.mmax)
    snaps, taken = [], 0
    for k in (0, 5, max(6, ops // 2), 3 * ops + 16):
        env.rollout("random", n_iter=k - taken, autoreset=False)
        taken = k
        snaps.append(env.fork(np.arange(B)))
    stage = np.arange(B) % 3
    stage[B - 2] = 3
    for s, snap in enumerate(snaps):
        env.copy_from(snap, np.where(stage == s, np.arange(B), -1).astype(np.int32))
    host = host_arrays(env)
    assert host["done"][B - 2] and host["env_const"][B - 1, _abi.C_JOBS] == 0 and not host["done"][:B - 2].all()
    A = env.jmax + 1
    J0 = int(host["env_const"][0, _abi.C_JOBS])
    # behind the columns: (parent, action, refused?) -- a parent of -1 and of B, an action of J + 1 and of -3, a job of the done
    # env (no operation left), no move of a live env, no move of the env never reset, the extremes of int32
    extras = [(-1, 0, True), (B, 0, True), (0, J0 + 1, True), (0, -3, True), (B - 2, 0, True), (0, -1, False), (B - 1, -1, True),
              (-2 ** 31, 0, True), (2 ** 31 - 1, 0, True)]
    if (B * A + len(extras)) % 4 == 0:
        extras.append((0, -1, False))
    par = np.concatenate([np.repeat(np.arange(B), A), [e[0] for e in extras]]).astype(np.int32)
    act = np.concatenate([np.tile(np.arange(A), B), [e[1] for e in extras]]).astype(np.int32)
    st = dict(env=env, sd=env.state_dict(), host=host, par=par, act=act, B=B, extras_refused=np.array([e[2] for e in extras]),
              ref={m: reference(host, par, act, m) for m in (False, True)}, ref_states=reference(host))
    _STATES[name] = st
    return st


def env_on(be, name):
    """the case's batch on `be`: the twin's own, or a batch built on `be` that has loaded the twin's state"""
    st = case_state(name)
    if be is twin_backend():
        return st["env"]
    env = CASES[name][0](be)
    env.load_state_dict(st["sd"])
    return env


def call_bound(be, env, parents, actions, use_mask, want=("job", "est"), n=None):
    """jss_bound through the backend's library: (rc, lower_bound, job_bound, est_start) as host arrays; the outputs are
    prefilled (FILL), so what a call leaves alone can be told from what it writes"""
    lib = search.bound_library(be)
    n = (env.batch if parents is None else len(parents)) if n is None else n
    rows = max(n, 1)
    with be.on_device():
        par = None if parents is None else be.from_numpy(np.asarray(parents, np.int32))
        act = None if actions is None else be.from_numpy(np.asarray(actions, np.int32))
        lower = be.from_numpy(np.full(rows, FILL, np.int32))
        jb = be.from_numpy(np.full(rows, FILL, np.int32)) if "job" in want else None
        est = be.from_numpy(np.full((rows, env.jmax, env.mmax), FILL, np.int32)) if "est" in want else None
        p = be.ptr
        arg = _abi.JssBound(n, p(par), p(act), p(env.action_mask) if use_mask else None, p(lower), p(jb), p(est))
        rc = lib.jss_bound(C.byref(env._desc), C.byref(env._state), C.byref(arg), be.stream())
        be.sync()
    host = lambda x: None if x is None else np.asarray(be.numpy(x))   # noqa: E731
    return rc, host(lower), host(jb), host(est)


def same(got, ref, what):
    rc, lower, jb, est = got
    assert rc == 0, (what, rc)
    n = ref[0].size
    assert lower.dtype == np.int32 and np.array_equal(lower[:n], ref[0]), (what, "lower_bound")
    if jb is not None:
        assert np.array_equal(jb[:n], ref[1]), (what, "job_bound")
    if est is not None:
        assert np.array_equal(est[:n], ref[2]), (what, "est_start")


def case_against_mirror(be, name):
    """every column of every env with and without the mask plus the candidates the header refuses, n no multiple of 4; parent ==
    NULL; action == NULL; n == 0; the batch untouched"""
    st = case_state(name)
    env = env_on(be, name)
    B, par, act, host = st["B"], st["par"], st["act"], st["host"]
    before = rows_of(env)
    assert par.size % 4
    for use_mask in (False, True):
        ref = st["ref"][use_mask]
        same(call_bound(be, env, par, act, use_mask), ref, (name, use_mask))
        refused = ref[0] < 0
        assert np.array_equal(refused[-st["extras_refused"].size:], st["extras_refused"])
        assert (ref[2][refused] == FILL).all() and (ref[1][refused] == -1).all()
        assert (ref[0][~refused] >= ref[1][~refused]).all() and (ref[1][~refused] >= 0).all()
    assert (st["ref"][True][0] >= 0).any() and (st["ref"][False][0] >= 0).sum() > (st["ref"][True][0] >= 0).sum()
    # the states' own bounds: parent == NULL and action == NULL; est_start is the solution wherever that is set
    got = call_bound(be, env, None, None, False)
    same(got, st["ref_states"], (name, "states"))
    live = st["ref_states"][0] >= 0
    sol = host["solution"]
    assert live[:B - 1].all() and not live[B - 1]
    assert np.array_equal(got[3][live][sol[live] >= 0], sol[live][sol[live] >= 0])
    assert got[1][B - 2] == host["makespan"][B - 2] == got[2][B - 2]     # a done env: its makespan
    # action == NULL over a parent list, mask given (not looked at without an action); lower_bound alone
    rev = np.arange(B, dtype=np.int32)[::-1].copy()
    ref = reference(host, rev, None, True)
    same(call_bound(be, env, rev, None, True, want=()), ref, (name, "action NULL"))
    same(call_bound(be, env, rev, None, True, want=("est",)), ref, (name, "est alone"))
    # n == 0: nothing runs
    rc, lower, jb, est = call_bound(be, env, rev, rev, True, n=0)
    assert rc == 0 and (lower == FILL).all() and (jb == FILL).all() and (est == FILL).all()
    after = rows_of(env)
    for k in before:
        assert np.array_equal(before[k], after[k]), (name, k)


# ---- anchors -----------------------------------------------------------------------------------------------------------------
def case_hand(be):
    env = BatchedJssEnv(hand_instance(), batch=1, _backend=be)
    env.reset()
    lower, jb, est = (np.asarray(be.numpy(x)) for x in env.lower_bound(job_bound=True, est_start=True))
    assert est[0].tolist() == [[0, 3], [0, 4]] and jb.tolist() == [5] and lower.tolist() == [6]
    cols = np.asarray(be.numpy(env.lower_bound("all")))
    assert cols.shape == (1, 3) and cols[0, 1] == 6
    lower, est = (np.asarray(be.numpy(x)) for x in env.lower_bound(actions=[1], parents=[0], est_start=True))
    assert lower.tolist() == [6] and est[0].tolist() == [[0, 4], [0, 4]]   # J1 holds m1 until 4: J0's second op waits for it


def case_anchor(be, name):
    """at reset the listed bounds; after an SPT episode the bound is the makespan"""
    want_lower, want_job, want_makespan = ANCHORS[name]
    env = BatchedJssEnv(name, batch=1, _backend=be)
    env.reset()
    lower, jb = (np.asarray(be.numpy(x)) for x in env.lower_bound(job_bound=True))
    assert (int(lower[0]), int(jb[0])) == (want_lower, want_job)
    for _ in range(3 * env.jmax * env.mmax):
        if be.numpy(env.done)[0]:
            break
        env.step(env.policy("SPT"))
    assert int(be.numpy(env.makespan)[0]) == want_makespan
    lower, jb = (np.asarray(be.numpy(x)) for x in env.lower_bound(job_bound=True))
    assert int(lower[0]) == want_makespan == int(jb[0])


# ---- properties along episodes -------------------------------------------------------------------------------------------------
def case_properties(be, instance, B=4, columns_every=5, seed=21):
    """Random episodes (NOPEs included) to the end.  At every step: the states' bounds never decrease, never exceed the final
    makespan, and est_start is the solution wherever that is set.  At every `columns_every`-th step, for every legal column:
    parent bound <= candidate bound <= the makespan of lookahead("SPT") of that column.  At done the bound is the makespan."""
    env = BatchedJssEnv(instance, batch=B, _backend=be, seed=seed)
    env.reset()
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    prev = n(env.lower_bound())
    history, checked = [prev], 0
    for step in range(3 * env.jmax * env.mmax):
        done = n(env.done) != 0
        if done.all():
            break
        if step % columns_every == 0:
            cols = n(env.lower_bound("all"))
            upper = n(env.lookahead("SPT")[0])
            mask = n(env.action_mask) != 0
            assert np.array_equal(cols >= 0, mask) and np.array_equal(upper >= 0, mask & ~done[:, None])
            legal = upper >= 0
            assert (cols >= prev[:, None])[legal].all() and (cols <= upper)[legal].all(), step
            checked += int(legal.sum())
            lower, est = (n(x) for x in env.lower_bound(est_start=True))
            sol = n(env.solution)
            assert np.array_equal(lower, prev) and np.array_equal(est[sol >= 0], sol[sol >= 0]), step
            J, M = int(env.jobs_per_env[0]), int(env.machines_per_env[0])
            assert (est[:, :J, :M] >= 0).all() and (est[:, J:] == -1).all() and (est[:, :, M:] == -1).all()
        env.step(env.policy("random"))
        cur = n(env.lower_bound())
        assert (cur >= prev).all(), step
        history.append(cur)
        prev = cur
    assert (n(env.done) != 0).all() and checked > 0
    assert np.array_equal(prev, n(env.makespan)) and (np.array(history) <= prev[None, :]).all()


def case_api(be):
    """BatchedJssEnv.lower_bound's forms against each other and against the raw call; the facade"""
    st = case_state("ragged-interleaved")
    env = env_on(be, "ragged-interleaved")
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    B, A = env.batch, env.jmax + 1
    par, act = np.repeat(np.arange(B), A).astype(np.int32), np.tile(np.arange(A), B).astype(np.int32)
    for legal_only in (True, False):
        ref = reference(st["host"], par, act, legal_only, est_fill=-1)
        lower, jb, est = (n(x) for x in env.lower_bound("all", legal_only=legal_only, job_bound=True, est_start=True))
        assert lower.shape == (B, A) and jb.shape == (B, A) and est.shape == (B, A, env.jmax, env.mmax)
        assert np.array_equal(lower.reshape(-1), ref[0]) and np.array_equal(jb.reshape(-1), ref[1])
        assert np.array_equal(est.reshape(ref[2].shape), ref[2])
        listed = n(env.lower_bound(actions=act[::-1].copy(), parents=par[::-1].copy(), legal_only=legal_only))
        assert listed.shape == (B * A,) and np.array_equal(listed[::-1], ref[0])
    own = n(env.lower_bound())
    assert own.shape == (B,) and own.dtype == np.int32 and np.array_equal(own, st["ref_states"][0])
    for bad in (dict(actions="every"), dict(actions="all", parents=[0]), dict(actions=[0]), dict(parents=[0]),
                dict(actions=[0, 1], parents=[0])):
        try:
            env.lower_bound(**bad)
        except ValueError:
            continue
        raise AssertionError(bad)


# ---- ABI errors ------------------------------------------------------------------------------------------------------------------
def case_abi_errors(be):
    """every code of include/jss_bound.h, before anything runs: the outputs keep their fill"""
    lib = search.bound_library(be)
    env = env_on(be, "3x3")
    B = env.batch
    with be.on_device():
        par = be.from_numpy(np.arange(B, dtype=np.int32))
        out = {k: be.from_numpy(np.full(s, FILL, np.int32)) for k, s in (("lower", B), ("job", B), ("est", (B, env.jmax, env.mmax)))}
    p = be.ptr

    def call(n=B, parent=True, lower=True, desc=None, state=True, arg=True):
        d = _abi.JssDesc.from_buffer_copy(env._desc)
        for k, v in ({} if desc in (None, "null") else desc).items():
            setattr(d, k, v)
        b = _abi.JssBound(n, p(par) if parent else None, p(par), p(env.action_mask), p(out["lower"]) if lower else None,
                          p(out["job"]), p(out["est"]))
        rc = lib.jss_bound(C.byref(d) if desc != "null" else None, C.byref(env._state) if state else None,
                           C.byref(b) if arg else None, be.stream())
        be.sync()
        return rc

    assert call(desc="null") == _abi.E_NULL and call(state=False) == _abi.E_NULL and call(arg=False) == _abi.E_NULL
    assert call(lower=False) == _abi.E_NULL
    assert call(desc={"rem": None}) == _abi.E_NULL and call(desc={"ops": None}) == _abi.E_NULL
    s = _abi.JssState.from_buffer_copy(env._state)
    s.solution = None
    b = _abi.JssBound(B, None, None, None, p(out["lower"]), None, None)
    assert lib.jss_bound(C.byref(env._desc), C.byref(s), C.byref(b), be.stream()) == _abi.E_NULL
    assert call(n=-1) == _abi.E_SHAPE
    assert call(n=B - 1, parent=False) == _abi.E_SHAPE and call(n=B + 1, parent=False) == _abi.E_SHAPE
    assert call(desc={"jmax": 0}) == _abi.E_SHAPE and call(desc={"mmax": 65}) == _abi.E_SHAPE and call(desc={"batch": -1}) == _abi.E_SHAPE
    assert call(desc={"kernel": 64}) == _abi.E_KIND
    assert call(n=0) == 0
    for k, v in out.items():
        assert (np.asarray(be.numpy(v)) == FILL).all(), k
    assert call() == 0 and call(parent=False) == 0
    assert not (np.asarray(be.numpy(out["lower"])) == FILL).any()


# ---- the built library ------------------------------------------------------------------------------------------------------------
def bound_kernel_rows():
    """[(name, vgprs, sgprs, spilled vgprs, spilled sgprs, scratch bytes, LDS bytes)] of libjss_bound_hip.so"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import LLVM, kernel_resources
    from jssenv_amd.build import build_bound_extension
    so = build_bound_extension()                                      # (built here if build() has not run)
    rows = kernel_resources(so)
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "bound.co")
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
