"""Backend-agnostic cases of jss_beam_select (include/jss_beam.h) and jssenv_amd.search.beam_search, run against the host-core
twin, the kernel source (jssenv_amd/csrc/jss_beam.hip) under the SIMT emulator and the HIP library libjss_beam_hip.so.

The selection's reference is search.beam_select_reference (NumPy); the driver's is its definition: the loop below, written from
lookahead, beam_select_reference, copy_from and step."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

from clone_cases import rows_of
from jssenv_amd import BatchedJssEnv, _abi, search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
BEAM_SRC = os.path.join(ROOT, "jssenv_amd", "csrc", "jss_beam.hip")
EMU_LIB = os.path.join(EMU, "libjss_beam_emu.so")
LDS_CAP = 2048          # kBeamCap of jss_beam.hip: a group with more valid candidates takes the kernel's rescanning path

# (G, W, A) of the synthetic inputs; the last one has a group on either side of LDS_CAP
SHAPES = [(1, 1, 2), (3, 4, 16), (5, 7, 21), (2, 64, 16), (1, 32, 101), (2, 240, 21)]
OUTPUTS = ("src", "action", "score", "next_parent", "counts")


def build_emu_beam():
    """jss_beam.hip, unmodified, compiled with g++ against the SIMT emulator's hip_runtime.h: a library of its own"""
    deps = [BEAM_SRC, os.path.join(EMU, "hip", "hip_runtime.h"), os.path.join(ROOT, "include", "jss_beam.h"),
            os.path.join(ROOT, "jssenv_amd", "csrc", "jss_abi_checks.hpp")]
    if not os.path.isfile(EMU_LIB) or any(os.path.getmtime(d) > os.path.getmtime(EMU_LIB) for d in deps):
        tmp = EMU_LIB + f".tmp{os.getpid()}"
        subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
                               "-Wno-unknown-pragmas", "-I" + EMU, "-I" + os.path.join(ROOT, "include"), BEAM_SRC, "-o", tmp])
        os.replace(tmp, EMU_LIB)
    return EMU_LIB


def emu_backend():
    """the emulator backend of the env kernels, with the emulated beam library attached as its `beam_lib`"""
    sys.path.insert(0, EMU)
    from emu_backend import EmuBackend
    be = EmuBackend(default_kernel="auto")
    be.beam_lib = _abi.bind_beam(C.CDLL(build_emu_beam()))
    return be


# ---- synthetic inputs ------------------------------------------------------------------------------------------------------
def make_inputs(G, W, A, seed, kinds=None):
    """Seeded inputs of jss_beam_select.  Makespans come from 8 values, steps from 4 and returns from 6, so that ties and equal
    triples are common; about a third of a running slot's columns are -1; a tenth of the slots are dead and a tenth done (with
    env_makespan); dead and done slots carry garbage in the lookahead arrays, which the selection must not read as candidates.
    Kind of group g (default: by g % 5 when G >= 3): "normal"; "finished" (live slots all done, or none live); "few" (one
    running slot with two legal columns: fewer survivors than W); "novalid" (running slots whose columns are all -1);
    "sparse" (two thirds of the slots dead)."""
    rng = np.random.default_rng(seed)
    S = G * W
    if kinds is None:
        kinds = [("normal", "finished", "few", "novalid", "normal")[g % 5] if G >= 3 else "normal" for g in range(G)]
    makespan = (1000 + 7 * rng.integers(0, 8, (S, A))).astype(np.int32)
    makespan[rng.random((S, A)) < 1 / 3] = -1
    steps = rng.integers(20, 24, (S, A)).astype(np.int32)
    # (returns that differ in bit 40 alone: all 64 bits take part in the comparison)
    rnum = (rng.integers(-1, 2, (S, A)) * 1000 + (rng.integers(0, 2, (S, A)) << 40)).astype(np.int64)
    state = rng.choice(3, S, p=[0.8, 0.1, 0.1])                                       # 0 running, 1 dead, 2 done
    for g, kind in enumerate(kinds):
        sl = slice(g * W, (g + 1) * W)
        if kind == "finished":
            state[sl] = rng.choice([1, 2], W) if g % 2 else 1
        elif kind == "few":
            state[sl] = 1
            state[g * W + W // 2] = 0
            makespan[g * W + W // 2] = -1
            makespan[g * W + W // 2, [0, A - 1]] = [1007, 1000]
        elif kind == "novalid":
            state[sl] = np.where(state[sl] == 2, 1, state[sl])
            state[g * W] = 0
            makespan[sl] = -1
        elif kind == "sparse":
            state[sl] = np.where(rng.random(W) < 2 / 3, 1, state[sl])
        elif W > 1:
            state[g * W + rng.integers(0, W)] = 0                                      # (a normal group is unfinished)
        else:
            state[sl] = 0
    slots = np.arange(S, dtype=np.int32)
    cand_parent = np.repeat(np.where(state == 1, -1, slots).astype(np.int32), A)
    done = (state == 2).astype(np.uint8)
    env_makespan = np.where(state == 2, 1000 + 7 * rng.integers(0, 8, S), rng.integers(0, 900, S)).astype(np.int32)
    return dict(cand_parent=cand_parent, makespan=makespan.reshape(-1), steps=steps.reshape(-1), reward_num=rnum.reshape(-1),
                done=done, env_makespan=env_makespan, width=W, n_actions=A), kinds


def threshold_inputs():
    """two groups of 128 running slots x 17 actions: exactly LDS_CAP valid candidates in group 0, one more in group 1"""
    W, A = 128, 17
    inp, _ = make_inputs(2, W, A, seed=77, kinds=["normal", "normal"])
    inp["cand_parent"] = np.repeat(np.arange(2 * W, dtype=np.int32), A)
    inp["done"][:] = 0
    mk = np.abs(inp["makespan"]).reshape(2, W * A)
    mk[0, LDS_CAP:] = -1
    mk[1, LDS_CAP + 1:] = -1
    inp["makespan"] = np.ascontiguousarray(mk.reshape(-1))
    return inp


def select_on(be, inp, dedupe):
    out = search.beam_select(be, **inp, dedupe=dedupe)
    return [np.asarray(be.numpy(x)).reshape(-1) for x in out]


def check_select(be, inp, dedupe, kinds=None):
    """the backend's five outputs against the NumPy mirror, bit for bit; what the special groups must show"""
    ref = search.beam_select_reference(**inp, dedupe=dedupe)
    got = select_on(be, inp, dedupe)
    for name, r, g in zip(OUTPUTS, ref, got):
        assert g.dtype == np.int32 and np.array_equal(np.asarray(r).reshape(-1), g), (name, dedupe)
    W, A = inp["width"], inp["n_actions"]
    src, action, score, nxt, counts = ref
    for g, kind in enumerate(kinds or ()):
        sl, cl = slice(g * W, (g + 1) * W), slice(g * W * A, (g + 1) * W * A)
        if kind == "finished":                     # left alone
            assert (src[sl] == -1).all() and (action[sl] == _abi.ACTION_SKIP).all() and (score[sl] == -1).all()
            assert np.array_equal(nxt[cl], inp["cand_parent"][cl]) and (counts[g] == 0).all()
        if kind == "few":
            assert 0 < counts[g, 0] < W or W <= 2
        if kind == "novalid":
            assert counts[g, 0] == 0 and counts[g, 1] > 0 and counts[g, 3] == 0 and (nxt[cl] == -1).all()
    return counts


def case_select_shape(be, shape):
    G, W, A = shape
    for seed in (1, 2):
        kinds = ["normal", "sparse"] if shape == SHAPES[-1] else None
        inp, kinds = make_inputs(G, W, A, seed, kinds)
        for dedupe in (True, False):
            counts = check_select(be, inp, dedupe, kinds)
            if shape == SHAPES[-1]:
                assert counts[0, 3] > LDS_CAP >= counts[1, 3] > 0


def case_threshold(be):
    inp = threshold_inputs()
    for dedupe in (True, False):
        counts = check_select(be, inp, dedupe)
        assert counts[0, 3] == LDS_CAP and counts[1, 3] == LDS_CAP + 1


# ---- ABI errors --------------------------------------------------------------------------------------------------------------
def case_abi_errors(be):
    """every code of include/jss_beam.h, before anything runs: the outputs keep their fill"""
    lib = search.beam_library(be)
    G, W, A = 2, 3, 5
    inp, _ = make_inputs(G, W, A, 3, ["normal", "normal"])
    names = ("cand_parent", "makespan", "steps", "reward_num", "done", "env_makespan")
    with be.on_device():
        bufs = {k: be.from_numpy(inp[k]) for k in names}
        for k, n in (("src", G * W), ("action", G * W), ("score", G * W), ("next_parent", G * W * A), ("counts", G * 4)):
            bufs[k] = be.from_numpy(np.full(n, 12345, np.int32))
    fields = names + OUTPUTS

    def call(G_=G, W_=W, A_=A, null=None, alias=False):
        ptrs = {k: be.ptr(bufs[k]) for k in fields}
        if null:
            ptrs[null] = 0
        if alias:
            ptrs["next_parent"] = ptrs["cand_parent"]
        arg = _abi.JssBeam(G_, W_, A_, 1, *[ptrs[k] for k in fields])
        rc = lib.jss_beam_select(C.byref(arg), be.stream())
        be.sync()
        return rc

    assert lib.jss_beam_select(None, be.stream()) == _abi.E_NULL
    for k in fields:
        assert call(null=k) == _abi.E_NULL, k
    assert call(G_=-1) == _abi.E_SHAPE
    assert call(W_=0) == _abi.E_SHAPE
    assert call(A_=1) == _abi.E_SHAPE
    assert call(W_=4096, A_=17) == _abi.E_SHAPE                      # 69 632 candidates per group
    assert call(alias=True) == _abi.E_SHAPE
    assert call(G_=0) == 0                                           # nothing to do, nothing launched
    for k in OUTPUTS:
        assert (np.asarray(be.numpy(bufs[k])) == 12345).all(), k
    for k in names:
        assert np.array_equal(np.asarray(be.numpy(bufs[k])).reshape(-1), inp[k]), k
    assert call() == 0
    assert not (np.asarray(be.numpy(bufs["src"])) == 12345).any()


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def make_beam_env(be, instances, W, seed=0):
    if isinstance(instances, str):
        return BatchedJssEnv(instances, batch=W, seed=seed, _backend=be)
    G = len(instances)
    return BatchedJssEnv(instances, batch=G * W, table_of_env=np.repeat(np.arange(G), W), order="interleaved", seed=seed,
                         _backend=be)


def definition_loop(be, instances, W, kind="SPT", dedupe=True, max_levels=None, truncated_return=False):
    """beam_search as its documentation defines it, from the public calls and the NumPy selection.  `lookahead` returns the
    float32 return reward_num / max_time_op; the numerator is rint(return * max_time_op), exact while |reward_num| < 2^23 (the
    quotient's relative error is 2^-24, and a numerator is at most an instance's total work, below 10^5 here).
    `truncated_return`: the triple's third member is the float return cut to a whole number instead, a coarser identity than
    include/jss_beam.h's -- not what the library does; test_beam.test_listed_anchors says what it is for.
    Returns (final batch, per-level src, per-level action, per-level score, per-level counts)."""
    a = make_beam_env(be, instances, W)
    S, A = a.batch, a.jmax + 1
    a.reset()
    b = a.fork(np.arange(S))
    mto = np.asarray(be.numpy(a.env_const))[:, _abi.C_MAX_TIME_OP].astype(np.float64)
    cand = np.repeat(np.where(np.arange(S) % W == 0, np.arange(S), -1).astype(np.int32), A)
    acts = np.tile(np.arange(A, dtype=np.int32), S)
    hist = ([], [], [], [])
    for _ in range(3 * a.jmax * a.mmax if max_levels is None else max_levels):
        mk, st, ret = (np.asarray(be.numpy(x)) for x in a.lookahead(kind, parents=cand, actions=acts))
        if truncated_return:
            rnum = ret.astype(np.int64)
        else:
            rnum = np.rint(ret.astype(np.float64) * mto[np.clip(cand, 0, S - 1)]).astype(np.int64)
        src, action, score, nxt, counts = search.beam_select_reference(cand, mk, st, rnum, be.numpy(a.done), be.numpy(a.makespan),
                                                                       W, A, dedupe)
        if (counts[:, 1] == 0).all():
            break
        b.copy_from(a, src)
        b.step(action)
        a.copy_from(b, nxt[::A].copy())
        cand = nxt
        for h, x in zip(hist, (src, action, score, counts)):
            h.append(x)
    return (a,) + tuple(np.array(h, dtype=np.int32).reshape(-1, S) for h in hist[:3]) + (np.array(hist[3], np.int32).reshape(-1, S // W, 4),)


def check_driver(be, instances, W, max_levels=None, check_every=(1, 8), definition_on=None):
    """beam_search is its definition: per-level src / action, the final batch byte for byte, whatever check_every is.
    `definition_on`: the backend that runs the definition loop when it is not `be` (the emulator is slow, and its rows are the
    twin's byte for byte)"""
    env, src, action, score, _ = definition_loop(definition_on or be, instances, W, max_levels=max_levels)
    want = rows_of(env)
    res = None
    for every in check_every:
        res = search.beam_search(instances, "SPT", width=W, max_levels=max_levels, check_every=every, _backend=be)
        assert res.levels == src.shape[0], (every, res.levels, src.shape[0])
        assert np.array_equal(res.src, src) and np.array_equal(res.action, action) and np.array_equal(res.score, score), every
        got = rows_of(res.env)
        for k in want:
            assert np.array_equal(got[k], want[k]), (k, every)
    return res


def replay(be, instance, actions):
    """a fresh B = 1 env stepped through `actions`: (makespan, solution, done)"""
    env = BatchedJssEnv(instance, batch=1, _backend=be)
    env.reset()
    for a in actions:
        env.step(np.array([a], np.int32))
    return int(be.numpy(env.makespan)[0]), np.asarray(be.numpy(env.solution))[0], bool(be.numpy(env.done)[0])


def pilot_loop(be, instance="ta01"):
    """the pilot method at B = 1: (actions, makespan)"""
    env = BatchedJssEnv(instance, batch=1, _backend=be)
    env.reset()
    out = []
    for _ in range(3 * env.jmax * env.mmax):
        if be.numpy(env.done)[0]:
            break
        info = env.pilot_step("SPT")[4]
        out.append(int(be.numpy(info["action"])[0]))
    return out, int(be.numpy(env.makespan)[0])


# ---- the built library ------------------------------------------------------------------------------------------------------------
def beam_kernel_rows():
    """[(name, vgprs, sgprs, spilled vgprs, spilled sgprs, scratch bytes, LDS bytes)] of libjss_beam_hip.so"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import LLVM, kernel_resources
    from jssenv_amd.build import build_beam_extension
    so = build_beam_extension()                                       # (built here if build() has not run)
    rows = kernel_resources(so)
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "beam.co")
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", so, fat], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    lds = [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", notes)]
    assert len(lds) == len(rows)
    return [r + (b,) for r, b in zip(rows, lds)]
