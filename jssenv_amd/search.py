"""Beam search over batched job-shop envs: ``jss_beam_select`` (include/jss_beam.h), its NumPy mirror and the driver.

A beam is G problems of W slots each over a batch of S = G * W envs; a level scores every action of every slot by a rule
rollout (``jss_lookahead``), keeps the W best candidates of every problem -- duplicates merged -- (``jss_beam_select``), clones
the chosen envs into the slots (``jss_clone``) and steps them by the chosen actions (``jss_step``).  The results are defined by
those calls alone: ``beam_select_reference`` is the selection written in NumPy, and the loop of ``beam_search`` written with
``lookahead``, ``beam_select_reference``, ``copy_from`` and ``step`` gives the same bytes (tests/beam_cases.py does that).

Also here: ``lower_bound_reference``, the NumPy mirror of ``jss_bound`` (include/jss_bound.h: makespan lower bounds of states and
of candidate moves, per-operation earliest starts), and ``bound_library``; ``BatchedJssEnv.lower_bound`` is the call.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _abi
from .env import BatchedJssEnv
from .instances import Instance, PackedBatch

SKIP = _abi.ACTION_SKIP


# ---- the selection, in NumPy -------------------------------------------------------------------------------------------
def beam_select_reference(cand_parent, makespan, steps, reward_num, done, env_makespan, width, n_actions, dedupe=True):
    """include/jss_beam.h's semantics on host arrays: returns ``(src, action, score, next_parent, counts)`` as
    ``jss_beam_select`` writes them (int32; shapes (S,), (S,), (S,), (S * A,), (G, 4))."""
    W, A = int(width), int(n_actions)
    cand_parent = np.asarray(cand_parent, dtype=np.int32).reshape(-1)
    S = cand_parent.size // A
    G = S // W
    par = cand_parent.reshape(S, A)
    mk = np.asarray(makespan, dtype=np.int64).reshape(S, A)
    st = np.asarray(steps, dtype=np.int64).reshape(S, A)
    rn = np.asarray(reward_num, dtype=np.int64).reshape(S, A)
    done = np.asarray(done).reshape(S) != 0
    env_mk = np.asarray(env_makespan, dtype=np.int64).reshape(S)
    live = par[:, 0] == np.arange(S)
    running = live & ~done
    # every candidate's triple and validity, (S, A)
    first = np.arange(A) == 0
    valid = np.where(done[:, None], first[None, :], mk >= 0) & live[:, None]
    trip = np.stack([np.where(done[:, None], env_mk[:, None], mk), np.where(done[:, None], 0, st),
                     np.where(done[:, None], 0, rn)], axis=-1)
    src = np.full(S, -1, np.int32)
    action = np.full(S, SKIP, np.int32)
    score = np.full(S, -1, np.int32)
    next_parent = np.full((S, A), -1, np.int32)
    counts = np.zeros((G, 4), np.int32)
    for g in range(G):
        sl = slice(g * W, (g + 1) * W)
        if not running[sl].any():
            next_parent[sl] = par[sl]
            continue
        c = np.flatnonzero(valid[sl].reshape(-1))                     # candidates of the group, index within it
        t = trip[sl].reshape(-1, 3)[c]
        order = np.lexsort((c, t[:, 0]))
        c, t = c[order], t[order]
        keep = np.arange(c.size)
        if dedupe and c.size:
            _, keep = np.unique(t, axis=0, return_index=True)         # the first of every triple in (makespan, c) order
            keep = np.sort(keep)
        taken = keep[:W]
        n = taken.size
        if keep.size >= W:
            dropped = int(taken[-1]) + 1 - W
        else:
            dropped = c.size - keep.size
        d = g * W + np.arange(n)
        w = c[taken] // A
        src[d] = g * W + w
        action[d] = np.where(done[g * W + w], SKIP, c[taken] % A)
        score[d] = t[taken, 0]
        next_parent[d] = d[:, None]
        counts[g] = (n, int(running[sl].sum()), dropped, c.size)
    return src, action, score, next_parent.reshape(-1), counts


# ---- the entry point -----------------------------------------------------------------------------------------------------
def beam_library(backend):
    """The library of ``backend`` that exports include/jss_beam.h: ``backend.beam_lib`` (HipBackend: libjss_beam_hip.so, loaded
    on first use; CpuBackend: the twin), else ``backend.lib`` itself when it carries the symbol."""
    lib = getattr(backend, "beam_lib", None)
    if lib is None:
        lib = backend.lib
        if not hasattr(lib, "jss_beam_select"):
            raise RuntimeError("beam search: the backend's library does not export jss_beam_select (include/jss_beam.h)")
        _abi.bind_beam(lib)
    return lib


def _select_call(be, lib, G, W, A, dedupe, cand_parent, makespan, steps, reward_num, done, env_makespan, src, action, score,
                 next_parent, counts):
    p = be.ptr
    arg = _abi.JssBeam(G, W, A, _abi.BEAM_DEDUPE if dedupe else 0, p(cand_parent), p(makespan), p(steps), p(reward_num), p(done),
                       p(env_makespan), p(src), p(action), p(score), p(next_parent), p(counts))
    rc = lib.jss_beam_select(C.byref(arg), be.stream())
    if rc:
        _abi.check(be.lib, rc, "jss_beam_select")


def beam_select(backend, cand_parent, makespan, steps, reward_num, done, env_makespan, width, n_actions, dedupe=True):
    """``jss_beam_select`` on ``backend`` (include/jss_beam.h): the inputs are host arrays or arrays of the backend, of S * A
    (the first four) and S entries; returns the five outputs ``(src, action, score, next_parent, counts)`` as arrays of the
    backend."""
    be = backend
    W, A = int(width), int(n_actions)

    def dev(x, dtype):
        if isinstance(x, np.ndarray) or not hasattr(x, "data_ptr"):
            return be.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=dtype))
        return x
    with be.on_device():
        par, mk, st = dev(cand_parent, np.int32), dev(makespan, np.int32), dev(steps, np.int32)
        rn, dn, em = dev(reward_num, np.int64), dev(done, np.uint8), dev(env_makespan, np.int32)
        S = int(np.prod(tuple(dn.shape)))
        if W < 1 or S % W or int(np.prod(tuple(par.shape))) != S * A:
            raise ValueError("beam_select: S = len(done) must be a multiple of width, and cand_parent must hold S * n_actions entries")
        G = S // W
        src, action, score = be.zeros((S,), "int32"), be.zeros((S,), "int32"), be.zeros((S,), "int32")
        next_parent, counts = be.zeros((S * A,), "int32"), be.zeros((G, 4), "int32")
        _select_call(be, beam_library(be), G, W, A, dedupe, par, mk, st, rn, dn, em, src, action, score, next_parent, counts)
        be.sync()                                                  # (the uploaded inputs are this call's own)
    return src, action, score, next_parent, counts


def lookahead_into(env, sel, cand_parent, actions, makespan, steps, reward_num, seed, explore_q16, n_iter):
    """``jss_lookahead`` (or its weighted / key namesake: ``sel``, the env's ``_selector``) into the caller's three buffers: the
    raw integer outputs, nothing allocated and nothing computed by the host layer"""
    be = env.backend
    p = be.ptr
    la = _abi.JssLookahead(int(np.prod(tuple(makespan.shape))), p(cand_parent), p(actions), 0, p(makespan), p(steps), p(reward_num))
    sel.call(be.lib, "lookahead", (C.byref(env._desc), C.byref(env._state), C.byref(la)), seed, explore_q16, n_iter, be.stream())


# ---- makespan lower bounds (include/jss_bound.h), in NumPy ----------------------------------------------------------------
def bound_library(backend):
    """The library of ``backend`` that exports include/jss_bound.h: ``backend.bound_lib`` (HipBackend: libjss_bound_hip.so,
    loaded on first use; CpuBackend: the twin), else ``backend.lib`` itself when it carries the symbol."""
    lib = getattr(backend, "bound_lib", None)
    if lib is None:
        lib = backend.lib
        if not hasattr(lib, "jss_bound"):
            raise RuntimeError("lower_bound: the backend's library does not export jss_bound (include/jss_bound.h)")
        _abi.bind_bound(lib)
    return lib


def lower_bound_reference(env_header, env_const, solution, ops, rem, parents=None, actions=None, mask=None, est_fill=None,
                          block=256):
    """include/jss_bound.h's semantics on host arrays, written from the header's definition (all candidates of a block at once,
    one pass per operation index; the per-machine terms by ``ufunc.at``).  ``env_header`` (B, 4), ``env_const`` (B, 12),
    ``solution`` (B, jmax, mmax), ``ops`` / ``rem`` (n_tables, jmax, mmax); ``parents`` / ``actions`` (n,) or None (every env;
    no move); ``mask`` (B, jmax + 1) or None.  Returns ``(lower_bound, job_bound, est_start)``: int32 (n,), (n,) and
    (n, jmax, mmax) -- the last one None unless ``est_fill`` is given, the value rows of refused candidates keep."""
    hdr = np.asarray(env_header, dtype=np.int64).reshape(-1, _abi.NH)
    B = hdr.shape[0]
    const = np.asarray(env_const, dtype=np.int64).reshape(B, _abi.NC)
    sol_all = np.asarray(solution, dtype=np.int64)
    jmax, mmax = sol_all.shape[-2:]
    sol_all = sol_all.reshape(B, jmax, mmax)
    ops = np.asarray(ops, dtype=np.int64).reshape(-1, jmax, mmax)
    rem = np.asarray(rem, dtype=np.int64).reshape(-1, jmax, mmax)
    parents = np.arange(B, dtype=np.int64) if parents is None else np.asarray(parents, dtype=np.int64).reshape(-1)
    n = parents.size
    actions = np.full(n, SKIP, np.int64) if actions is None else np.asarray(actions, dtype=np.int64).reshape(-1)
    lower, jobb = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    est = None if est_fill is None else np.full((n, jmax, mmax), est_fill, np.int32)
    ok = (parents >= 0) & (parents < B)
    par = np.where(ok, parents, 0)
    ok &= const[par, _abi.C_JOBS] > 0
    ok &= (actions >= SKIP) & (actions <= const[par, _abi.C_JOBS])
    if mask is not None:
        mask = np.asarray(mask).reshape(B, jmax + 1)
        ok &= (actions < 0) | (mask[par, np.clip(actions, 0, jmax)] != 0)
    BIG = np.int64(2) ** 40
    kk = np.arange(mmax)

    def prefix(S, D, real):
        """scheduled flags, s_j and jobend_j of solutions S (v, jmax, mmax)"""
        sched = real & (S >= 0)
        s = sched.sum(axis=2)
        last = np.take_along_axis(S + D, np.maximum(s - 1, 0)[:, :, None], axis=2)[:, :, 0]
        return sched, s, np.where(s > 0, last, 0)

    def releases(S, D, mach, sched):
        r = np.zeros((S.shape[0], _abi.MAX_MACHINES), np.int64)
        v = np.nonzero(sched)
        np.maximum.at(r, (v[0], mach[v]), (S + D)[v])
        return r

    for lo in range(0, n, block):
        idx = lo + np.flatnonzero(ok[lo:lo + block])
        if idx.size == 0:
            continue
        p, a = par[idx], actions[idx]
        J, M, tab, t = const[p, _abi.C_JOBS], const[p, _abi.C_MACHINES], const[p, _abi.C_TABLE], hdr[p, _abi.H_CLOCK]
        S = sol_all[p].copy()
        D, mach, R = ops[tab] & 0xFFFF, ops[tab] >> 16, rem[tab]
        real = (np.arange(jmax)[None, :, None] < J[:, None, None]) & (kk[None, None, :] < M[:, None, None])
        rows = np.arange(idx.size)
        sched, s, jobend = prefix(S, D, real)
        # the candidate's move: sol[a][s_a] = h(a, s_a), with the parent's clock
        job = (a >= 0) & (a < J)
        aj = np.where(job, a, 0)
        s_a = s[rows, aj]
        good = ~(job & (s_a >= M))                                    # a job with no operation left: refused
        mv = np.flatnonzero(job & good)
        if mv.size:
            r = releases(S, D, mach, sched)
            m_a = mach[mv, aj[mv], s_a[mv]]
            S[mv, aj[mv], s_a[mv]] = np.maximum(np.maximum(t[mv], jobend[mv, aj[mv]]), r[mv, m_a])
            sched, s, jobend = prefix(S, D, real)
        r = releases(S, D, mach, sched)
        # heads, operation index by operation index
        H = np.zeros_like(S)
        for k in range(mmax):
            rk = np.take_along_axis(r, mach[:, :, k], axis=1)
            first = np.maximum(np.maximum(t[:, None], jobend), rk)
            chain = np.maximum(H[:, :, k - 1] + D[:, :, k - 1], rk) if k else first
            H[:, :, k] = np.where(sched[:, :, k], S[:, :, k], np.where(s == k, first, chain))
        last = (M - 1)[:, None, None]
        ends = (np.take_along_axis(H, last, axis=2) + np.take_along_axis(D, last, axis=2))[:, :, 0]
        jb = np.where(np.arange(jmax)[None, :] < J[:, None], ends, 0).max(axis=1)
        # per machine: min h + sum d + min tail over the unscheduled ops
        minh = np.full((idx.size, _abi.MAX_MACHINES), BIG)
        sumd = np.zeros_like(minh)
        mint = np.full_like(minh, BIG)
        u = np.nonzero(real & ~sched)
        np.minimum.at(minh, (u[0], mach[u]), H[u])
        np.add.at(sumd, (u[0], mach[u]), D[u])
        np.minimum.at(mint, (u[0], mach[u]), (R - D)[u])
        lbm = np.where(minh < BIG, minh + sumd + mint, -1).max(axis=1)
        g = np.flatnonzero(good)
        lower[idx[g]] = np.maximum(jb, lbm)[g]
        jobb[idx[g]] = jb[g]
        if est is not None:
            est[idx[g]] = np.where(real, H, -1)[g]
    return lower, jobb, est


# ---- the driver ------------------------------------------------------------------------------------------------------------
@dataclass
class BeamResult:
    """What ``beam_search`` returns.  ``makespan`` (G,) and ``solution`` (G, jmax, mmax: start times) are slot g * W of the final
    batch ``env``, the lowest of the group by the selection's order; ``levels`` the levels that did work.  With ``record``:
    ``actions``, one list per group that replays its schedule on a fresh env, and the kept per-level outputs ``src``,
    ``action`` and ``score``, (levels, S) each.  ``cand_parent`` (S * A, on the env's device) says which slots of ``env`` are
    live: the last level's ``next_parent``."""
    makespan: np.ndarray
    solution: np.ndarray
    levels: int
    env: BatchedJssEnv
    width: int
    cand_parent: object = None
    actions: Optional[list] = None
    src: Optional[np.ndarray] = None
    action: Optional[np.ndarray] = None
    score: Optional[np.ndarray] = None


def beam_search(instances, kind="SPT", width=64, device=None, dedupe=True, seed=None, explore=0.0, weights=None, keys=None,
                nope_key=None, max_levels=None, check_every=8, record=True, _backend=None):
    """Beam search of width ``width`` on one instance or on a list of them (one group of ``width`` envs per instance, all in
    one batch), with the rule ``kind`` as the continuation that scores a candidate (``weights`` / ``keys`` / ``nope_key``: the
    batch-shared forms of ``lookahead``, shapes (8,) and (jmax, mmax)).

    A level: ``lookahead`` scores every action of every live slot; ``jss_beam_select`` keeps each group's ``width`` best
    candidates in (makespan, candidate index) order, with ``dedupe`` dropping a candidate whose (makespan, steps, return) a
    candidate of a lower index already has; the chosen envs are cloned into a second batch and stepped there by the chosen
    actions, and the filled slots are cloned back.  A finished schedule stays in the beam and competes.  Nothing of a level is
    computed by torch and nothing comes back to the host; every ``check_every`` levels the driver reads the levels' counts and
    stops at the first level that found no group with a running slot (or at ``max_levels``, default 3 * jmax * mmax).  Levels
    run past that one change nothing, so the result does not depend on ``check_every``.

    Dedupe merges by the continuation's signature, a heuristic identity: permutations of one partial schedule have equal
    signatures, and so may two different states.  Without it a beam fills with such permutations and finds what width 1 -- the
    pilot method -- finds.  With a deterministic rule the best score of a group never rises from one level to the next (the
    best candidate's rule move is among its children); with ``kind="random"`` or ``explore > 0`` that does not hold, and the
    result is the best of the final beam."""
    W = int(width)
    if W < 1:
        raise ValueError("beam_search: width must be >= 1")
    check_every = int(check_every)
    if check_every < 1:
        raise ValueError("beam_search: check_every must be >= 1")
    if isinstance(instances, (PackedBatch, BatchedJssEnv)):
        raise NotImplementedError("beam_search takes instances (a name, a path, an Instance, or a list of them): generated batches, "
                                  "per-env tables and by-shape batches are not searched")
    one = isinstance(instances, (str, os.PathLike, Instance))
    names = [instances] if one else list(instances)
    G = len(names)
    if G < 1:
        raise ValueError("beam_search: need at least one instance")
    S = G * W
    kw = dict(device=device) if _backend is None else dict(_backend=_backend)
    if G == 1:
        a = BatchedJssEnv(names[0], batch=S, seed=int(seed or 0), **kw)
    else:
        a = BatchedJssEnv(names, batch=S, table_of_env=np.repeat(np.arange(G), W), order="interleaved", seed=int(seed or 0), **kw)
    be, A = a.backend, a.jmax + 1
    if W * A > 65536:
        raise ValueError(f"beam_search: width * (jmax + 1) = {W * A} exceeds 65536 (include/jss_beam.h)")
    for x, name, one_shape in ((weights, "weights", (_abi.RW_N,)), (keys, "keys", (a.jmax, a.mmax))):
        if x is not None and tuple(x.shape) != one_shape:
            raise ValueError(f"beam_search: {name} must have the batch-shared shape {one_shape} (the slots of a beam change hands)")
    sel = a._selector(kind, "beam_search", weights, keys, nope_key)
    lib = beam_library(be)
    _abi.ensure_bound(be.lib, "jss")
    n_iter = 3 * a.jmax * a.mmax
    max_levels = n_iter if max_levels is None else int(max_levels)
    la_seed, explore_q16 = a.seed if seed is None else int(seed), int(round(explore * 65536))

    a.reset()
    b = a.fork(np.arange(S))
    # which clone call: on the device the index stays there (a slot's source is a slot of its own group, and the clone back is
    # the identity: the host mirrors of the instance assignment never change)
    on_device = getattr(be, "name", "") == "hip"
    clone = (lambda dst, src, idx: dst._clone_from(src, idx)) if on_device else (lambda dst, src, idx: dst.copy_from(src, idx))
    with be.on_device():
        first = np.where(np.arange(S) % W == 0, np.arange(S), -1).astype(np.int32)
        cand = [be.from_numpy(np.repeat(first, A)), be.zeros((S * A,), "int32")]
        acts = be.from_numpy(np.tile(np.arange(A, dtype=np.int32), S))
        mk, st, rn = be.zeros((S * A,), "int32"), be.zeros((S * A,), "int32"), be.zeros((S * A,), "int64")
        win_src, win_act, win_score = (be.zeros((check_every, S), "int32") for _ in range(3))
        win_counts = be.zeros((check_every, G, 4), "int32")
        hist = {"src": [], "action": [], "score": []}
        levels, cur, finished = 0, 0, False
        while levels < max_levels and not finished:
            n_win = min(check_every, max_levels - levels)
            for i in range(n_win):
                lookahead_into(a, sel, cand[cur], acts, mk, st, rn, la_seed, explore_q16, n_iter)
                _select_call(be, lib, G, W, A, dedupe, cand[cur], mk, st, rn, a.done, a.makespan, win_src[i], win_act[i],
                             win_score[i], cand[1 - cur], win_counts[i])
                clone(b, a, win_src[i])
                b.step(win_act[i])
                clone(a, b, cand[1 - cur][::A])            # the filled slots back: next_parent[d * A] is d or -1
                cur = 1 - cur
            counts = be.numpy(win_counts)[:n_win]                       # the one host round trip of the window
            idle = np.flatnonzero((counts[:, :, 1] == 0).all(axis=1))
            done_at = int(idle[0]) if idle.size else n_win
            finished = bool(idle.size)
            if record and done_at:
                for name, win in (("src", win_src), ("action", win_act), ("score", win_score)):
                    hist[name].append(be.numpy(win)[:done_at])
            levels += done_at
        makespan = be.numpy(a.makespan)[::W].astype(np.int32)
        solution = be.numpy(a.solution)[::W].copy()
    res = BeamResult(makespan=makespan, solution=solution, levels=levels, env=a, width=W, cand_parent=cand[cur])
    if record:
        for name in hist:
            setattr(res, name, np.concatenate(hist[name]) if hist[name] else np.zeros((0, S), np.int32))
        res.actions = [_walk_back(res.src, res.action, g * W) for g in range(G)]
    return res


def _walk_back(src, action, slot):
    """the actions that led to ``slot`` of the final beam, from the kept per-level outputs"""
    out = []
    for lv in range(src.shape[0] - 1, -1, -1):
        if src[lv, slot] < 0:                      # the group had finished by this level
            continue
        if action[lv, slot] != SKIP:               # (SKIP: a finished schedule carried along)
            out.append(int(action[lv, slot]))
        slot = int(src[lv, slot])
    return out[::-1]
