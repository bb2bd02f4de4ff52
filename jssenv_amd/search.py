"""Beam search over batched job-shop envs: ``jss_beam_select`` (include/jss_beam.h), its NumPy mirror and the driver.

A beam is G problems of W slots each over a batch of S = G * W envs; a level scores every action of every slot by a rule
rollout (``jss_lookahead``), keeps the W best candidates of every problem -- duplicates merged -- (``jss_beam_select``), clones
the chosen envs into the slots (``jss_clone``) and steps them by the chosen actions (``jss_step``).  The results are defined by
those calls alone: ``beam_select_reference`` is the selection written in NumPy, and the loop of ``beam_search`` written with
``lookahead``, ``beam_select_reference``, ``copy_from`` and ``step`` gives the same bytes (tests/beam_cases.py does that).

Also here: ``lower_bound_reference``, the NumPy mirror of ``jss_bound`` (include/jss_bound.h: makespan lower bounds of states and
of candidate moves, per-operation earliest starts), and ``bound_library``; ``BatchedJssEnv.lower_bound`` is the call.

And the evaluation of machine orders (include/jss_order.h): ``order_eval_reference``, the NumPy mirror of ``jss_order_eval``,
``order_library``, and ``improve``, steepest descent over swaps of adjacent critical operations -- three launches per iteration,
defined by ``BatchedJssEnv.evaluate_order``, an arg-min and a swap (tests/order_cases.py writes that loop out).

And tabu search over that neighbourhood (include/jss_tabu.h): ``tabu_reference``, the NumPy mirror of ``jss_tabu_search`` on top of
``order_eval_reference``, ``tabu_library``, and ``tabu_search``, the driver: many walkers per instance, whole walks in one launch
(``BatchedJssEnv.tabu``), defined by ``reset``, ``lower_bound``, ``rollout``, ``tabu`` and ``evaluate_order`` alone
(tests/tabu_cases.py writes that loop out).

And the same walk over block insertions (include/jss_block.h): ``block_reference``, the NumPy mirror of ``jss_block_search``,
``block_library``, and ``tabu_search(moves="block")`` through ``BatchedJssEnv.tabu_blocks``.

And path relinking between machine orders (include/jss_relink.h): ``relink_reference``, the NumPy mirror of ``jss_relink_walk``,
``relink_library``, and ``relink_search``, the population driver: block walks whose walkers restart from a point on the path to
their group's elite order, defined by ``tabu_blocks``, ``order_distance`` and ``relink`` (tests/relink_cases.py writes that loop
out).

And Giffler-Thompson decoding of key tables (include/jss_decode.h): ``decode_reference`` and ``evolve_reference``, the NumPy mirrors
of ``jss_decode_keys`` and ``jss_keys_evolve``, ``rng_u32``, the libraries' counter RNG, ``decode_library``, and ``brkga_search``, a
biased random-key genetic algorithm defined by ``decode_keys``, ``evolve_keys``, ``lower_bound`` and ``tabu_blocks``
(tests/decode_cases.py writes that loop out).

And one-machine relaxations of partial selections (include/jss_machine.h): ``machine_reference`` and ``bottleneck_reference``, the
NumPy mirrors of ``jss_machine_relax`` and ``jss_bottleneck_build`` and their executable definition, ``machine_library``, and
``bottleneck_search``, biased shifting bottleneck builds defined by ``relax_machines``, ``bottleneck``, ``tabu_blocks`` and
``evaluate_order`` (tests/machine_cases.py writes that loop out).  ``target="one_machine"`` of ``tabu_search``, ``relink_search``
and ``brkga_search`` is ``relax_machines()`` of the empty selection, a stronger bound than ``lower_bound()`` of the reset state.

And Carlier's branch and bound for those one-machine problems (include/jss_carlier.h): ``carlier_reference``, the search itself,
``solve_reference`` and ``bottleneck_exact_reference``, the NumPy mirrors of ``jss_machine_solve`` and ``jss_bottleneck_exact`` and
their executable definition, ``carlier_library``, ``bottleneck_search(nodes=...)`` and ``target="one_machine_exact"``.

And constraint propagation on operation windows (include/jss_propagate.h): ``propagate_reference``, the NumPy mirror of
``jss_propagate`` and its executable definition, ``propagate_library``, ``destructive_bound`` -- trial makespans scanned upward and
shaved on the device -- with ``destructive_reference``, the same loop over the mirror, and ``target="destructive"``.
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
from .search_calls import library

SKIP = _abi.ACTION_SKIP


# ---- the library of a family on a backend (search_calls.library), by the names the case modules of the tests call -----------
def beam_library(backend): return library(backend, "beam")                # noqa: E704
def bound_library(backend): return library(backend, "bound")              # noqa: E704
def order_library(backend): return library(backend, "order")              # noqa: E704
def tabu_library(backend): return library(backend, "tabu")                # noqa: E704
def block_library(backend): return library(backend, "block")              # noqa: E704
def relink_library(backend): return library(backend, "relink")            # noqa: E704
def decode_library(backend): return library(backend, "decode")            # noqa: E704
def machine_library(backend): return library(backend, "machine")          # noqa: E704
def carlier_library(backend): return library(backend, "carlier")          # noqa: E704
def propagate_library(backend): return library(backend, "propagate")      # noqa: E704


# ---- what the drivers share: the instances, the batch of groups, the target, the winners ----------------------------------------
_TARGETS = ("lower_bound", "one_machine", "one_machine_exact", "destructive")


def _instance_groups(what, instances, hint):
    """``names, G``: the instances of a driver as a list and their number; NotImplementedError for an env object, with ``hint``,
    the call that serves it instead"""
    if isinstance(instances, (PackedBatch, BatchedJssEnv)) or type(instances).__name__ in ("BucketedJssEnv", "JssVectorEnv", "JssEnv"):
        raise NotImplementedError(f"{what} takes instances (a name, a path, an Instance, or a list of them): {hint}")
    names = [instances] if isinstance(instances, (str, os.PathLike, Instance)) else list(instances)
    if len(names) < 1:
        raise ValueError(f"{what}: need at least one instance")
    return names, len(names)


def _grouped_env(names, per_group, seed, device, _backend):
    """one batch of ``len(names)`` groups of ``per_group`` envs each, group g on instance g"""
    kw = dict(device=device) if _backend is None else dict(_backend=_backend)
    if len(names) == 1:
        return BatchedJssEnv(names[0], batch=per_group, seed=int(seed or 0), **kw)
    return BatchedJssEnv(names, batch=len(names) * per_group, table_of_env=np.repeat(np.arange(len(names)), per_group),
                         order="interleaved", seed=int(seed or 0), **kw)


def _check_target(what, target):
    if isinstance(target, str) and target not in _TARGETS:
        raise ValueError(f"{what}: target is 'lower_bound', 'one_machine', 'one_machine_exact', 'destructive', None, an int or one int per instance")


def _resolve_target(what, env, target, G, per_group):
    """The target of every env of the (reset) batch ``env``: a bound by its name, as the batch's backend returns it; None; or an
    int, or one per instance, repeated over the groups' envs on the host."""
    _check_target(what, target)
    if isinstance(target, str):
        return (env.lower_bound() if target == "lower_bound" else env.relax_machines()[0] if target == "one_machine"
                else env.solve_machines()[0] if target == "one_machine_exact" else _destructive_target(env, G, per_group))
    if target is None:
        return None
    return np.repeat(np.broadcast_to(np.asarray(target, np.int32), (G,)), per_group)


def _group_winners(mk, G, W):
    """``walker, winner``: of every group of W the walker with the lowest ``(makespan, walker)`` -- one without a schedule counts
    as +inf --, within its group and within the batch"""
    by_group = np.where(mk >= 0, mk.astype(np.int64), np.iinfo(np.int64).max).reshape(G, W)
    walker = by_group.argmin(axis=1).astype(np.int32)                # (the first of equal makespans)
    return walker, (np.arange(G) * W + walker).astype(np.int32)


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


# ---- machine orders (include/jss_order.h), in NumPy ---------------------------------------------------------------------------
def order_eval_reference(env_const, ops, rank, parents=None, swap_a=None, swap_b=None, pair_cap=None, fill=-1):
    """include/jss_order.h's jss_order_eval on host arrays, written from the header's definition, one candidate after the
    other: the machines' orders by a lexicographic sort, the starts over the operations in an order in which every predecessor
    comes first (what cannot be so ordered is cyclic), the tails over the same order backwards, the pairs by a walk along the
    machines.  ``env_const`` (B, 12), ``ops`` (n_tables, jmax, mmax), ``rank`` (B, jmax, mmax); ``parents``, ``swap_a``,
    ``swap_b`` (n,) or None.  Returns ``(makespan, start, tail, pair_a, pair_b, n_pairs)``: int32 (n,), (n, jmax, mmax) twice,
    (n, pair_cap) twice and (n,) -- the pair outputs None unless ``pair_cap`` is given.  Rows of refused (-1) and cyclic (-2)
    candidates hold ``fill`` in every output but the makespan."""
    rank = np.asarray(rank, dtype=np.int64)
    B, jmax, mmax = rank.shape
    const = np.asarray(env_const, dtype=np.int64).reshape(B, _abi.NC)
    ops = np.asarray(ops, dtype=np.int64).reshape(-1, jmax, mmax)
    region = jmax * mmax
    parents = np.arange(B) if parents is None else np.asarray(parents, dtype=np.int64).reshape(-1)
    n = parents.size
    swap_a = np.full(n, -1, np.int64) if swap_a is None else np.asarray(swap_a, dtype=np.int64).reshape(-1)
    swap_b = np.full(n, -1, np.int64) if swap_b is None else np.asarray(swap_b, dtype=np.int64).reshape(-1)
    makespan = np.full(n, -1, np.int32)
    start = np.full((n, jmax, mmax), fill, np.int32)
    tail = np.full((n, jmax, mmax), fill, np.int32)
    cap = None if pair_cap is None else int(pair_cap)
    pair_a = pair_b = n_pairs = None
    if cap is not None:
        pair_a, pair_b, n_pairs = np.full((n, cap), fill, np.int32), np.full((n, cap), fill, np.int32), np.full(n, fill, np.int32)
    for c in range(n):
        i, a, b = int(parents[c]), int(swap_a[c]), int(swap_b[c])
        if not 0 <= i < B:
            continue
        J, M, tab = (int(x) for x in const[i, [_abi.C_JOBS, _abi.C_MACHINES, _abi.C_TABLE]])
        if J < 1:
            continue
        real = np.zeros((jmax, mmax), bool)
        real[:J, :M] = True
        flat_real = real.reshape(-1)
        r = rank[i].reshape(-1).copy()
        if (r[flat_real] < 0).any():
            continue
        if (a, b) != (-1, -1):
            if not (0 <= a < region and 0 <= b < region and flat_real[a] and flat_real[b]):
                continue
            r[a], r[b] = r[b], r[a]
        mach = (ops[tab].reshape(-1) >> 16) & 63
        dur = ops[tab].reshape(-1) & 0xFFFF
        real_ops = np.flatnonzero(flat_real)
        before = np.full(region, -1)                                  # the operation before / behind on the machine
        behind = np.full(region, -1)
        orders = []
        for m in range(_abi.MAX_MACHINES):
            on = real_ops[mach[real_ops] == m]
            on = on[np.lexsort((on, r[on]))]                          # by (rank, flat index) = (rank, j, k)
            orders.append(on)
            before[on[1:]], behind[on[:-1]] = on[:-1], on[1:]
        waits = np.zeros(region, np.int64)                            # predecessors not placed yet
        waits[real_ops] = (real_ops % mmax > 0).astype(np.int64) + (before[real_ops] >= 0)
        st = np.zeros(region, np.int64)
        todo = [int(e) for e in real_ops if waits[e] == 0]
        placed = []
        while todo:
            e = todo.pop()
            placed.append(e)
            end = st[e] + dur[e]
            for nxt in ((e + 1) if e % mmax + 1 < M else -1, int(behind[e])):
                if nxt >= 0:
                    st[nxt] = max(st[nxt], end)
                    waits[nxt] -= 1
                    if waits[nxt] == 0:
                        todo.append(nxt)
        if len(placed) != real_ops.size:
            makespan[c] = -2
            continue
        mk = int((st + dur)[real_ops].max())
        tl = np.zeros(region, np.int64)
        for e in reversed(placed):
            job_next = e + 1 if e % mmax + 1 < M else -1
            for nxt in (job_next, int(behind[e])):
                if nxt >= 0:
                    tl[e] = max(tl[e], dur[nxt] + tl[nxt])
        makespan[c] = mk
        start[c] = np.where(flat_real, st, -1).reshape(jmax, mmax)
        tail[c] = np.where(flat_real, tl, -1).reshape(jmax, mmax)
        if cap is not None:
            critical = st + dur + tl == mk
            found = []
            for on in orders:
                for u, v in zip(on[:-1], on[1:]):
                    if u // mmax != v // mmax and critical[u] and critical[v] and st[v] == st[u] + dur[u]:
                        found.append((int(u), int(v)))
            n_pairs[c] = len(found)
            pair_a[c], pair_b[c] = -1, -1
            for k, (u, v) in enumerate(found[:cap]):
                pair_a[c, k], pair_b[c, k] = u, v
    return makespan, start, tail, pair_a, pair_b, n_pairs


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
    a = _grouped_env(names, W, seed, device, _backend)
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


# ---- descent over swaps of adjacent critical operations -----------------------------------------------------------------------
@dataclass
class ImproveResult:
    """What ``improve`` returns, host arrays: ``makespan_before`` and ``makespan`` (B,), the final ``rank`` and the ``start``
    times of its schedule (B, jmax, mmax; a negative makespan and -1 rows: the env's schedule could not be evaluated).
    ``iterations``: those in which some env improved; ``evaluations``: swap candidates evaluated, over all envs and all
    iterations up to and including the one that improved nothing; ``truncated``: the (env, iteration) whose neighbourhood did
    not fit ``pair_cap``; ``history`` (iterations run, B): the makespans at the start of every iteration; ``env`` the batch."""
    makespan_before: np.ndarray
    makespan: np.ndarray
    rank: np.ndarray
    start: np.ndarray
    iterations: int
    evaluations: int
    truncated: int
    history: Optional[np.ndarray] = None
    env: Optional[BatchedJssEnv] = None


def improve(env_or_instances, kind="SPT", max_iter=None, pair_cap=128, check_every=8, device=None, _backend=None):
    """Steepest descent over swaps of adjacent critical operations, every env of a batch at once.  ``env_or_instances``: an
    instance (a name, a path, an ``Instance``) or a list of them -- one env each, reset and rolled out with the rule ``kind``
    -- or a ``BatchedJssEnv``: one that was never reset is reset and rolled out, one whose envs are all done is taken as it is.

    The rank starts as the solution (start times order every machine).  An iteration is three launches and nothing else:
    ``jss_order_eval`` of the B rows with the pairs out; ``jss_order_eval`` of the B * ``pair_cap`` candidates, candidate
    (i, k) being env i's row with the ranks of its k-th pair exchanged in the kernel; ``jss_order_apply``, which takes each env's
    lowest (makespan, k) if that is lower than the env's current makespan.  Every ``check_every`` iterations the driver reads
    the window's ``improved`` flags and stops after the first iteration in which no env improved (or after ``max_iter``);
    iterations run past that one change nothing, so the result does not depend on ``check_every``.  No acceptance of equal or
    worse neighbours, no tabu list, no restarts: the schedule ends in a local optimum of this neighbourhood."""
    cap, check_every = int(pair_cap), int(check_every)
    if cap < 1 or check_every < 1:
        raise ValueError("improve: pair_cap and check_every must be >= 1")
    if isinstance(env_or_instances, BatchedJssEnv):
        env = env_or_instances
        fresh = not env._is_reset
    elif isinstance(env_or_instances, PackedBatch) or type(env_or_instances).__name__ in ("BucketedJssEnv", "JssVectorEnv", "JssEnv"):
        raise NotImplementedError("improve takes instances or a BatchedJssEnv")
    else:
        one = isinstance(env_or_instances, (str, os.PathLike, Instance))
        names = [env_or_instances] if one else list(env_or_instances)
        if not names:
            raise ValueError("improve: need at least one instance")
        env = _grouped_env(names, 1, 0, device, _backend)
        fresh = True
    be = env.backend
    if fresh:
        env.reset()
        env.rollout(kind, n_iter=3 * env.jmax * env.mmax, autoreset=False)
    elif not (np.asarray(be.numpy(env.done)) != 0).all():
        raise ValueError("improve: the batch is neither fresh nor done -- finish its episodes first")
    lib = order_library(be)
    B, region = env.batch, env.jmax * env.mmax
    p = be.ptr
    with be.on_device():
        rank = env.solution.clone() if hasattr(env.solution, "clone") else np.array(env.solution, copy=True)
        cur = env.evaluate_order(rank)
        before = np.asarray(be.numpy(cur)).astype(np.int32)
        cand_parent = be.from_numpy(np.repeat(np.arange(B, dtype=np.int32), cap))
        pa, pb = be.zeros((B, cap), "int32"), be.zeros((B, cap), "int32")
        cand_mk = be.zeros((B * cap,), "int32")
        win_mk, win_pairs, win_improved = (be.zeros((check_every, B), "int32") for _ in range(3))
        rows = _abi.JssOrder(B, cap, p(rank), None, None, None, None, None, None, p(pa), p(pb), None)
        cands = _abi.JssOrder(B * cap, 0, p(rank), p(cand_parent), p(pa), p(pb), p(cand_mk), None, None, None, None, None)
        apply = _abi.JssOrderApply(B, env.jmax, env.mmax, cap, p(rank), p(cur), p(cand_mk), p(pa), p(pb), None)
        desc, state, stream = C.byref(env._desc), C.byref(env._state), be.stream()
        history, iterations, evaluations, truncated, ran, finished = [], 0, 0, 0, 0, False
        while not finished and (max_iter is None or ran < int(max_iter)):
            n_win = check_every if max_iter is None else min(check_every, int(max_iter) - ran)
            for i in range(n_win):
                rows.makespan, rows.n_pairs, apply.improved = p(win_mk[i]), p(win_pairs[i]), p(win_improved[i])
                for rc, what in ((lib.jss_order_eval(desc, state, C.byref(rows), stream), "jss_order_eval"),
                                 (lib.jss_order_eval(desc, state, C.byref(cands), stream), "jss_order_eval"),
                                 (lib.jss_order_apply(C.byref(apply), stream), "jss_order_apply")):
                    if rc:
                        _abi.check(be.lib, rc, what)
            improved = np.asarray(be.numpy(win_improved))[:n_win]       # the one host round trip of the window
            idle = np.flatnonzero(~(improved != 0).any(axis=1))
            used = int(idle[0]) + 1 if idle.size else n_win          # up to and including the iteration that improved nothing
            finished = bool(idle.size)
            pairs = np.asarray(be.numpy(win_pairs))[:used].astype(np.int64)
            history.append(np.asarray(be.numpy(win_mk))[:used].copy())
            iterations += used - (1 if finished else 0)
            evaluations += int(np.minimum(np.maximum(pairs, 0), cap).sum())
            truncated += int((pairs > cap).sum())
            ran += used
        makespan, start = env.evaluate_order(rank, start=True)
        res = ImproveResult(makespan_before=before, makespan=np.asarray(be.numpy(makespan)).astype(np.int32),
                            rank=np.asarray(be.numpy(rank)).copy(), start=np.asarray(be.numpy(start)).copy(), iterations=iterations,
                            evaluations=evaluations, truncated=truncated,
                            history=np.concatenate(history) if history else np.zeros((0, B), np.int32), env=env)
    return res


# ---- tabu search over swaps of adjacent critical operations (include/jss_tabu.h) ---------------------------------------------------
def tabu_reference(env_const, ops, rank, iters, tenure, target=None, fill=-1, log=None):
    """include/jss_tabu.h's jss_tabu_search on host arrays, written from the header's definition on top of
    ``order_eval_reference``, one walker after the other: the start's refusal, cycle and order, every move's pairs and every
    neighbour's makespan are calls of that mirror.  ``env_const`` (B, 12), ``ops`` (n_tables, jmax, mmax), ``rank``
    (B, jmax, mmax); ``tenure`` an int or (B,); ``target`` None, an int or (B,).  Returns ``(best_makespan, best_rank,
    last_rank, info, trace)``: int32 (B,), (B, jmax, mmax) twice, (B, 4), (B, iters).  The rows of refused (-1) and cyclic (-2)
    walkers hold ``fill`` in both ranks and in the trace.  ``log``: a list that receives ``(walker, move, "aspired" | "forced")``
    for every move that took a tabu neighbour: by aspiration, or because no neighbour was admissible."""
    rank = np.asarray(rank, dtype=np.int64)
    B, jmax, mmax = rank.shape
    region, iters = jmax * mmax, int(iters)
    const = np.asarray(env_const, dtype=np.int64).reshape(B, _abi.NC)
    ops = np.asarray(ops, dtype=np.int64).reshape(-1, jmax, mmax)
    tenure = np.broadcast_to(np.asarray(tenure, dtype=np.int64), (B,))
    target = None if target is None else np.broadcast_to(np.asarray(target, dtype=np.int64), (B,))
    best_mk = np.full(B, -1, np.int32)
    best_rank = np.full((B, jmax, mmax), fill, np.int32)
    last_rank = np.full((B, jmax, mmax), fill, np.int32)
    info = np.zeros((B, _abi.TABU_NI), np.int32)
    trace = np.full((B, iters), fill, np.int32)
    first = order_eval_reference(const, ops, rank)[0]
    for i in range(B):
        L = int(tenure[i])
        if first[i] < 0 or not 0 <= L <= _abi.TABU_MAX_TENURE:
            best_mk[i] = info[i, 0] = -1 if first[i] == -1 or not 0 <= L <= _abi.TABU_MAX_TENURE else -2
            continue
        J, M, tab = (int(x) for x in const[i, [_abi.C_JOBS, _abi.C_MACHINES, _abi.C_TABLE]])
        one = const[i:i + 1]
        mach = (ops[tab].reshape(-1) >> 16) & 63
        real = np.zeros((jmax, mmax), bool)
        real[:J, :M] = True
        real_ops = np.flatnonzero(real.reshape(-1))
        pos = np.full(region, -1, np.int64)                          # the order as positions: the operation's index on its machine
        row = rank[i].reshape(-1)
        for m in range(_abi.MAX_MACHINES):
            on = real_ops[mach[real_ops] == m]
            pos[on[np.lexsort((on, row[on]))]] = np.arange(on.size)
        cur = best = int(first[i])
        best_pos = pos.copy()
        moves = best_move = evaluations = stop = 0
        taken = []                                                    # (pair, move number) of every move
        if target is not None and best <= target[i]:
            stop = 2
        for t in range(1, iters + 1):
            if stop:
                break
            now = pos.reshape(1, jmax, mmax)
            _, _, _, pa, pb, found = order_eval_reference(one, ops, now, pair_cap=region)
            n = int(found[0])
            evaluations += n
            mk = order_eval_reference(one, ops, now, np.zeros(n, np.int64), pa[0, :n], pb[0, :n])[0] if n else np.zeros(0, np.int32)
            usable = [k for k in range(n) if mk[k] >= 0]
            if not usable:
                stop = 1
                break
            pairs = [frozenset((int(pa[0, k]), int(pb[0, k]))) for k in range(n)]
            recent = [max([s for pair, s in taken if pair == pairs[k] and s >= t - L], default=0) for k in range(n)]
            admissible = [k for k in usable if recent[k] == 0 or mk[k] < best]
            if admissible:
                k = min(admissible, key=lambda k: (int(mk[k]), k))
            else:
                k = min(usable, key=lambda k: recent[k])
            if log is not None and recent[k]:
                log.append((i, t, "aspired" if admissible else "forced"))
            a, b = int(pa[0, k]), int(pb[0, k])
            pos[a], pos[b] = pos[b], pos[a]
            cur = int(mk[k])
            taken.append((pairs[k], t))
            moves = t
            trace[i, t - 1] = cur
            if cur < best:
                best, best_pos, best_move = cur, pos.copy(), t
            if target is not None and best <= target[i]:
                stop = 2
        best_mk[i] = best
        best_rank[i], last_rank[i] = best_pos.reshape(jmax, mmax), pos.reshape(jmax, mmax)
        trace[i, moves:] = -1
        info[i] = (stop, moves, best_move, evaluations)
    return best_mk, best_rank, last_rank, info, trace


# ---- tabu search over block insertions, scored by heads and tails (include/jss_block.h) -----------------------------------------
def block_reference(env_const, ops, rank, iters, tenure, target=None, reach=0, fill=-1, log=None):
    """include/jss_block.h's jss_block_search on host arrays, written from the header's definition on top of
    ``order_eval_reference``, one walker after the other: the start's refusal, cycle and order, every move's starts and tails and
    the re-timing of the move taken are calls of that mirror; blocks, candidates, screen, estimate and choice are written out
    here.  Arguments as ``tabu_reference``'s, and ``reach``.  Returns ``(best_makespan, best_rank, last_rank, info, trace,
    move_log)``: int32 (B,), (B, jmax, mmax) twice, (B, 8), (B, iters), (B, iters, 2).  The rows of refused (-1) and cyclic (-2)
    walkers hold ``fill`` in both ranks, the trace and the move log.  ``log``: a list that receives ``(walker, move, event)``:
    "F far" / "B far" for a move of distance >= 2 taken, "aspired" / "forced" for a tabu move taken, "job" / "successor" /
    "predecessor" for a screened candidate (the first of the header's three conditions that holds), "reach" for a candidate that
    ``reach`` cut."""
    rank = np.asarray(rank, dtype=np.int64)
    B, jmax, mmax = rank.shape
    region, iters, reach = jmax * mmax, int(iters), int(reach)
    const = np.asarray(env_const, dtype=np.int64).reshape(B, _abi.NC)
    ops = np.asarray(ops, dtype=np.int64).reshape(-1, jmax, mmax)
    tenure = np.broadcast_to(np.asarray(tenure, dtype=np.int64), (B,))
    target = None if target is None else np.broadcast_to(np.asarray(target, dtype=np.int64), (B,))
    best_mk = np.full(B, -1, np.int32)
    best_rank = np.full((B, jmax, mmax), fill, np.int32)
    last_rank = np.full((B, jmax, mmax), fill, np.int32)
    info = np.zeros((B, _abi.BLOCK_NI), np.int32)
    trace = np.full((B, iters), fill, np.int32)
    move_log = np.full((B, iters, 2), fill, np.int32)
    note = (lambda *event: log.append(event)) if log is not None else (lambda *event: None)
    first = order_eval_reference(const, ops, rank)[0]
    for i in range(B):
        L = int(tenure[i])
        if first[i] < 0 or not 0 <= L <= _abi.TABU_MAX_TENURE:
            best_mk[i] = info[i, 0] = -1 if first[i] == -1 or not 0 <= L <= _abi.TABU_MAX_TENURE else -2
            continue
        J, M, tab = (int(x) for x in const[i, [_abi.C_JOBS, _abi.C_MACHINES, _abi.C_TABLE]])
        one = const[i:i + 1]
        mach = (ops[tab].reshape(-1) >> 16) & 63
        dur = ops[tab].reshape(-1) & 0xFFFF
        real = np.zeros((jmax, mmax), bool)
        real[:J, :M] = True
        real_ops = np.flatnonzero(real.reshape(-1))
        pos = np.full(region, -1, np.int64)                          # the order as positions: the operation's index on its machine
        row = rank[i].reshape(-1)
        for m in range(_abi.MAX_MACHINES):
            on = real_ops[mach[real_ops] == m]
            pos[on[np.lexsort((on, row[on]))]] = np.arange(on.size)
        cur = best = int(first[i])
        best_pos = pos.copy()
        moves = best_move = evaluations = screened = far = hits = stop = 0
        taken = []                                                    # (pair, move number) of every move
        if target is not None and best <= target[i]:
            stop = 2
        for t in range(1, iters + 1):
            if stop:
                break
            _, st, tl = order_eval_reference(one, ops, pos.reshape(1, jmax, mmax))[:3]
            st, tl = st[0].reshape(-1).astype(np.int64), tl[0].reshape(-1).astype(np.int64)
            E = lambda e: int(st[e] + dur[e]) if e >= 0 else 0       # noqa: E731  (a missing neighbour contributes 0)
            Q = lambda e: int(dur[e] + tl[e]) if e >= 0 else 0       # noqa: E731
            JP = lambda e: e - 1 if e % mmax > 0 else -1             # noqa: E731
            JS = lambda e: e + 1 if e % mmax + 1 < M else -1         # noqa: E731
            critical = st + dur + tl == cur
            marks = 0
            listed = []                                               # (estimate, x, y, the machine's new order, distance, kind)
            for m in range(_abi.MAX_MACHINES):
                on = real_ops[mach[real_ops] == m]
                on = [int(e) for e in on[np.argsort(pos[on])]]
                at_m = lambda a: on[a] if 0 <= a < len(on) else -1   # noqa: E731
                marked = [a for a in range(len(on) - 1) if on[a] // mmax != on[a + 1] // mmax and critical[on[a]]
                          and critical[on[a + 1]] and st[on[a + 1]] == st[on[a]] + dur[on[a]]]
                marks += len(marked)
                for at in marked:
                    p0 = pL = at                                      # the block's marked positions are p0 ... pL - 1
                    while p0 - 1 in marked:
                        p0 -= 1
                    while pL in marked:
                        pL += 1
                    cands = [("F", on[at], on[pL], on[at + 1:pL + 1], pL - at, at_m(at - 1), at_m(pL + 1))]
                    if pL - p0 >= 2:
                        cands.append(("B", on[at + 1], on[p0], on[p0:at + 1], at + 1 - p0, at_m(p0 - 1), at_m(at + 2)))
                    for kind, x, y, jumped, dist, before, behind in cands:
                        if reach > 0 and dist > reach:
                            note(i, t, "reach")
                            continue
                        if any(w // mmax == x // mmax for w in jumped):
                            screened += 1
                            note(i, t, "job")
                            continue
                        if kind == "F" and JS(x) >= 0 and not Q(y) > tl[JS(x)]:
                            screened += 1
                            note(i, t, "successor")
                            continue
                        if kind == "B" and JP(x) >= 0 and not E(y) > st[JP(x)]:
                            screened += 1
                            note(i, t, "predecessor")
                            continue
                        evaluations += 1
                        order = jumped + [x] if kind == "F" else [x] + jumped
                        head, h = E(before), {}
                        for e in order:
                            h[e] = max(E(JP(e)), head)
                            head = h[e] + int(dur[e])
                        tail, est = Q(behind), 0
                        for e in reversed(order):
                            tail = int(dur[e]) + max(Q(JS(e)), tail)
                            est = max(est, h[e] + tail)
                        listed.append((est, x, y, jumped, dist, kind))
            if not marks:
                stop = 1
                break
            if not listed:
                stop = 3
                break
            pairs = [frozenset((c[1], c[2])) for c in listed]
            recent = [max([s for pair, s in taken if pair == pairs[k] and s >= t - L], default=0) for k in range(len(listed))]
            admissible = [k for k in range(len(listed)) if recent[k] == 0 or listed[k][0] < best]
            if admissible:
                k = min(admissible, key=lambda k: (listed[k][0], k))
            else:
                k = min(range(len(listed)), key=lambda k: (recent[k], k))
            est, x, y, jumped, dist, kind = listed[k]
            old = pos.copy()
            if kind == "F":
                pos[x] = old[y]
                pos[jumped] = old[jumped] - 1
            else:
                pos[x] = old[y]
                pos[jumped] = old[jumped] + 1
            mk = int(order_eval_reference(one, ops, pos.reshape(1, jmax, mmax))[0][0])
            if mk < 0:                                                # (the screen makes this unreachable)
                pos = old
                stop = 4
                break
            if recent[k]:
                note(i, t, "aspired" if admissible else "forced")
            if dist >= 2:
                far += 1
                note(i, t, kind + " far")
            hits += int(est == mk)
            cur = mk
            taken.append((pairs[k], t))
            moves = t
            trace[i, t - 1] = cur
            move_log[i, t - 1] = (x, y)
            if cur < best:
                best, best_pos, best_move = cur, pos.copy(), t
            if target is not None and best <= target[i]:
                stop = 2
        best_mk[i] = best
        best_rank[i], last_rank[i] = best_pos.reshape(jmax, mmax), pos.reshape(jmax, mmax)
        trace[i, moves:] = -1
        move_log[i, moves:] = -1
        info[i] = (stop, moves, best_move, evaluations, screened, far, hits, 0)
    return best_mk, best_rank, last_rank, info, trace, move_log


# ---- path relinking between machine orders (include/jss_relink.h) ----------------------------------------------------------------
def relink_reference(env_const, ops, rank, guide, steps, until, margin=0, fill=-1, log=None):
    """include/jss_relink.h's jss_relink_walk on host arrays, written from the header's definition on top of
    ``order_eval_reference``, one walker after the other: the refusal and the cycle check of both rows, every move's starts and
    tails and every re-timing are calls of that mirror; the orders, the distance, candidates, screen, estimate, choice and
    fallback are written out here.  ``rank``, ``guide`` (B, jmax, mmax); ``until`` an int or (B,); ``margin`` an int.  Returns
    ``(best_makespan, best_rank, last_makespan, last_rank, info, trace, move_log)``: int32 (B,), (B, jmax, mmax), (B,),
    (B, jmax, mmax), (B, 8), (B, steps), (B, steps, 2).  The rows of refused (-1) and cyclic (-2) walkers hold ``fill`` in both
    ranks, the trace and the move log.  ``log``: a list that receives ``(walker, move, event)``: "unsure" for a candidate the
    screen did not pass, "fallback" for a move without a sure candidate, "retry" for a candidate the fallback swapped back."""
    rank = np.asarray(rank, dtype=np.int64)
    guide = np.asarray(guide, dtype=np.int64)
    B, jmax, mmax = rank.shape
    region, steps, margin = jmax * mmax, int(steps), int(margin)
    const = np.asarray(env_const, dtype=np.int64).reshape(B, _abi.NC)
    ops = np.asarray(ops, dtype=np.int64).reshape(-1, jmax, mmax)
    until = np.broadcast_to(np.asarray(until, dtype=np.int64), (B,))
    best_mk = np.full(B, -1, np.int32)
    last_mk = np.full(B, -1, np.int32)
    best_rank = np.full((B, jmax, mmax), fill, np.int32)
    last_rank = np.full((B, jmax, mmax), fill, np.int32)
    info = np.zeros((B, _abi.RELINK_NI), np.int32)
    trace = np.full((B, steps), fill, np.int32)
    move_log = np.full((B, steps, 2), fill, np.int32)
    note = (lambda *event: log.append(event)) if log is not None else (lambda *event: None)
    of_source = order_eval_reference(const, ops, rank)[0]
    of_guide = order_eval_reference(const, ops, guide)[0]
    for i in range(B):
        if of_source[i] == -1 or of_guide[i] == -1 or until[i] < 0:
            best_mk[i] = last_mk[i] = info[i, 0] = -1
            continue
        if of_source[i] == -2 or of_guide[i] == -2:
            best_mk[i] = last_mk[i] = info[i, 0] = -2
            continue
        J, M, tab = (int(x) for x in const[i, [_abi.C_JOBS, _abi.C_MACHINES, _abi.C_TABLE]])
        one = const[i:i + 1]
        mach = (ops[tab].reshape(-1) >> 16) & 63
        dur = ops[tab].reshape(-1) & 0xFFFF
        real = np.zeros((jmax, mmax), bool)
        real[:J, :M] = True
        real_ops = np.flatnonzero(real.reshape(-1))
        machines = [real_ops[mach[real_ops] == m] for m in range(_abi.MAX_MACHINES)]

        def positions(row):                                           # a rank row as positions on the machines
            out = np.full(region, -1, np.int64)
            for on in machines:
                out[on[np.lexsort((on, row[on]))]] = np.arange(on.size)
            return out

        pos, g = positions(rank[i].reshape(-1)), positions(guide[i].reshape(-1))
        dist = 0
        for on in machines:
            for a in on:
                dist += int(((pos[on] > pos[a]) & (g[on] < g[a])).sum())
        dist0 = dist
        cur = int(of_source[i])
        moves = candidates = fallbacks = retries = 0
        best, best_move, best_pos = None, -1, None
        if 0 >= margin and dist >= margin:
            best, best_move, best_pos = cur, 0, pos.copy()
        stops = lambda: 1 if dist == 0 else 2 if dist <= until[i] else 0   # noqa: E731
        stop = stops()
        for t in range(1, steps + 1):
            if stop:
                break
            _, st, tl = order_eval_reference(one, ops, pos.reshape(1, jmax, mmax))[:3]
            st, tl = st[0].reshape(-1).astype(np.int64), tl[0].reshape(-1).astype(np.int64)
            E = lambda e: int(st[e] + dur[e]) if e >= 0 else 0       # noqa: E731  (a missing neighbour contributes 0)
            Q = lambda e: int(dur[e] + tl[e]) if e >= 0 else 0       # noqa: E731
            JP = lambda e: e - 1 if e % mmax > 0 else -1             # noqa: E731
            JS = lambda e: e + 1 if e % mmax + 1 < M else -1         # noqa: E731
            listed = []                                               # (estimate, listing index, u, v, sure)
            for on in machines:
                on = [int(e) for e in on[np.argsort(pos[on])]]
                at_m = lambda a: on[a] if 0 <= a < len(on) else -1   # noqa: E731
                for at in range(len(on) - 1):
                    u, v = on[at], on[at + 1]
                    if not g[u] > g[v]:
                        continue
                    s, p = JS(u), JP(v)
                    sure = s < 0 or p < 0 or (s != p and st[p] < st[s] + dur[s])
                    hv = max(E(p), E(at_m(at - 1)))
                    hu = max(E(JP(u)), hv + int(dur[v]))
                    tu = int(dur[u]) + max(Q(s), Q(at_m(at + 2)))
                    tv = int(dur[v]) + max(Q(JS(v)), tu)
                    if not sure:
                        note(i, t, "unsure")
                    listed.append((max(hv + tv, hu + tu), len(listed), u, v, sure))
            candidates += len(listed)

            def swapped(u, v):
                out = pos.copy()
                out[u], out[v] = pos[v], pos[u]
                return out, int(order_eval_reference(one, ops, out.reshape(1, jmax, mmax))[0][0])

            taken = None
            sure = [c for c in listed if c[4]]
            if sure:
                _, _, u, v, _ = min(sure)
                new, mk = swapped(u, v)
                if mk >= 0:
                    taken = (u, v, new, mk)
            else:
                fallbacks += 1
                note(i, t, "fallback")
                for _, _, u, v, _ in sorted(listed):
                    new, mk = swapped(u, v)
                    if mk >= 0:
                        taken = (u, v, new, mk)
                        break
                    retries += 1
                    note(i, t, "retry")
            if taken is None:                                         # (the header says why this is unreachable)
                stop = 4
                break
            u, v, pos, cur = taken
            moves, dist = t, dist - 1
            trace[i, t - 1] = cur
            move_log[i, t - 1] = (u, v)
            if t >= margin and dist >= margin and (best is None or cur < best):
                best, best_move, best_pos = cur, t, pos.copy()
            stop = stops()
        if best is None:
            best, best_pos = cur, pos
        best_mk[i], last_mk[i] = best, cur
        best_rank[i], last_rank[i] = best_pos.reshape(jmax, mmax), pos.reshape(jmax, mmax)
        trace[i, moves:] = -1
        move_log[i, moves:] = -1
        info[i] = (stop, moves, best_move, dist0, dist, candidates, fallbacks, retries)
    return best_mk, best_rank, last_mk, last_rank, info, trace, move_log


@dataclass
class TabuResult:
    """What ``tabu_search`` returns, host arrays.  Per instance: ``makespan`` (G,), the lowest ``(best_makespan, walker)`` of its
    group; ``walker`` (G,), that walker's index within the group; ``rank`` (G, jmax, mmax), its best order as positions; ``start``
    (G, jmax, mmax), that order's start times; ``optimal`` (G,): the makespan is proven optimal (it reached the target, a lower
    bound, or the walk found no critical machine arc).  ``best_makespan`` (S,) and ``info`` (S, 4; S, 8 with ``moves="block"``) are the whole batch's,
    ``target`` (S,) what the walks were given (None: nothing), ``tenure`` (S,) their tenures, ``env`` the batch."""
    makespan: np.ndarray
    walker: np.ndarray
    rank: np.ndarray
    start: np.ndarray
    optimal: np.ndarray
    best_makespan: np.ndarray
    info: np.ndarray
    target: Optional[np.ndarray] = None
    tenure: Optional[np.ndarray] = None
    env: Optional[BatchedJssEnv] = None


def tabu_search(instances, kind="SPT", walkers=64, iters=1000, tenure=(5, 12), explore=0.1, seed=0, target="lower_bound",
                device=None, _backend=None, moves="swap", reach=0):
    """Tabu search on one instance or on a list of them: one group of ``walkers`` envs per instance, all in one batch (laid out
    like ``beam_search``'s groups), every walker's whole walk in ONE launch (``BatchedJssEnv.tabu``, include/jss_tabu.h).

    The batch is reset and rolled out with the rule ``kind`` (``explore``: the share of random moves, so that the walkers of a
    group start from different schedules); walker w of a group walks with tenure ``lo + w % (hi - lo + 1)`` for
    ``tenure=(lo, hi)`` (an int: that tenure for all) for at most ``iters`` moves.  ``target="lower_bound"`` stops a walker
    that reaches ``env.lower_bound()`` of the reset state -- a proof of optimality; ``"one_machine"`` takes
    ``env.relax_machines()[0]`` instead, the stronger one-machine bound of the empty selection (include/jss_machine.h), and
    ``"one_machine_exact"`` ``env.solve_machines()[0]``, that bound with the one-machine problems solved (include/jss_carlier.h); ``None``
    gives no target, an int or one int per instance that target.  The result is defined by those public calls alone: ``reset``, ``lower_bound``, ``rollout``,
    one ``tabu``, one ``evaluate_order``.

    ``moves="block"`` walks over block insertions instead (``BatchedJssEnv.tabu_blocks``, include/jss_block.h: candidates scored
    by head and tail estimates, one exact re-timing per move), ``reach`` its largest distance (0: no limit); the one ``tabu`` of
    the definition is then one ``tabu_blocks``, ``info`` has its 8 columns, and stop 1 alone still proves optimality."""
    W = int(walkers)
    if W < 1:
        raise ValueError("tabu_search: walkers must be >= 1")
    if moves not in ("swap", "block"):
        raise ValueError("tabu_search: moves is 'swap' or 'block'")
    reach = int(reach)
    if not 0 <= reach <= _abi.BLOCK_MAX_REACH or (reach and moves == "swap"):
        raise ValueError(f"tabu_search: reach must lie in [0, {_abi.BLOCK_MAX_REACH}], and is 0 with moves='swap'")
    names, G = _instance_groups("tabu_search", instances, "call tabu on a BatchedJssEnv for anything else")
    lo, hi = (int(tenure), int(tenure)) if np.ndim(tenure) == 0 else (int(tenure[0]), int(tenure[1]))
    if not 0 <= lo <= hi <= _abi.TABU_MAX_TENURE:
        raise ValueError(f"tabu_search: tenure must lie in [0, {_abi.TABU_MAX_TENURE}], low <= high")
    S = G * W
    env = _grouped_env(names, W, seed, device, _backend)
    be = env.backend
    env.reset()
    tgt = _resolve_target("tabu_search", env, target, G, W)
    env.rollout(kind, n_iter=3 * env.jmax * env.mmax, autoreset=False, explore=explore, seed=seed)
    ten = (lo + (np.arange(S) % W) % (hi - lo + 1)).astype(np.int32)
    if moves == "block":
        best, best_rank, info = env.tabu_blocks(None, iters, ten, tgt, reach)
    else:
        best, best_rank, info = env.tabu(None, iters, ten, tgt)
    host = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    mk, info = host(best).astype(np.int32), host(info).astype(np.int32)
    tgt = None if tgt is None else host(tgt).astype(np.int32)
    walker, winner = _group_winners(mk, G, W)
    again, start = env.evaluate_order(best_rank, winner, start=True)
    assert np.array_equal(host(again), mk[winner])
    proven = info[:, 0] == 1
    if tgt is not None:
        proven |= (mk >= 0) & (mk <= tgt)
    return TabuResult(makespan=mk[winner], walker=walker, rank=host(best_rank)[winner].copy(), start=host(start).copy(),
                      optimal=proven[winner], best_makespan=mk, info=info, target=tgt, tenure=ten, env=env)


@dataclass
class RelinkResult(TabuResult):
    """What ``relink_search`` returns: ``TabuResult``'s fields -- ``best_makespan`` (S,) the walkers' bests over all stages,
    ``info`` (S, 8) that of the block walk that gave a walker its best -- and ``history`` (G, rounds + 1), the group's best
    after the first walk and after every round, and ``distance`` (S, rounds), every walker's distance to its group's elite
    order at the start of every round."""
    history: Optional[np.ndarray] = None
    distance: Optional[np.ndarray] = None


def relink_search(instances, kind="SPT", walkers=64, iters=1000, rounds=4, share=(1, 2), tenure=(5, 12), explore=0.1, seed=0,
                  target="lower_bound", reach=0, device=None, _backend=None):
    """Block-insertion tabu walks whose walkers learn from their group's best one (after Nowicki and Smutnicki's i-TSAB): one group
    of ``walkers`` envs per instance, all in one batch, as ``tabu_search`` lays them out.  Defined by public calls alone:

    start   exactly ``tabu_search(moves="block")``'s: the batch, ``reset``, the target, ``rollout(kind, explore, seed)``, the
            tenures, and one ``tabu_blocks(None, iters, tenures, target, reach)``: ``best`` and ``best_rank`` per walker.
    round   (``rounds`` of them) the elite of a group is its walker with the lowest ``(best, walker)``; every walker's guide is
            its group's elite order, gathered on the device; ``d = order_distance(best_rank, guide)``;
            ``relink(best_rank, guide, until=d - d * share[0] // share[1])`` walks that share of the way towards the elite (a
            walker that is already at its target gets ``until = d`` and stays put; the elite has distance 0 and simply walks on
            from its best order); ``tabu_blocks(last_rank, iters, tenures, target, reach)`` walks on from where the relinking
            ended; a walker keeps the lower of its old and its new best, the old one on a tie, with its order and that walk's
            ``info`` (a ``where`` on the device).  Nothing comes back to the host inside a round.
    end     as ``tabu_search``: the lowest ``(best, walker)`` of every group, one ``evaluate_order`` for its start times.

    ``rounds=0`` returns what ``tabu_search(moves="block")`` returns, in the fields they share.  Returns a ``RelinkResult``."""
    W, rounds, reach = int(walkers), int(rounds), int(reach)
    if W < 1:
        raise ValueError("relink_search: walkers must be >= 1")
    if rounds < 0:
        raise ValueError("relink_search: rounds must be >= 0")
    num, den = (int(x) for x in share)
    if not (den >= 1 and 0 <= num <= den):
        raise ValueError("relink_search: share is (a, b) with 0 <= a <= b and b >= 1")
    if not 0 <= reach <= _abi.BLOCK_MAX_REACH:
        raise ValueError(f"relink_search: reach must lie in [0, {_abi.BLOCK_MAX_REACH}]")
    names, G = _instance_groups("relink_search", instances, "call relink and tabu_blocks on a BatchedJssEnv for anything else")
    lo, hi = (int(tenure), int(tenure)) if np.ndim(tenure) == 0 else (int(tenure[0]), int(tenure[1]))
    if not 0 <= lo <= hi <= _abi.TABU_MAX_TENURE:
        raise ValueError(f"relink_search: tenure must lie in [0, {_abi.TABU_MAX_TENURE}], low <= high")
    S = G * W
    env = _grouped_env(names, W, seed, device, _backend)
    be = env.backend
    env.reset()
    tgt = _resolve_target("relink_search", env, target, G, W)
    env.rollout(kind, n_iter=3 * env.jmax * env.mmax, autoreset=False, explore=explore, seed=seed)
    ten = (lo + (np.arange(S) % W) % (hi - lo + 1)).astype(np.int32)
    best, best_rank, info = env.tabu_blocks(None, iters, ten, tgt, reach)
    xp = be.torch if getattr(be, "torch", None) is not None else np
    with be.on_device():
        on = lambda x, dtype: be.from_numpy(np.asarray(x, dtype))   # noqa: E731
        first = on(np.arange(G) * W, np.int64)                       # the groups' first walkers
        group = on(np.repeat(np.arange(G), W), np.int64)             # every walker's group
        ten_dev = on(ten, np.int32)
        tgt_dev = None if tgt is None else on(tgt, np.int32) if isinstance(tgt, np.ndarray) else tgt
        never = 2 ** 31 - 1

        def group_low(mk):                                           # (G, W): a walker without a schedule counts as +inf
            return xp.where(mk >= 0, mk, never).reshape(G, W)

        history, distance = [group_low(best).min(1) if xp is np else group_low(best).min(1).values], []
        for _ in range(rounds):
            elite = first + group_low(best).argmin(1)                # (the first of equal makespans)
            guide = best_rank[elite[group]]
            d = env.order_distance(best_rank, guide)
            until = d - d * num // den
            if tgt_dev is not None:
                until = xp.where((best >= 0) & (best <= tgt_dev), d, until)
            last_rank = env.relink(best_rank, guide, None, until)[3]
            new, new_rank, new_info = env.tabu_blocks(last_rank, iters, ten_dev, tgt_dev, reach)
            keep = (new >= 0) & ((best < 0) | (new < best))
            best = xp.where(keep, new, best)
            best_rank = xp.where(keep[:, None, None], new_rank, best_rank)
            info = xp.where(keep[:, None], new_info, info)
            history.append(group_low(best).min(1) if xp is np else group_low(best).min(1).values)
            distance.append(d)
    host = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    mk, info = host(best).astype(np.int32), host(info).astype(np.int32)
    tgt = None if tgt is None else host(tgt).astype(np.int32)
    walker, winner = _group_winners(mk, G, W)
    again, start = env.evaluate_order(best_rank, winner, start=True)
    assert np.array_equal(host(again), mk[winner])
    proven = info[:, 0] == 1
    if tgt is not None:
        proven |= (mk >= 0) & (mk <= tgt)
    return RelinkResult(makespan=mk[winner], walker=walker, rank=host(best_rank)[winner].copy(), start=host(start).copy(),
                        optimal=proven[winner], best_makespan=mk, info=info, target=tgt, tenure=ten, env=env,
                        history=np.stack([host(h) for h in history], axis=1).astype(np.int32),
                        distance=np.stack([host(x) for x in distance], axis=1).astype(np.int32).reshape(S, rounds) if rounds
                        else np.zeros((S, 0), np.int32))


# ---- Giffler-Thompson decoding of key tables, one BRKGA generation (include/jss_decode.h) ------------------------------------------
def decode_reference(env_const, ops, keys, parents=None, delta=65536, fill=-1):
    """include/jss_decode.h's jss_decode_keys on host arrays, written from the header's definition, one candidate after the
    other.  ``keys`` (jmax, mmax), one table for all, or (n, jmax, mmax); ``parents`` (n,) or None (candidate c is env c);
    ``delta`` in units of 1 / 65536, an int or (n,).  Returns ``(makespan, start, info)``: int32 (n,), (n, jmax, mmax), (n, 4).  The
    rows of refused candidates (-1) hold ``fill`` in start and info."""
    const = np.asarray(env_const, dtype=np.int64).reshape(-1, _abi.NC)
    B = const.shape[0]
    keys = np.asarray(keys, dtype=np.int64)
    jmax, mmax = keys.shape[-2:]
    ops = np.asarray(ops, dtype=np.int64).reshape(-1, jmax, mmax)
    n = len(parents) if parents is not None else keys.shape[0] if keys.ndim == 3 else B
    parents = np.arange(n) if parents is None else np.asarray(parents, dtype=np.int64)
    delta = np.broadcast_to(np.asarray(delta, dtype=np.int64), (n,))
    makespan = np.full(n, -1, np.int32)
    start = np.full((n, jmax, mmax), fill, np.int32)
    info = np.full((n, _abi.DECODE_NI), fill, np.int32)
    for c in range(n):
        i, dl = int(parents[c]), int(delta[c])
        if not 0 <= i < B or not 0 <= dl <= 65536:
            continue
        J, M, tab = (int(const[i, x]) for x in (_abi.C_JOBS, _abi.C_MACHINES, _abi.C_TABLE))
        if not (1 <= J <= jmax and 1 <= M <= mmax and 0 <= tab < ops.shape[0]):
            continue
        table = keys[c] if keys.ndim == 3 else keys
        mach, dur = ((ops[tab] >> 16) & 63).tolist(), (ops[tab] & 0xFFFF).tolist()
        key = table.tolist()
        k, jobend, rel = [0] * J, [0] * J, [0] * 64
        row = np.full((jmax, mmax), -1, np.int32)
        conflicts = widest = delayed = 0
        for _ in range(J * M):
            live = [j for j in range(J) if k[j] < M]
            est = {j: max(jobend[j], rel[mach[j][k[j]]]) for j in live}
            ect, first = min((est[j] + dur[j][k[j]], j) for j in live)
            m = mach[first][k[first]]
            on_m = [j for j in live if mach[j][k[j]] == m]
            e0 = min(est[j] for j in on_m)
            conflict = [j for j in on_m if est[j] == e0 or (est[j] - e0) * 65536 < dl * (ect - e0)]
            chosen = max(conflict, key=lambda j: (key[j][k[j]], -j))
            conflicts += len(conflict) > 1
            widest = max(widest, len(conflict))
            delayed += est[chosen] > e0
            row[chosen, k[chosen]] = est[chosen]
            jobend[chosen] = rel[m] = est[chosen] + dur[chosen][k[chosen]]
            k[chosen] += 1
        makespan[c], start[c], info[c] = max(jobend), row, (conflicts, widest, delayed, 0)
    return makespan, start, info


_M32 = np.uint64(0xFFFFFFFF)


def _fmix32(x):
    x = x & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    return x ^ (x >> np.uint64(16))


def rng_u32(seed, env_id, episode, step):
    """The counter RNG of the libraries (jss_common.hpp rng_u32, oracle/jss_oracle.c orc_rng_u32), vectorised over ``env_id``,
    ``episode`` and ``step``: uint64 arrays holding 32-bit values."""
    seed = int(seed) & (2 ** 64 - 1)
    env_id = np.asarray(env_id, dtype=np.uint64)
    episode = np.asarray(episode, dtype=np.int64).astype(np.uint64) & _M32
    step = np.asarray(step, dtype=np.int64).astype(np.uint64) & _M32
    a = (np.uint64(seed & 0xFFFFFFFF) + (env_id & _M32) * np.uint64(0x9E3779B9) + episode * np.uint64(0x85EBCA6B)
         + step * np.uint64(0xC2B2AE35)) & _M32
    b = np.uint64(seed >> 32) ^ (((env_id >> np.uint64(32)) * np.uint64(0x27D4EB2F)) & _M32)
    return _fmix32(_fmix32(a) ^ b)


def evolve_reference(keys_in, fitness, groups, pop, n_elite, n_mutant, rho_q16, generation, seed, region=None, rng=rng_u32):
    """include/jss_decode.h's jss_keys_evolve on host arrays, written from the header's definition, one group and one child after
    the other.  ``keys_in`` (G * P, region) and ``fitness`` (G * P,) may be None for an initial population (``n_elite == 0``,
    ``n_mutant == pop``; ``region`` is then needed).  ``rng``: the counter RNG, ``rng(seed, row, generation, x)``.  Returns
    ``(keys_out, by_rank)``: int32 (G * P, region) and (G * P,)."""
    G, P = int(groups), int(pop)
    if keys_in is not None:
        keys_in = np.asarray(keys_in, dtype=np.int32).reshape(G * P, -1)
        region = keys_in.shape[1]
    region = int(region)
    ranked = not (n_elite == 0 and n_mutant == P)
    out = np.zeros((G * P, region), np.int32)
    by_rank = np.zeros(G * P, np.int32)
    key = (int(seed) ^ _abi.EVOLVE_SEED_XOR) & (2 ** 64 - 1)
    entries = np.arange(region)
    for g in range(G):
        order = list(range(P))
        if ranked:
            fit = [int(x) for x in np.asarray(fitness).reshape(G, P)[g]]
            order.sort(key=lambda p: (fit[p] < 0, fit[p], p))
        by_rank[g * P:(g + 1) * P] = order
        for c in range(P):
            i = g * P + c
            if c < n_elite:
                out[i] = keys_in[g * P + order[c]]
                continue
            r = rng(key, i, generation, entries)
            if c >= P - n_mutant:
                out[i] = r.astype(np.uint32).view(np.int32)
                continue
            a = order[int(rng(key, i, generation, region)) % n_elite]
            b = order[n_elite + int(rng(key, i, generation, region + 1)) % (P - n_elite)]
            out[i] = np.where((r >> np.uint64(16)) < np.uint64(rho_q16), keys_in[g * P + a], keys_in[g * P + b])
    return out, by_rank


@dataclass
class BrkgaResult:
    """What ``brkga_search`` returns, host arrays.  Per instance: ``makespan`` (G,); ``keys`` (G, jmax, mmax), the key table of the
    individual that gave it; ``start`` (G, jmax, mmax), the start times of its schedule; ``rank`` (G, jmax, mmax), its machine
    order (the decoded start times, or with ``polish`` the positions the block walk returned); ``history`` (G, generations + 1),
    the group's best decoded makespan of every population; ``generations``, the generations made; ``optimal`` (G,): the makespan
    reached the target, a lower bound; ``env`` the batch of G envs."""
    makespan: np.ndarray
    keys: np.ndarray
    start: np.ndarray
    rank: np.ndarray
    history: np.ndarray
    generations: int
    optimal: np.ndarray
    env: Optional[BatchedJssEnv] = None
    target: Optional[np.ndarray] = None          # (G,), the target the search stopped at; None without one


def brkga_search(instances, population=256, generations=100, elite=0.15, mutants=0.15, rho=0.7, delta=0.5, seed_rules=("SPT", "MWR"),
                 polish=0, tenure=8, seed=0, target="lower_bound", check_every=8, device=None, _backend=None):
    """A biased random-key genetic algorithm over per-operation priority keys, decoded by Giffler and Thompson's procedure, on
    one instance or on a list of them: one group of ``population`` individuals per instance and ONE batch of one env per
    instance, which is only read (``parents = repeat(arange(G), P)``).  Defined by public calls alone:

    start   the batch, ``reset``, the target (``"lower_bound"``: ``env.lower_bound()`` of the reset state; ``"one_machine"``:
            ``env.relax_machines()[0]``, the one-machine bound of the empty selection; ``"one_machine_exact"``:
            ``env.solve_machines()[0]``; None; an int or one per instance); population 0 is ``evolve_keys((G * P, jmax, mmax), None, P, 0, P, generation=0, seed=seed)``, the
            first individuals of every group overwritten by ``dispatching.rule_keys(instance, rule)`` for ``seed_rules`` (padding 0).
    generation t = 1 ...  ``fitness = decode_keys(keys, parents, delta)`` then ``keys = evolve_keys(keys, fitness, P, n_elite,
            n_mutant, rho, generation=t, seed=seed)`` with ``n_elite = max(1, round(elite * P))`` and ``n_mutant = round(mutants *
            P)``.  Nothing is computed by the host and nothing comes to it, but every ``check_every`` generations the
            groups' minima of that window: the search ends once every group is at or below its target, or after ``generations``.
            Elites are copied, so a group's best never rises.
    end     one more ``decode_keys`` of the last population, with its start times.  ``polish == 0``: the result is the lowest
            ``(makespan, individual)`` of every group, ``rank`` its start times.  ``polish > 0``: every individual's start
            times are the rank of one walker of ``tabu_blocks(rank=start, iters=polish, tenure=tenure)`` on a batch of G * P
            envs, and the result is the lowest ``(best_makespan, individual)`` of every group.

    Returns a ``BrkgaResult``."""
    from .dispatching import rule_keys
    P, gens, polish, check_every = int(population), int(generations), int(polish), int(check_every)
    if not 1 <= P <= _abi.EVOLVE_MAX_POP:
        raise ValueError(f"brkga_search: population must lie in [1, {_abi.EVOLVE_MAX_POP}]")
    if gens < 0 or polish < 0 or check_every < 1:
        raise ValueError("brkga_search: generations >= 0, polish >= 0, check_every >= 1")
    if not (0.0 <= float(rho) <= 1.0 and 0.0 <= float(delta) <= 1.0 and 0.0 <= float(elite) <= 1.0 and 0.0 <= float(mutants) <= 1.0):
        raise ValueError("brkga_search: rho, delta, elite and mutants lie in [0, 1]")
    n_elite, n_mutant = max(1, int(round(float(elite) * P))), int(round(float(mutants) * P))
    if n_elite + n_mutant > P:
        raise ValueError("brkga_search: elite + mutants must not exceed the population")
    if not 0 <= int(tenure) <= _abi.TABU_MAX_TENURE:
        raise ValueError(f"brkga_search: tenure must lie in [0, {_abi.TABU_MAX_TENURE}]")
    names, G = _instance_groups("brkga_search", instances, "call decode_keys and evolve_keys on a BatchedJssEnv for anything else")
    rules = tuple(seed_rules or ())
    if len(rules) > P:
        raise ValueError("brkga_search: more seed rules than individuals")
    _check_target("brkga_search", target)
    S = G * P
    env = _grouped_env(names, 1, seed, device, _backend)
    be = env.backend
    env.reset()
    host = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    tgt = _resolve_target("brkga_search", env, target, G, 1)
    tgt = None if tgt is None else host(tgt).astype(np.int32)
    jmax, mmax = env.jmax, env.mmax
    xp = be.torch if getattr(be, "torch", None) is not None else np
    never = 2 ** 31 - 1
    with be.on_device():
        parents = be.from_numpy(np.repeat(np.arange(G), P).astype(np.int32))
        keys, _ = env.evolve_keys((S, jmax, mmax), None, P, 0, P, rho, 0, seed)
        if rules:
            seeds = np.zeros((G, len(rules), jmax, mmax), np.int32)
            for g, name in enumerate(names):
                for r, rule in enumerate(rules):
                    table = rule_keys(name, rule)
                    seeds[g, r, :table.shape[0], :table.shape[1]] = table
            keys.reshape(G, P, jmax, mmax)[:, :len(rules)] = be.from_numpy(seeds)

        def group_low(mk):                                           # (G,): an individual without a schedule counts as +inf
            low = xp.where(mk >= 0, mk, never).reshape(G, P).min(1)
            return low if xp is np else low.values

        history, t = [], 0
        while True:
            fitness = env.decode_keys(keys, parents, delta)
            history.append(group_low(fitness))
            if t == gens:
                break
            if tgt is not None and t and t % check_every == 0:
                window = np.stack([host(h) for h in history[-check_every:]], axis=1)
                if (window.min(axis=1) <= tgt).all():
                    break
            t += 1
            keys, _ = env.evolve_keys(keys, fitness, P, n_elite, n_mutant, rho, t, seed)
        fitness, start = env.decode_keys(keys, parents, delta, start=True)
    mk = host(fitness).astype(np.int32)
    if polish:
        walkers = _grouped_env(names, P, seed, device, _backend)
        walkers.reset()
        best, rank, _ = walkers.tabu_blocks(start, polish, int(tenure))
        mk = host(best).astype(np.int32)
    _, winner = _group_winners(mk, G, P)
    if polish:
        again, begin = walkers.evaluate_order(rank, winner, start=True)
        assert np.array_equal(host(again), mk[winner])
        rank_out, start_out = host(rank)[winner].copy(), host(begin).copy()
    else:
        start_out = host(start)[winner].copy()
        rank_out = start_out.copy()
    return BrkgaResult(makespan=mk[winner], keys=host(keys)[winner].copy(), start=start_out, rank=rank_out,
                       history=np.stack([host(h) for h in history], axis=1).astype(np.int32), generations=t,
                       optimal=np.zeros(G, bool) if tgt is None else mk[winner] <= tgt, env=env, target=tgt)


# ---- one-machine relaxations of partial selections, the shifting bottleneck construction (include/jss_machine.h) ----------------
def _jackson_preemptive(r, p, q):
    """the value of Jackson's preemptive schedule: always the released unfinished operation with the largest q"""
    n = len(r)
    rem, done, t, left, value = list(p), [False] * n, min(r), n, 0
    while left:
        ready = [i for i in range(n) if not done[i] and r[i] <= t]
        later = [r[i] for i in range(n) if not done[i] and r[i] > t]
        if not ready:
            t = min(later)
            continue
        i = max(ready, key=lambda x: (q[x], -x))
        run = min(rem[i], min(later) - t) if later else rem[i]
        t += run
        if run == rem[i]:
            done[i], left, value = True, left - 1, max(value, t + q[i])
        else:
            rem[i] -= run
    return value


def _schrage(r, p, q):
    """Schrage's schedule: (value, starts).  The operations are listed by ascending flat index, so the lowest index wins ties"""
    n = len(r)
    todo, t, value, starts = set(range(n)), min(r), 0, [0] * n
    while todo:
        ready = [i for i in todo if r[i] <= t]
        if not ready:
            t = min(r[i] for i in todo)
            continue
        i = max(ready, key=lambda x: (q[x], -x))
        starts[i], value = t, max(value, t + p[i] + q[i])
        t += p[i]
        todo.discard(i)
    return value, starts


def machine_reference(env_const, ops, rank=None, fixed=None, parents=None, fill=-1):
    """include/jss_machine.h's jss_machine_relax on host arrays, written from the header's definition, one candidate after the
    other.  ``rank`` (jmax, mmax), one table for all, or (n, jmax, mmax), or None (with nothing fixed; ``ops`` must then have its
    (tables, jmax, mmax) shape); ``fixed`` None, an int or (n,) integers, bit m set for a sequenced machine; ``parents`` (n,) or
    None (candidate c is env c).  Returns ``(length, lower_bound, bottleneck, jps, schrage, head, tail, rank_out)``: int32 (n,)
    three times, (n, mmax) twice, (n, jmax, mmax) three times.  The rows of refused (-1) and cyclic (-2) candidates hold ``fill``."""
    const = np.asarray(env_const, dtype=np.int64).reshape(-1, _abi.NC)
    B = const.shape[0]
    if rank is not None:
        rank = np.asarray(rank, dtype=np.int64)
        jmax, mmax = rank.shape[-2:]
    else:
        jmax, mmax = np.asarray(ops).shape[-2:]
    ops = np.asarray(ops, dtype=np.int64).reshape(-1, jmax, mmax)
    fixed_n = None if fixed is None or np.ndim(fixed) == 0 else len(fixed)
    n = len(parents) if parents is not None else rank.shape[0] if rank is not None and rank.ndim == 3 else fixed_n if fixed_n is not None else B
    parents = np.arange(n) if parents is None else np.asarray(parents, dtype=np.int64)
    masks = [0] * n if fixed is None else [int(fixed) & (2 ** 64 - 1)] * n if np.ndim(fixed) == 0 else [int(x) & (2 ** 64 - 1) for x in fixed]
    length, lower, neck = (np.full(n, fill, np.int32) for _ in range(3))
    jps, sch = (np.full((n, mmax), fill, np.int32) for _ in range(2))
    head, tail, rank_out = (np.full((n, jmax, mmax), fill, np.int32) for _ in range(3))
    for c in range(n):
        i, mask = int(parents[c]), masks[c]
        length[c] = -1
        if not 0 <= i < B:
            continue
        J, M, tab = (int(const[i, x]) for x in (_abi.C_JOBS, _abi.C_MACHINES, _abi.C_TABLE))
        if not (1 <= J <= jmax and 1 <= M <= mmax and 0 <= tab < ops.shape[0]) or mask >> M:
            continue
        mach, dur = ((ops[tab] >> 16) & 63).tolist(), (ops[tab] & 0xFFFF).tolist()
        row = None if rank is None else (rank[c] if rank.ndim == 3 else rank).tolist()
        real = [(j, k) for j in range(J) for k in range(M)]
        on = {}
        for j, k in real:
            on.setdefault(mach[j][k], []).append((j, k))
        if any(row[j][k] < 0 for j, k in real if mask >> mach[j][k] & 1):
            continue
        # the graph: job arcs, and the arcs of the fixed machines' orders
        succ, pred = {o: [] for o in real}, {o: [] for o in real}
        for j, k in real:
            if k + 1 < M:
                succ[(j, k)].append((j, k + 1)), pred[(j, k + 1)].append((j, k))
        for m, its in on.items():
            if mask >> m & 1:
                seq = sorted(its, key=lambda o: (row[o[0]][o[1]], o))
                for u, v in zip(seq[:-1], seq[1:]):
                    succ[u].append(v), pred[v].append(u)
        waits = {o: len(pred[o]) for o in real}
        topo = [o for o in real if not waits[o]]
        for o in topo:                                                 # (grows while it is walked)
            for v in succ[o]:
                waits[v] -= 1
                if not waits[v]:
                    topo.append(v)
        if len(topo) < len(real):
            length[c] = -2
            continue
        d = lambda o: dur[o[0]][o[1]]   # noqa: E731
        h, t = {}, {}
        for o in topo:
            h[o] = max([h[u] + d(u) for u in pred[o]] or [0])
        for o in reversed(topo):
            t[o] = max([d(v) + t[v] for v in succ[o]] or [0])
        length[c] = max(h[o] + d(o) for o in real)
        jps[c], sch[c], head[c], tail[c], rank_out[c] = -1, -1, -1, -1, -1
        for j, k in real:
            head[c, j, k], tail[c, j, k] = h[(j, k)], t[(j, k)]
            if mask >> mach[j][k] & 1:
                rank_out[c, j, k] = row[j][k]
        for m in sorted(on):
            if mask >> m & 1:
                continue
            its = on[m]                                                # (ascending by flat index)
            r, p, q = [h[o] for o in its], [d(o) for o in its], [t[o] for o in its]
            jps[c, m] = _jackson_preemptive(r, p, q)
            sch[c, m], starts = _schrage(r, p, q)
            for (j, k), s in zip(its, starts):
                rank_out[c, j, k] = s
        free = [(int(jps[c, m]), -m) for m in on if not mask >> m & 1]
        lower[c] = max([int(length[c])] + [v for v, _ in free])
        neck[c] = -max(free)[1] if free else -1
    return length, lower, neck, jps, sch, head, tail, rank_out


def bottleneck_reference(env_const, ops, parents=None, bias=None, reopt=1, rank=None, fixed=None, fill=-1):
    """include/jss_machine.h's jss_bottleneck_build on host arrays: the header's loop over ``machine_reference``, one candidate
    after the other.  ``ops`` (tables, jmax, mmax); ``bias`` (n, mmax) or None; ``rank`` (n, jmax, mmax) with ``fixed`` (n,), or
    neither.  Returns ``(makespan, rank, info, order)``: int32 (n,), (n, jmax, mmax), (n, 4), (n, mmax); the rows of refused (-1)
    and cyclic (-2) candidates hold ``fill``."""
    const = np.asarray(env_const, dtype=np.int64).reshape(-1, _abi.NC)
    ops = np.asarray(ops, dtype=np.int64)
    jmax, mmax = ops.shape[-2:]
    ops = ops.reshape(-1, jmax, mmax)
    n = len(parents) if parents is not None else const.shape[0]
    parents = np.arange(n) if parents is None else np.asarray(parents, dtype=np.int64)
    makespan = np.full(n, fill, np.int32)
    rank_o, info, order = np.full((n, jmax, mmax), fill, np.int32), np.full((n, _abi.BOTTLENECK_NI), fill, np.int32), np.full((n, mmax), fill, np.int32)
    for c in range(n):
        par = parents[c:c + 1]
        row = np.zeros((1, jmax, mmax), np.int64) if rank is None else np.asarray(rank, dtype=np.int64)[c:c + 1].copy()
        mask = 0 if fixed is None else int(fixed[c]) & (2 ** 64 - 1)
        relax = lambda r, f: machine_reference(const, ops, r, [f], par)   # noqa: E731
        i = int(par[0])
        tab = int(const[i, _abi.C_TABLE]) if 0 <= i < const.shape[0] else 0
        mach = (ops[tab] >> 16) & 63 if 0 <= tab < ops.shape[0] else None
        res = relax(row, mask)
        first, fixed_here, tried, shorter, seq = int(res[1][0]), 0, 0, 0, []
        while res[0][0] >= 0 and res[2][0] >= 0:
            free = [m for m in range(mmax) if res[3][0, m] >= 0]
            star = max(free, key=lambda m: (int(res[3][0, m]) + (0 if bias is None else int(bias[c][m])), -m))
            row = np.where(mach == star, res[7], row)                 # its Schrage starts as ranks
            mask |= 1 << star
            fixed_here, seq = fixed_here + 1, seq + [star]
            cur = int(relax(row, mask)[0][0])
            if cur < 0:
                res = (np.array([cur]),)
                break
            for _ in range(int(reopt)):
                for k in range(mmax):
                    if not mask >> k & 1 or k == star:
                        continue
                    loose = relax(row, mask & ~(1 << k))
                    trial = np.where(mach == k, loose[7], row)
                    new = int(relax(trial, mask)[0][0])
                    tried += 1
                    if 0 <= new <= cur:
                        shorter += new < cur
                        row, cur = trial, new
            res = relax(row, mask)
        makespan[c] = res[0][0]
        if makespan[c] < 0:
            continue
        J, M = (int(const[i, x]) for x in (_abi.C_JOBS, _abi.C_MACHINES))
        rank_o[c] = -1
        rank_o[c, :J, :M] = row[0, :J, :M]
        info[c] = (fixed_here, tried, shorter, first)
        order[c] = (seq + [-1] * mmax)[:mmax]
    return makespan, rank_o, info, order


@dataclass
class BottleneckResult(TabuResult):
    """What ``bottleneck_search`` returns: ``TabuResult``'s fields -- ``best_makespan`` (S,) every walker's makespan, ``info``
    (S, 4) its build's counters, ``target`` (G,) -- and ``lower_bound`` (G,), the one-machine bound of the empty selection."""
    lower_bound: Optional[np.ndarray] = None


def bottleneck_search(instances, walkers=64, reopt=1, spread=50, polish=0, tenure=8, seed=0, target="one_machine", device=None,
                      _backend=None, nodes=0):
    """Shifting bottleneck builds on one instance or on a list of them: ``walkers`` builds per instance, all in ONE launch
    (``BatchedJssEnv.bottleneck``, include/jss_machine.h), on a batch of one env per instance, which is only read.  Defined by
    public calls alone:

    start   the batch, ``reset``; ``lower_bound = relax_machines()[0]``, the one-machine bound of the empty selection; the target
            (``"one_machine"``: that bound; ``"lower_bound"``: ``env.lower_bound()``; None; an int or one per instance).
    builds  ``bias = numpy.random.default_rng(seed).integers(0, spread + 1, (G * walkers, mmax))``, the rows of walker 0 of every
            instance set to 0 (the unbiased build); ``bottleneck(repeat(arange(G), walkers), bias, reopt)``.
    polish  ``polish > 0``: every build is the rank of one walker of ``tabu_blocks(rank, iters=polish, tenure=tenure)`` on a batch
            of G * walkers envs, whose best never exceeds its start.
    end     the lowest ``(makespan, walker)`` of every instance, its order re-timed by ``evaluate_order``.

    ``nodes > 0`` (at most 4096) sequences the machines exactly (include/jss_carlier.h): the builds are
    ``bottleneck_exact(parents, bias, reopt, nodes)``, ``info`` has their 8 counters, ``lower_bound = solve_machines(nodes=nodes)[0]``,
    and ``"one_machine_exact"`` is the target that means this bound (``"one_machine"`` means it too then).  ``nodes=0`` is the path
    above, bit for bit.

    Returns a ``BottleneckResult``; ``optimal``: the makespan reached the target."""
    W, reopt, spread, polish, nodes = int(walkers), int(reopt), int(spread), int(polish), int(nodes)
    if not 0 <= nodes <= _abi.CARLIER_MAX_NODES:
        raise ValueError(f"bottleneck_search: nodes must lie in [0, {_abi.CARLIER_MAX_NODES}]")
    if W < 1:
        raise ValueError("bottleneck_search: walkers must be >= 1")
    if not 0 <= reopt <= _abi.BOTTLENECK_MAX_REOPT:
        raise ValueError(f"bottleneck_search: reopt must lie in [0, {_abi.BOTTLENECK_MAX_REOPT}]")
    if not 0 <= spread < 2 ** 30 or polish < 0:
        raise ValueError("bottleneck_search: spread in [0, 2**30), polish >= 0")
    if not 0 <= int(tenure) <= _abi.TABU_MAX_TENURE:
        raise ValueError(f"bottleneck_search: tenure must lie in [0, {_abi.TABU_MAX_TENURE}]")
    if isinstance(target, str) and target not in ("lower_bound", "one_machine", "destructive") + (("one_machine_exact",) if nodes else ()):
        raise ValueError("bottleneck_search: target is 'one_machine', 'lower_bound', 'destructive', None, an int or one int per instance"
                         " ('one_machine_exact' with nodes > 0)")
    names, G = _instance_groups("bottleneck_search", instances, "call bottleneck on a BatchedJssEnv for anything else")
    env = _grouped_env(names, 1, seed, device, _backend)
    be = env.backend
    env.reset()
    host = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    bound = host(env.solve_machines(nodes=nodes)[0] if nodes else env.relax_machines()[0]).astype(np.int32)
    if isinstance(target, str):
        tgt = (host(env.lower_bound()).astype(np.int32) if target == "lower_bound" else _destructive_target(env, G, 1) if target == "destructive"
               else bound.copy())
    elif target is None:
        tgt = None
    else:
        tgt = np.broadcast_to(np.asarray(target, np.int32), (G,)).copy()
    parents = np.repeat(np.arange(G), W).astype(np.int32)
    bias = np.random.default_rng(int(seed or 0)).integers(0, spread + 1, (G * W, env.mmax)).astype(np.int32)
    bias[::W] = 0
    best, rank, info = env.bottleneck_exact(parents, bias, reopt, nodes) if nodes else env.bottleneck(parents, bias, reopt)
    info = host(info).astype(np.int32)
    if polish:
        crowd = _grouped_env(names, W, seed, device, _backend)
        crowd.reset()
        best, rank, _ = crowd.tabu_blocks(rank, polish, int(tenure))
    mk = host(best).astype(np.int32)
    walker, winner = _group_winners(mk, G, W)
    best_rank = host(rank)[winner].copy()
    again, start = env.evaluate_order(best_rank, np.arange(G, dtype=np.int32), start=True)
    assert np.array_equal(host(again), mk[winner])
    return BottleneckResult(makespan=mk[winner], walker=walker, rank=best_rank, start=host(start).copy(),
                            optimal=np.zeros(G, bool) if tgt is None else mk[winner] <= tgt, best_makespan=mk, info=info, target=tgt,
                            env=env, lower_bound=bound)


# ---- Carlier's one-machine search, shifting bottleneck constructions sequenced by it (include/jss_carlier.h) --------------------
def carlier_reference(r, p, q, nodes):
    """include/jss_carlier.h's one-machine search, written from the header: the operations by ascending flat index with heads
    ``r``, durations ``p`` and tails ``q``, a budget of ``nodes``.  Returns ``(opt, proved, low, nodes_used, starts)``."""
    r, p, q, n = list(r), list(p), list(q), len(r)
    st = dict(best=None, starts=None, count=0, open=False)
    root = _jackson_preemptive(r, p, q)

    def node(depth):
        # 1. counted; Schrage's schedule of the working r and q, in the order it schedules
        st["count"] += 1
        todo, t, value, s, order = set(range(n)), min(r), 0, [0] * n, []
        while todo:
            ready = [i for i in todo if r[i] <= t]
            if not ready:
                t = min(r[i] for i in todo)
                continue
            i = max(ready, key=lambda x: (q[x], -x))
            s[i], value = t, max(value, t + p[i] + q[i])
            t += p[i]
            todo.discard(i)
            order.append(i)
        if st["best"] is None or value < st["best"]:
            st["best"], st["starts"] = value, list(s)
        # 2. positions in that order
        b = min(pos for pos, i in enumerate(order) if s[i] + p[i] + q[i] == value)
        a = b
        while a > 0 and s[order[a]] == s[order[a - 1]] + p[order[a - 1]]:
            a -= 1
        critical = [pos for pos in range(a, b) if q[order[pos]] < q[order[b]]]
        if not critical:
            return
        c, J = order[critical[-1]], order[critical[-1] + 1:b + 1]
        # 3.
        rJ, qJ, pJ = min(r[i] for i in J), min(q[i] for i in J), sum(p[i] for i in J)
        if max(rJ + pJ + qJ, min(rJ, r[c]) + pJ + p[c] + min(qJ, q[c])) >= st["best"]:
            return
        # 4. the budget is spent, or the depth: no child could be entered.  Else c before J, then c after J
        if st["count"] >= nodes or depth >= _abi.CARLIER_MAX_DEPTH:
            st["open"] = True
            return
        for values, raised in ((q, pJ + qJ), (r, rJ + pJ)):
            if st["open"]:
                return
            old = values[c]
            values[c] = max(old, raised)
            if _jackson_preemptive(r, p, q) < st["best"]:
                if st["count"] + 1 > nodes:
                    st["open"] = True
                else:
                    node(depth + 1)
            values[c] = old

    node(1)
    proved = not st["open"]
    return st["best"], proved, st["best"] if proved else root, st["count"], st["starts"]


def _machine_problems(const, ops, parent, relaxed, c):
    """the one-machine problems of candidate c of a machine_reference result: {m: (its, r, p, q)} for the free machines with
    operations, `its` the (j, k) ascending by flat index"""
    J, M, tab = (int(const[parent, x]) for x in (_abi.C_JOBS, _abi.C_MACHINES, _abi.C_TABLE))
    mach, dur = ((ops[tab] >> 16) & 63).tolist(), (ops[tab] & 0xFFFF).tolist()
    on = {}
    for j in range(J):
        for k in range(M):
            on.setdefault(mach[j][k], []).append((j, k))
    head, tail = relaxed[5][c], relaxed[6][c]
    return {m: (its, [int(head[o]) for o in its], [dur[j][k] for j, k in its], [int(tail[o]) for o in its])
            for m, its in sorted(on.items()) if relaxed[3][c, m] >= 0}


def solve_reference(env_const, ops, rank=None, fixed=None, parents=None, nodes=256, fill=-1):
    """include/jss_carlier.h's jss_machine_solve on host arrays, written from the header: ``machine_reference`` for what the
    header takes from jss_machine.h, then ``carlier_reference`` on every free machine.  Returns ``(length, lower_bound,
    bottleneck, opt, low, nodes_used, proved, head, tail, rank_out)``: int32 (n,) three times, (n, mmax) three times, uint64 (n,),
    int32 (n, jmax, mmax) three times.  The rows of refused (-1) and cyclic (-2) candidates hold ``fill``."""
    relaxed = machine_reference(env_const, ops, rank, fixed, parents, fill)
    length, _, _, jps, _, head, tail, rank_out = relaxed
    const = np.asarray(env_const, dtype=np.int64).reshape(-1, _abi.NC)
    jmax, mmax = head.shape[1:]
    ops = np.asarray(ops, dtype=np.int64).reshape(-1, jmax, mmax)
    n = length.size
    parents = np.arange(n) if parents is None else np.asarray(parents, dtype=np.int64)
    lower, neck = np.full(n, fill, np.int32), np.full(n, fill, np.int32)
    opt, low, used = (np.full((n, mmax), fill, np.int32) for _ in range(3))
    proved = np.full(n, np.uint64(np.int64(fill).astype(np.uint64)), np.uint64)
    rank_out = rank_out.copy()
    for c in range(n):
        if length[c] < 0:
            continue
        opt[c], low[c], used[c], mask = -1, -1, -1, 0
        for m, (its, r, p, q) in _machine_problems(const, ops, int(parents[c]), relaxed, c).items():
            opt[c, m], ok, low[c, m], used[c, m], starts = carlier_reference(r, p, q, nodes)
            mask |= int(ok) << m
            for o, s in zip(its, starts):
                rank_out[c][o] = s
        free = [(int(low[c, m]), -m) for m in range(mmax) if low[c, m] >= 0 and jps[c, m] >= 0]
        lower[c] = max([int(length[c])] + [v for v, _ in free])
        neck[c] = -max(free)[1] if free else -1
        proved[c] = mask
    return length, lower, neck, opt, low, used, proved, head, tail, rank_out


def bottleneck_exact_reference(env_const, ops, parents=None, bias=None, reopt=1, nodes=256, rank=None, fixed=None, fill=-1):
    """include/jss_carlier.h's jss_bottleneck_exact on host arrays: ``bottleneck_reference``'s loop with the machines sequenced by
    ``carlier_reference``'s best schedule, by Schrage's where that closes a cycle.  Returns ``(makespan, rank, info, order)``:
    int32 (n,), (n, jmax, mmax), (n, 8), (n, mmax); the rows of refused (-1) and cyclic (-2) candidates hold ``fill``."""
    const = np.asarray(env_const, dtype=np.int64).reshape(-1, _abi.NC)
    ops = np.asarray(ops, dtype=np.int64)
    jmax, mmax = ops.shape[-2:]
    ops = ops.reshape(-1, jmax, mmax)
    n = len(parents) if parents is not None else const.shape[0]
    parents = np.arange(n) if parents is None else np.asarray(parents, dtype=np.int64)
    makespan = np.full(n, fill, np.int32)
    rank_o, info, order = np.full((n, jmax, mmax), fill, np.int32), np.full((n, _abi.EXACT_NI), fill, np.int32), np.full((n, mmax), fill, np.int32)
    for c in range(n):
        par = parents[c:c + 1]
        row = np.zeros((1, jmax, mmax), np.int64) if rank is None else np.asarray(rank, dtype=np.int64)[c:c + 1].copy()
        mask = 0 if fixed is None else int(fixed[c]) & (2 ** 64 - 1)
        relax = lambda r, f: machine_reference(const, ops, r, [f], par)   # noqa: E731
        i = int(par[0])
        tab = int(const[i, _abi.C_TABLE]) if 0 <= i < const.shape[0] else 0
        mach = (ops[tab] >> 16) & 63 if 0 <= tab < ops.shape[0] else None
        count = dict(total=0, most=0, open=0, replaced=0)

        def sequence(loose, k, row, with_k):
            """machine k, free in the relaxation `loose`, sequenced: (the rank table, the length of (table, with_k))"""
            its, r, p, q = _machine_problems(const, ops, i, loose, 0)[k]
            _, ok, _, used, starts = carlier_reference(r, p, q, nodes)
            count["total"] += used
            count["most"] = max(count["most"], used)
            count["open"] += not ok
            trial = row.copy()
            for o, s in zip(its, starts):
                trial[0][o] = s
            new = int(relax(trial, with_k)[0][0])
            if new == -2:
                count["replaced"] += 1
                trial = np.where(mach == k, loose[7], row)             # its Schrage starts as ranks
                new = int(relax(trial, with_k)[0][0])
            return trial, new

        res = relax(row, mask)
        first, fixed_here, tried, shorter, seq = int(res[1][0]), 0, 0, 0, []
        if res[0][0] >= 0:
            first = max([int(res[0][0])] + [carlier_reference(r, p, q, nodes)[2] for _, r, p, q in _machine_problems(const, ops, i, res, 0).values()])
        while res[0][0] >= 0 and res[2][0] >= 0:
            free = [m for m in range(mmax) if res[3][0, m] >= 0]
            star = max(free, key=lambda m: (int(res[3][0, m]) + (0 if bias is None else int(bias[c][m])), -m))
            mask |= 1 << star
            row, cur = sequence(res, star, row, mask)
            fixed_here, seq = fixed_here + 1, seq + [star]
            if cur < 0:
                res = (np.array([cur]),)
                break
            for _ in range(int(reopt)):
                for k in range(mmax):
                    if not mask >> k & 1 or k == star:
                        continue
                    tried += 1
                    loose = relax(row, mask & ~(1 << k))
                    if loose[3][0, k] < 0:                             # (a fixed machine without operations: nothing changes)
                        continue
                    trial, new = sequence(loose, k, row, mask)
                    if 0 <= new <= cur:
                        shorter += new < cur
                        row, cur = trial, new
            res = relax(row, mask)
        makespan[c] = res[0][0]
        if makespan[c] < 0:
            continue
        J, M = (int(const[i, x]) for x in (_abi.C_JOBS, _abi.C_MACHINES))
        rank_o[c] = -1
        rank_o[c, :J, :M] = row[0, :J, :M]
        info[c] = (fixed_here, tried, shorter, first, count["total"], count["most"], count["open"], count["replaced"])
        order[c] = (seq + [-1] * mmax)[:mmax]
    return makespan, rank_o, info, order


# ---- constraint propagation on operation windows, destructive lower bounds (include/jss_propagate.h) ---------------------------
PROPAGATE_RULES = ("job", "fixed", "pairs", "overload", "after", "before")


def _task_intervals(est, lct, d, rules, slack):
    """Rule 4 of include/jss_propagate.h on one free machine's operations of positive duration, as the header states it: every
    pair (a, b), its set W, the overload test and the bounds that "after" and "before" give every operation outside W.  Returns
    ``(overload, est deductions, lct deductions)``."""
    n = est.size
    inside = (est[None, None, :] >= est[:, None, None]) & (lct[None, None, :] <= lct[None, :, None])        # [a, b, x]
    idx = np.arange(n)
    counts = inside[idx, :, idx] & inside[:, idx, idx]                                                        # a in W and b in W
    P = (inside * d).sum(axis=2)
    over = bool((counts & (est[:, None] + P + slack > lct[None, :])).any()) if "overload" in rules else False
    new_est, new_lct = est.copy(), lct.copy()
    weights = (inside * d).reshape(n * n, n).astype(np.float64)
    # [a, b, x]: the sum of d over {y in W(a, b) : with[x, y]}, one matrix product (in doubles, which hold these sums exactly)
    sums = lambda with_: np.rint(weights @ with_.T.astype(np.float64)).astype(np.int64).reshape(n, n, n)   # noqa: E731
    if "after" in rules:
        later = (est[None, :] >= est[:, None]).astype(np.int64)                                               # [x, y]: est_y >= est_x
        ends = np.where(inside, est[None, None, :] + sums(later), -2 ** 62).max(axis=2)
        hit = counts[:, :, None] & ~inside & (np.minimum(est[:, None, None], est[None, None, :]) + P[:, :, None] + d[None, None, :]
                                              > lct[None, :, None])
        new_est = np.maximum(new_est, np.where(hit, ends[:, :, None], -2 ** 62).max(axis=(0, 1)))
    if "before" in rules:
        sooner = (lct[None, :] <= lct[:, None]).astype(np.int64)                                              # [x, y]: lct_y <= lct_x
        begins = np.where(inside, lct[None, None, :] - sums(sooner), 2 ** 62).min(axis=2)
        hit = counts[:, :, None] & ~inside & (est[:, None, None] + P[:, :, None] + d[None, None, :]
                                              > np.maximum(lct[None, :, None], lct[None, None, :]))
        new_lct = np.minimum(new_lct, np.where(hit, begins[:, :, None], 2 ** 62).min(axis=(0, 1)))
    return over, new_est, new_lct


def propagate_reference(env_const, ops, ub, rank=None, fixed=None, parents=None, est=None, lct=None, hyp=None, passes=256, fill=-1,
                        rules=PROPAGATE_RULES, _overload_slack=0):
    """include/jss_propagate.h's jss_propagate on host arrays, the plain restatement of the header's definition, one candidate
    after the other: ``machine_reference`` for what the header takes from jss_machine.h, then Jacobi passes of the rules.
    ``ub`` an int or (n,); ``est`` / ``lct`` (jmax, mmax), one table for all, or (n, jmax, mmax), or None; ``hyp`` three (n,) arrays
    or None; the rest as in ``machine_reference``.  ``rules`` names the rules that are applied (all of them: the definition; fewer
    tell what a rule contributes).  Returns ``(status, passes_used, est, lct)``: int32 (n,) twice, (n, jmax, mmax) twice; rows
    that the call does not write hold ``fill``."""
    const = np.asarray(env_const, dtype=np.int64).reshape(-1, _abi.NC)
    B = const.shape[0]
    if rank is not None:
        rank = np.asarray(rank, dtype=np.int64)
        jmax, mmax = rank.shape[-2:]
    else:
        jmax, mmax = np.asarray(ops).shape[-2:]
    ops = np.asarray(ops, dtype=np.int64).reshape(-1, jmax, mmax)
    est_in = None if est is None else np.asarray(est, dtype=np.int64)
    lct_in = None if lct is None else np.asarray(lct, dtype=np.int64)
    sizes = [len(parents) if parents is not None else None, rank.shape[0] if rank is not None and rank.ndim == 3 else None,
             None if fixed is None or np.ndim(fixed) == 0 else len(fixed), est_in.shape[0] if est_in is not None and est_in.ndim == 3 else None,
             len(ub) if np.ndim(ub) == 1 else None, len(hyp[0]) if hyp is not None else None, B]
    n = next(x for x in sizes if x is not None)
    par = np.arange(n) if parents is None else np.asarray(parents, dtype=np.int64)
    masks = [0] * n if fixed is None else [int(fixed) & (2 ** 64 - 1)] * n if np.ndim(fixed) == 0 else [int(x) & (2 ** 64 - 1) for x in fixed]
    ubs = np.broadcast_to(np.asarray(ub, dtype=np.int64), (n,))
    status, used = np.full(n, fill, np.int32), np.full(n, fill, np.int32)
    est_o, lct_o = np.full((n, jmax, mmax), fill, np.int32), np.full((n, jmax, mmax), fill, np.int32)
    ok = lambda v: 0 <= int(v) <= _abi.PROPAGATE_MAX_TIME   # noqa: E731
    for c in range(n):
        row = None if rank is None else rank[c] if rank.ndim == 3 else rank
        res = machine_reference(const, ops, None if row is None else row[None], [masks[c]], par[c:c + 1])
        status[c] = -1
        if res[0][0] == -1:
            continue
        i = int(par[c])
        J, M, tab = (int(const[i, x]) for x in (_abi.C_JOBS, _abi.C_MACHINES, _abi.C_TABLE))
        mach, d = ((ops[tab] >> 16) & 63)[:J, :M], (ops[tab] & 0xFFFF)[:J, :M]
        e_in = None if est_in is None else (est_in[c] if est_in.ndim == 3 else est_in)[:J, :M]
        l_in = None if lct_in is None else (lct_in[c] if lct_in.ndim == 3 else lct_in)[:J, :M]
        h = -1 if hyp is None else int(hyp[0][c])
        if not ok(ubs[c]) or (e_in is not None and not (all(ok(v) for v in e_in.reshape(-1)) and all(ok(v) for v in l_in.reshape(-1)))):
            continue
        if h >= 0 and not (h < jmax * mmax and h // mmax < J and h % mmax < M and ok(hyp[1][c]) and ok(hyp[2][c])):
            continue
        if res[0][0] == -2:
            status[c] = -2
            continue
        e = res[5][0, :J, :M].astype(np.int64)
        l = int(ubs[c]) - res[6][0, :J, :M].astype(np.int64)   # noqa: E741
        if e_in is not None:
            e, l = np.maximum(e, e_in), np.minimum(l, l_in)   # noqa: E741
        if h >= 0:
            e[h // mmax, h % mmax] = max(e[h // mmax, h % mmax], int(hyp[1][c]))
            l[h // mmax, h % mmax] = min(l[h // mmax, h % mmax], int(hyp[2][c]))
        # the arcs of the fixed machines, and the free machines' operations of positive duration
        arcs, free = [], []
        for m in sorted(set(mach.reshape(-1).tolist())):
            its = [(j, k) for j in range(J) for k in range(M) if mach[j, k] == m]
            if masks[c] >> m & 1:
                seq = sorted(its, key=lambda o: (row[o[0]][o[1]], o))
                arcs += list(zip(seq[:-1], seq[1:]))
            else:
                its = [o for o in its if d[o] > 0]
                if its:
                    free.append((np.array([o[0] for o in its]), np.array([o[1] for o in its])))
        state, count = _abi.PROPAGATE_REFUTED if (e + d > l).any() else _abi.PROPAGATE_BUDGET, 0
        while state == _abi.PROPAGATE_BUDGET and count < int(passes):
            count += 1
            ne, nl, over = e.copy(), l.copy(), False
            if "job" in rules:
                ne[:, 1:] = np.maximum(ne[:, 1:], (e + d)[:, :-1])
                nl[:, :-1] = np.minimum(nl[:, :-1], (l - d)[:, 1:])
            if "fixed" in rules:
                for u, v in arcs:
                    ne[v] = max(ne[v], e[u] + d[u])
                    nl[u] = min(nl[u], l[v] - d[v])
            for js, ks in free:
                ee, ll, dd = e[js, ks], l[js, ks], d[js, ks]
                if "pairs" in rules:
                    never = (ee[:, None] + dd[:, None] + dd[None, :] > ll[None, :]) & ~np.eye(ee.size, dtype=bool)    # [i, j]: i cannot precede j
                    ne[js, ks] = np.maximum(ne[js, ks], np.where(never, (ee + dd)[None, :], -2 ** 62).max(axis=1))
                    nl[js, ks] = np.minimum(nl[js, ks], np.where(never, (ll - dd)[:, None], 2 ** 62).min(axis=0))
                o, te, tl = _task_intervals(ee, ll, dd, rules, int(_overload_slack))
                over = over or o
                ne[js, ks], nl[js, ks] = np.maximum(ne[js, ks], te), np.minimum(nl[js, ks], tl)
            moved = not (np.array_equal(ne, e) and np.array_equal(nl, l))
            e, l = ne, nl   # noqa: E741
            state = _abi.PROPAGATE_REFUTED if over or (e + d > l).any() else _abi.PROPAGATE_BUDGET if moved else _abi.PROPAGATE_FIXPOINT
        status[c], used[c] = state, count
        if state != _abi.PROPAGATE_REFUTED:
            est_o[c], lct_o[c] = -1, -1
            est_o[c, :J, :M], lct_o[c, :J, :M] = e, l
    return status, used, est_o, lct_o


@dataclass
class DestructiveResult:
    """What ``destructive_bound`` returns, one entry per instance: ``lower_bound`` (G,), the first trial makespan that neither
    propagation nor shaving refuted (never above ``upper``); ``first_bound`` (G,), the scan's: the first that propagation alone
    left open; ``one_machine`` (G,), ``solve_machines()[0]`` of the empty selection, where the scan began; ``est`` and ``lct`` (G,
    jmax, mmax), the windows at ``lower_bound`` (-1 in the padding; -1 everywhere where ``upper`` itself was refuted); ``launches``
    and ``propagations`` (G,), the calls of ``propagate`` and their candidates; ``proved_optimal`` (G,): the bound reached
    ``upper``."""
    lower_bound: np.ndarray
    first_bound: np.ndarray
    one_machine: np.ndarray
    est: np.ndarray
    lct: np.ndarray
    launches: np.ndarray
    propagations: np.ndarray
    proved_optimal: np.ndarray
    env: Optional[object] = None


def _destructive_scan(prop, start, upper, span):
    """the first trial makespan from ``start`` on that ``prop(ubs)`` -> (status, est, lct) does not refute, ``span`` of them per
    call and none at or above ``upper``: (bound, est, lct or None twice, launches, propagations)"""
    U, launches, count = int(start), 0, 0
    while upper is None or U < upper:
        ubs = U + np.arange(span, dtype=np.int64)
        if upper is not None:
            ubs = ubs[ubs < upper]
        status, est, lct = prop(ubs)
        launches, count = launches + 1, count + ubs.size
        left = np.flatnonzero(status != _abi.PROPAGATE_REFUTED)
        if left.size:
            return int(ubs[left[0]]), est[left[0]].copy(), lct[left[0]].copy(), launches, count
        U += ubs.size
    return int(upper), None, None, launches, count


def shaving_hypotheses(est, lct, dur):
    """One shaving round's candidates on the window tables ``est`` / ``lct`` (jmax, mmax; -1 in the padding) with the durations
    ``dur``: two per operation whose window holds more than one start, "the start is at most mid" and "at least mid + 1", mid the
    middle of its starts.  Returns ``(ops, mid, d, hyp)``: the operations' flat indices, their middles and durations, and the
    three (2 * len(ops),) arrays ``BatchedJssEnv.propagate`` takes as ``hyp``."""
    late = lct - dur                                                   # the latest starts
    ops = np.flatnonzero(((est >= 0) & (late > est)).reshape(-1))
    e, s, d = est.reshape(-1)[ops].astype(np.int64), late.reshape(-1)[ops].astype(np.int64), dur.reshape(-1)[ops].astype(np.int64)
    mid = (e + s) // 2
    hyp = (np.repeat(ops, 2).astype(np.int32), np.stack([e, mid + 1], axis=1).reshape(-1).astype(np.int32),
           np.stack([mid + d, s + d], axis=1).reshape(-1).astype(np.int32))
    return ops, mid, d, hyp


def _destructive_loop(prop, dur, one_machine, upper, shave, rounds, span):
    """``destructive_bound``'s loop on one instance.  ``prop(ubs, est=None, lct=None, hyp=None)`` propagates one candidate per
    entry of ``ubs`` -- from the shared tables ``est`` / ``lct`` and under the hypotheses ``hyp`` where given -- and returns host
    arrays ``(status, est, lct)``; ``dur`` (jmax, mmax) holds the durations."""
    upper = None if upper is None else int(upper)
    U, est, lct, launches, count = _destructive_scan(prop, one_machine if upper is None else min(one_machine, upper), upper, span)
    first = U
    while shave and est is not None and (upper is None or U < upper):
        dead = False
        for _ in range(int(rounds)):
            ops, mid, d, hyp = shaving_hypotheses(est, lct, dur)
            if not ops.size:
                break
            status = prop(np.full(2 * ops.size, U, np.int64), est, lct, hyp)[0]
            launches, count = launches + 1, count + 2 * ops.size
            gone = (status == _abi.PROPAGATE_REFUTED).reshape(-1, 2)
            dead = bool(gone.all(axis=1).any())
            if dead or not gone.any():
                break
            est, lct = est.copy(), lct.copy()
            low, high = gone[:, 0], gone[:, 1]
            est.reshape(-1)[ops[low]] = (mid + 1)[low]                 # the lower half is refuted: the start lies above mid
            lct.reshape(-1)[ops[high]] = (mid + d)[high]               # the upper half is refuted: the start lies at or below mid
            status, new_est, new_lct = prop(np.full(1, U, np.int64), est, lct)
            launches, count = launches + 1, count + 1
            dead = status[0] == _abi.PROPAGATE_REFUTED
            if dead:
                break
            est, lct = new_est[0].copy(), new_lct[0].copy()
        if not dead:
            break
        U, est, lct, more, n = _destructive_scan(prop, U + 1, upper, 1)  # U is refuted: on from U + 1, where shaving starts anew
        launches, count = launches + more, count + n
    if est is None:                                                    # the bound is `upper`, which was not propagated
        status, e, l = prop(np.full(1, U, np.int64))   # noqa: E741
        launches, count = launches + 1, count + 1
        fill = status[0] == _abi.PROPAGATE_REFUTED
        est, lct = (np.full_like(e[0], -1), np.full_like(l[0], -1)) if fill else (e[0].copy(), l[0].copy())
    return U, first, est, lct, launches, count


def _pack_destructive(rows, one_machine, upper, env):
    bound, first, est, lct, launches, count = (np.asarray(x) for x in zip(*rows))
    upper_of = None if upper is None else np.broadcast_to(np.asarray(upper, np.int64), bound.shape)
    return DestructiveResult(lower_bound=bound.astype(np.int32), first_bound=first.astype(np.int32), one_machine=np.asarray(one_machine, np.int32),
                             est=est.astype(np.int32), lct=lct.astype(np.int32), launches=launches.astype(np.int64),
                             propagations=count.astype(np.int64),
                             proved_optimal=np.zeros(bound.shape, bool) if upper_of is None else bound >= upper_of, env=env)


def _destructive_args(what, instances, upper, rounds, span, passes):
    names, _ = _instance_groups(what, instances, "call propagate on a BatchedJssEnv for anything else")
    if int(rounds) < 0 or int(span) < 1 or not 1 <= int(passes) <= _abi.PROPAGATE_MAX_PASSES:
        raise ValueError(f"{what}: rounds >= 0, span >= 1, passes in [1, {_abi.PROPAGATE_MAX_PASSES}]")
    uppers = [None] * len(names) if upper is None else [int(x) for x in np.broadcast_to(np.asarray(upper, np.int64), (len(names),))]
    if any(x is not None and not 0 <= x <= _abi.PROPAGATE_MAX_TIME for x in uppers):
        raise ValueError(f"{what}: upper must lie in [0, {_abi.PROPAGATE_MAX_TIME}]")
    return names, uppers


def destructive_bound(instances, upper=None, shave=True, rounds=8, span=64, passes=256, device=None, _backend=None):
    """A destructive lower bound per instance (one, or a list of them), by constraint propagation on the device
    (``BatchedJssEnv.propagate``, include/jss_propagate.h) on a batch of one env per instance, which is only read.  Defined by
    public calls alone, per instance:

    scan    from ``solve_machines()[0]``, the one-machine bound of the empty selection: one ``propagate`` launch takes ``span``
            consecutive trial makespans as candidates; the first that is not refuted is ``first_bound``; the next span follows
            where all are refuted.  No makespan at or above ``upper`` (an int, or one per instance) is tried: the bound never
            exceeds it.
    shave   at the bound U, with the windows of U's propagation as one shared table: a round is one launch with two candidates
            per operation whose window holds more than one start -- "the start is at most mid" and "at least mid + 1", mid the
            middle of its starts.  A refuted half is cut off the table; both halves of one operation refuted refute U.  After a
            round that cut something the table is propagated again, one candidate without a hypothesis.  U refuted: the bound is
            U + 1 (scanned on, one makespan a launch) and shaving starts anew there.  It ends with a round that cuts nothing,
            after ``rounds`` rounds at one U, or at ``upper``.

    Returns a ``DestructiveResult``."""
    names, uppers = _destructive_args("destructive_bound", instances, upper, rounds, span, passes)
    G = len(names)
    env = _grouped_env(names, 1, 0, device, _backend)
    be = env.backend
    env.reset()
    host = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    one_machine = host(env.solve_machines()[0]).astype(np.int64)
    const = host(env.env_const).reshape(-1, _abi.NC)
    ops = np.asarray(env.packed.ops).reshape(-1, env.jmax, env.mmax)
    rows = []
    for g in range(G):
        def prop(ubs, est=None, lct=None, hyp=None, g=g):
            out = env.propagate(np.asarray(ubs, np.int32), parents=np.full(len(ubs), g, np.int32), est=est, lct=lct, hyp=hyp, passes=passes,
                                windows=True)
            return host(out[0]), host(out[2]), host(out[3])
        dur = (ops[int(const[g, _abi.C_TABLE])] & 0xFFFF).astype(np.int64)
        rows.append(_destructive_loop(prop, dur, int(one_machine[g]), uppers[g], shave, rounds, int(span)))
    return _pack_destructive(rows, one_machine, upper, env)


def destructive_reference(instances, upper=None, shave=True, rounds=8, span=64, passes=256):
    """``destructive_bound``'s loop over the NumPy mirrors ``solve_reference`` and ``propagate_reference``; the instance tables
    come from a batch on the host-core twin, which is only reset."""
    from .env import CpuBackend
    names, uppers = _destructive_args("destructive_reference", instances, upper, rounds, span, passes)
    G = len(names)
    env = _grouped_env(names, 1, 0, None, CpuBackend(threads=1))
    env.reset()
    const = np.asarray(env.backend.numpy(env.env_const)).reshape(-1, _abi.NC)
    ops = np.asarray(env.packed.ops).reshape(-1, env.jmax, env.mmax)
    one_machine = solve_reference(const, ops)[1].astype(np.int64)
    rows = []
    for g in range(G):
        def prop(ubs, est=None, lct=None, hyp=None, g=g):
            out = propagate_reference(const, ops, np.asarray(ubs), parents=np.full(len(ubs), g), est=est, lct=lct, hyp=hyp, passes=passes)
            return out[0], out[2], out[3]
        dur = (ops[int(const[g, _abi.C_TABLE])] & 0xFFFF).astype(np.int64)
        rows.append(_destructive_loop(prop, dur, int(one_machine[g]), uppers[g], shave, rounds, int(span)))
    return _pack_destructive(rows, one_machine, upper, None)


def _destructive_target(env, groups, walkers, span=64, passes=256):
    """the scan's bound of ``destructive_bound`` for every group of ``walkers`` envs of ``env`` (the group's first env is
    asked), one entry per env"""
    be = env.backend
    host = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    firsts = (np.arange(groups) * walkers).astype(np.int32)
    start = host(env.solve_machines(parents=firsts)[0]).astype(np.int64)
    out = np.zeros(groups, np.int32)
    for g in range(groups):
        def prop(ubs, g=g):
            res = env.propagate(np.asarray(ubs, np.int32), parents=np.full(len(ubs), firsts[g], np.int32), passes=passes, windows=True)
            return host(res[0]), host(res[2]), host(res[3])
        out[g] = _destructive_scan(prop, int(start[g]), None, span)[0]
    return np.repeat(out, walkers)
