"""The search calls of ``BatchedJssEnv``: candidate moves scored by rollouts, lower bounds, machine orders and the walks over
them, key decoding, one-machine relaxations and constraint propagation -- one launch each through the C ABI of a library of its
own (include/jss_search.h, jss_bound.h, jss_order.h, jss_tabu.h, jss_block.h, jss_relink.h, jss_decode.h, jss_machine.h,
jss_carlier.h, jss_propagate.h).

``SearchCalls`` is the mixin ``BatchedJssEnv`` inherits them from; it reads the batch (``backend``, ``batch``, ``jmax``,
``mmax``, ``_desc``, ``_state``, ``solution``, ``action_mask``, ``env_const``, ``seed``) and its ``_selector`` and
``_no_open_session``, and knows nothing else of the env module.  What the calls share is written once: the guard, the staging of
the caller's arrays, the launch.  Also here: ``library``, which finds the library of a family on a backend, and the refusals of
the wrappers that do not search (``BucketedJssEnv``, ``JssVectorEnv``).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Union

import numpy as np

from . import _abi

# ---- the libraries ---------------------------------------------------------------------------------------------------------------
# family -> the symbols its header declares, what binds them, what to say of a library without them
LIBRARIES = {
    "beam": (("jss_beam_select",), _abi.bind_beam, "beam search: the backend's library does not export jss_beam_select (include/jss_beam.h)"),
    "bound": (("jss_bound",), _abi.bind_bound, "lower_bound: the backend's library does not export jss_bound (include/jss_bound.h)"),
    "order": (_abi.ORDER_SYMBOLS, _abi.bind_order, "evaluate_order: the backend's library does not export include/jss_order.h"),
    "tabu": (_abi.TABU_SYMBOLS, _abi.bind_tabu, "tabu: the backend's library does not export include/jss_tabu.h"),
    "block": (_abi.BLOCK_SYMBOLS, _abi.bind_block, "tabu_blocks: the backend's library does not export include/jss_block.h"),
    "relink": (_abi.RELINK_SYMBOLS, _abi.bind_relink, "relink: the backend's library does not export include/jss_relink.h"),
    "decode": (_abi.DECODE_SYMBOLS, _abi.bind_decode, "decode: the backend's library does not export include/jss_decode.h"),
    "machine": (_abi.MACHINE_SYMBOLS, _abi.bind_machine, "relax_machines: the backend's library does not export include/jss_machine.h"),
    "carlier": (_abi.CARLIER_SYMBOLS, _abi.bind_carlier, "solve_machines: the backend's library does not export include/jss_carlier.h"),
    "propagate": (_abi.PROPAGATE_SYMBOLS, _abi.bind_propagate, "propagate: the backend's library does not export include/jss_propagate.h"),
}


def library(backend, family):
    """The library of ``backend`` that exports the header of ``family``: ``backend.<family>_lib`` (HipBackend:
    libjss_<family>_hip.so, loaded on first use; CpuBackend: the twin), else ``backend.lib`` itself when it carries the symbols."""
    symbols, bind, message = LIBRARIES[family]
    lib = getattr(backend, family + "_lib", None)
    if lib is None:
        lib = backend.lib
        if not all(hasattr(lib, name) for name in symbols):
            raise RuntimeError(message)
        bind(lib)
    return lib


# ---- the wrappers that do not search ---------------------------------------------------------------------------------------------
# method, what the wrapper does not do, the driver that takes a list of instances instead
REFUSALS = (
    ("evaluate_order", "does not evaluate machine orders", "search.improve takes one, or a list of instances"),
    ("tabu", "does not run tabu search", "search.tabu_search takes a list of instances"),
    ("tabu_blocks", "does not run tabu search", "search.tabu_search takes a list of instances"),
    ("relink", "does not relink machine orders", "search.relink_search takes a list of instances"),
    ("order_distance", "does not relink machine orders", "search.relink_search takes a list of instances"),
    ("decode_keys", "does not decode key tables", "search.brkga_search takes a list of instances"),
    ("evolve_keys", "does not evolve key tables", "search.brkga_search takes a list of instances"),
    ("relax_machines", "does not relax partial selections", "search.bottleneck_search takes a list of instances"),
    ("bottleneck", "does not build machine orders", "search.bottleneck_search takes a list of instances"),
    ("solve_machines", "does not solve one-machine problems", "search.bottleneck_search takes a list of instances"),
    ("bottleneck_exact", "does not build machine orders", "search.bottleneck_search takes a list of instances"),
    ("propagate", "does not propagate operation windows", "search.destructive_bound takes a list of instances"),
)


def refuses_search_calls(cls):
    """Class decorator: the methods of ``REFUSALS`` on ``cls``, each raising NotImplementedError with the way to go instead."""
    def refusal(name, does_not, hint):
        def method(self, *args, **kwargs):
            raise NotImplementedError(f"{cls.__name__} {does_not}: call {name} on a BatchedJssEnv ({hint})")
        method.__name__, method.__qualname__ = name, f"{cls.__qualname__}.{name}"
        return method
    for row in REFUSALS:
        setattr(cls, row[0], refusal(*row))
    return cls


_NO_TABLE = (None, None, 0)


class SearchCalls:
    # -- what the calls share --------------------------------------------------------------------------------------------------
    def _guard(self, what):
        """reset first, no open step session"""
        if not self._is_reset:
            raise RuntimeError(f"call reset() before {what}()")
        if what in ("lookahead", "lower_bound"):
            self._no_open_session(what)
        elif self._session is not None and not self._session.closed:
            raise NotImplementedError(f"{what} does not run while a step session is open on this env: close() it first")

    def _ints(self, x, fits=None, error=None, got=False):
        """The caller's integers (a host sequence or an array of the backend) as an int32 array of the backend that is this
        call's own; ``fits``: the shape it must have, or the number of its axes, else ValueError(``error``[, got its shape])."""
        be = self.backend
        x = be.as_device(x, "int32")
        if getattr(be, "torch", None) is None:
            x = x.copy()                                           # (as_device keeps ONE array alive: a second would drop the first)
        shape = tuple(x.shape)
        if fits is not None and (len(shape) != fits if isinstance(fits, int) else shape != tuple(fits)):
            raise ValueError(error + (f", got {shape}" if got else ""))
        return x

    def _per_candidate(self, what, name, x, n, scale=None):
        """The argument that is one scalar for all or one entry per candidate: None for a scalar (or None: the caller reads it
        itself), else ``(n,)`` int32 of the backend.  ``scale``: the entries are floats in [0, 1] and arrive as
        ``round(x * scale)``."""
        if x is None or (x.ndim if hasattr(x, "ndim") else np.ndim(x)) == 0:
            return None
        if scale is None:
            return self._ints(x, (n,), f"{what}: {name} must be an int or have shape {(n,)}")
        d = np.asarray(x.detach().cpu() if hasattr(x, "detach") else x, np.float64)
        if d.shape != (n,):
            raise ValueError(f"{what}: {name} must be a float or have shape {(n,)}")
        if not ((d >= 0.0) & (d <= 1.0)).all():
            raise ValueError(f"{what}: {name} must lie in [0, 1]")
        return self.backend.from_numpy(np.round(d * scale).astype(np.int32))

    def _order(self, what, name, rank):
        """a machine order per env, ``(B, jmax, mmax)``; None: the envs' own ``solution``"""
        shape = (self.batch, self.jmax, self.mmax)
        return self.solution if rank is None else self._ints(rank, shape, f"{what}: {name} must have shape {shape}", got=True)

    def _tables(self, what, name, x):
        """``(jmax, mmax)`` -- one table for every candidate -- or ``(n, jmax, mmax)``: the array, n (None for the one table) and
        the stride from a candidate's table to the next (0 for the one table)"""
        J, M = self.jmax, self.mmax
        x = self._ints(x)
        shape = tuple(x.shape)
        if not (shape == (J, M) or (len(shape) == 3 and shape[1:] == (J, M))):
            raise ValueError(f"{what}: {name} must have shape {(J, M)} or (n, {J}, {M}), got {shape}")
        return (x, shape[0], J * M) if len(shape) == 3 else (x, None, 0)

    def _candidates(self, what, parents, actions, every):
        """The candidate moves of ``lookahead`` and ``lower_bound``, ``(parents, actions, shape of the result)``: with ``every``
        all actions of all envs, parent-major, built on the device; the caller's two lists; or none -- the states themselves."""
        be = self.backend
        B, A = self.batch, self.jmax + 1
        if every:
            t = getattr(be, "torch", None)
            if t is not None:
                return (t.arange(B, dtype=t.int32, device=be.device).repeat_interleave(A),
                        t.arange(A, dtype=t.int32, device=be.device).repeat(B), (B, A))
            return np.repeat(np.arange(B, dtype=np.int32), A), np.tile(np.arange(A, dtype=np.int32), B), (B, A)
        if parents is None:
            return None, None, (B,)
        par, act = self._ints(parents), self._ints(actions)
        if par.ndim != 1 or tuple(par.shape) != tuple(act.shape):
            raise ValueError(f"{what}: parents and actions must be 1-d and of equal length")
        return par, act, (int(par.shape[0]),)

    def _minus_one(self, *shape, want=True):
        """an int32 output filled with -1 (None unless ``want``)"""
        if not want:
            return None
        x = self.backend.zeros(shape, "int32")
        x -= 1
        return x

    def _launch(self, what, lib, fn, arg, n, inputs, with_env=True):
        """``lib.fn([desc, state,] arg, stream)`` unless there is nothing to do (``n == 0``), RuntimeError naming the entry point
        unless it returns 0; the staged ``inputs`` stay alive until the next call of ``what``: the launch has read them by then."""
        be = self.backend
        if n:
            env = (C.byref(self._desc), C.byref(self._state)) if with_env else ()
            rc = getattr(lib, fn)(*env, C.byref(arg), be.stream())
            if rc:
                _abi.check(be.lib, rc, fn)
        self.__dict__.setdefault("_search_inputs", {})[what] = inputs

    # -- search: candidate moves scored by rule rollouts (jss_lookahead, include/jss_search.h) ----------------------------
    def lookahead(self, kind: Union[str, int] = "SPT", actions=None, parents=None, n_iter: Optional[int] = None,
                  seed: Optional[int] = None, explore: float = 0.0, id_base: int = 0, weights=None, keys=None, nope_key=None):
        """Score candidate moves without cloning: candidate k starts from env ``parents[k]``, takes ``actions[k]`` (job, J =
        NOPE, -1 = none) and then follows the rule ``kind`` to the end of the episode, on the device, in registers; the batch
        is not touched.  Exactly what ``fork([parents[k]], env_id_base=id_base + k)``, ``step(actions[k])`` and
        ``rollout(kind, n_iter, seed, explore=explore, autoreset=False)`` would give, bit for bit, random draws included.

        Returns device arrays ``(makespan, steps, ret)``: the clock at done (int32; -1 when the parent is done, the action is
        not in its mask or out of range, the parent index is out of range, or the episode has not ended after ``n_iter``
        policy steps), the env steps taken (int32, the forced one included) and the return, the sum of the rewards as
        ``reward_num / max_time_op`` of the parent (float32).  ``parents`` / ``actions``: host or device int sequences of
        equal length -> shape ``(n,)``; both None: every action of every env, parent-major, built on the device -> shape
        ``(B, jmax + 1)`` (illegal and padded columns -1).  ``n_iter=None``: ``3 * jmax * mmax``, enough to finish any
        episode.  A batch dealt out by shape class is evaluated in one launch on the padded extents' kernel.
        ``weights`` (with ``kind="weighted"``): the continuation follows the caller's weighted rule (``jss_rule_lookahead``,
        see ``policy``), candidate k with the row of ``parents[k]``.  ``keys`` / ``nope_key`` (with ``kind="keys"``): it follows
        the caller's key tables (``jss_key_lookahead``), candidate k with the table of ``parents[k]``."""
        self._guard("lookahead")
        if (actions is None) != (parents is None):
            raise ValueError("lookahead: give both parents and actions, or neither (every action of every env)")
        be = self.backend
        _abi.ensure_bound(be.lib, "jss")                       # (a library bound by _abi.bind alone: test backends)
        t = getattr(be, "torch", None)
        B = self.batch
        sel = self._selector(kind, "lookahead", weights, keys, nope_key)
        n_iter = 3 * self.jmax * self.mmax if n_iter is None else int(n_iter)
        with be.on_device():
            par, act, shape = self._candidates("lookahead", parents, actions, every=parents is None)
            n = int(np.prod(shape))
            makespan, steps, rnum = be.zeros((n,), "int32"), be.zeros((n,), "int32"), be.zeros((n,), "int64")
            if n:
                p = be.ptr
                la = _abi.JssLookahead(n, p(par), p(act), int(id_base), p(makespan), p(steps), p(rnum))
                sel.call(be.lib, "lookahead", (C.byref(self._desc), C.byref(self._state), C.byref(la)),
                         self.seed if seed is None else int(seed), int(round(explore * 65536)), n_iter, be.stream())
            # the return: reward numerators over the parent's max_time_op (0 where nothing was evaluated)
            if t is not None:
                mto = self.env_const[:, _abi.C_MAX_TIME_OP].to(t.float64)[par.long().clamp(0, max(B - 1, 0))] if B else \
                    t.ones(n, dtype=t.float64, device=be.device)
                ret = t.where(mto > 0, rnum.to(t.float64) / mto.clamp(min=1), t.zeros_like(mto)).to(t.float32)
            else:
                mto = np.asarray(self.env_const)[:, _abi.C_MAX_TIME_OP].astype(np.float64)[np.clip(par, 0, max(B - 1, 0))] if B \
                    else np.ones(n)
                ret = np.where(mto > 0, rnum / np.maximum(mto, 1), 0.0).astype(np.float32)
        return makespan.reshape(shape), steps.reshape(shape), ret.reshape(shape)

    # -- makespan lower bounds of states and of candidate moves (jss_bound, include/jss_bound.h) ----------------------------
    def lower_bound(self, actions=None, parents=None, legal_only: bool = True, job_bound: bool = False, est_start: bool = False):
        """A lower bound of the makespan of EVERY completion of a state, or of a state after one more move: the larger of the
        longest job's earliest end and, per machine, earliest head + remaining work on it + shortest tail (include/jss_bound.h
        defines it; integers, the same bits on every backend).  Where ``lookahead`` pays for a rollout and returns an upper
        bound, this reads the clock, the solution and the instance tables once; the batch is not touched.

        No arguments: the states' own bounds, int32 ``(B,)``.  ``actions="all"``: every column of every env in ``lookahead``'s
        parent-major order, ``(B, jmax + 1)`` -- job a takes its next operation at its earliest start, column J (NOPE) is the
        state's own bound, columns behind J are -1.  ``parents`` / ``actions`` (host or device int sequences of equal length, -1
        = no move): ``(n,)``.  -1 marks what cannot be evaluated: a parent out of range or never reset, an action outside
        [-1, J], a job with no operation left, and -- with ``legal_only`` -- an action that ``action_mask`` does not allow.
        A done env's bound is its makespan.
        ``job_bound=True`` adds the job term alone, ``est_start=True`` the per-operation earliest starts ``(..., jmax, mmax)``
        (a scheduled operation's start, -1 in the padding; rows of refused candidates are -1 throughout): the result is then
        the tuple ``(lower_bound[, job_bound][, est_start])``.  Arrays of the env's backend."""
        self._guard("lower_bound")
        be = self.backend
        lib = library(be, "bound")
        every = isinstance(actions, str)
        if every and (actions != "all" or parents is not None):
            raise ValueError("lower_bound: actions is 'all' (without parents), an array given with parents, or None")
        if not every and (actions is None) != (parents is None):
            raise ValueError("lower_bound: give both parents and actions, actions='all', or neither (the states' own bounds)")
        with be.on_device():
            par, act, shape = self._candidates("lower_bound", parents, actions, every)
            n = int(np.prod(shape))
            lower = be.zeros((n,), "int32")
            jb = be.zeros((n,), "int32") if job_bound else None
            est = self._minus_one(n, self.jmax, self.mmax, want=est_start)
            p = be.ptr
            arg = _abi.JssBound(n, p(par), p(act), p(self.action_mask) if (legal_only and act is not None) else None, p(lower),
                                p(jb), p(est))
            self._launch("lower_bound", lib, "jss_bound", arg, n, (par, act))
        out = (lower.reshape(shape),)
        if job_bound:
            out += (jb.reshape(shape),)
        if est_start:
            out += (est.reshape(shape + (self.jmax, self.mmax)),)
        return out[0] if len(out) == 1 else out

    # -- the exact schedule of a machine order (jss_order_eval, include/jss_order.h) ---------------------------------------------
    def evaluate_order(self, rank=None, parents=None, swaps=None, start: bool = False, tail: bool = False, pairs: Optional[int] = None):
        """The semi-active schedule of an order of the operations on each machine, and its makespan (include/jss_order.h defines
        it; integers, the same bits on every backend).  ``rank`` is int32 ``(B, jmax, mmax)``, one row per env: machine m works
        through its operations ascending by (rank, job, operation index); ``None`` takes the env's own ``solution`` -- the start
        times of a finished schedule are such a rank.  Only the instance tables are read; the batch is not touched.

        No further arguments: every env's row, int32 ``(B,)`` makespans.  ``parents`` (n,): candidate c evaluates env
        ``parents[c]``'s row.  ``swaps=(a, b)`` (two (n,) sequences, or one (n, 2) array) exchanges the ranks of the flat
        operation indices ``j * mmax + k`` first, in the kernel -- the rank tensor is neither copied nor written; (-1, -1) is no
        swap.  -1 marks what is refused (a parent out of range or never reset, a negative rank of a real operation, e.g. an
        unfinished env's solution, a swap index that is out of range, names padding or stands alone), -2 an order that is cyclic
        with the job chains.
        ``start=True`` adds the start times ``(n, jmax, mmax)``, ``tail=True`` the tails (the longest path from an operation's
        end to the end of the schedule), ``pairs=cap`` the neighbourhood ``pair_a, pair_b (n, cap)`` and ``n_pairs (n,)``:
        consecutive critical operations of different jobs on a machine without a gap, by machine and position, -1 behind the
        count, which also counts what did not fit.  Padding and the rows of refused or cyclic candidates are -1 (``n_pairs``
        too).  The result is then the tuple ``(makespan[, start][, tail][, pair_a, pair_b, n_pairs])``.  Arrays of the env's
        backend."""
        self._guard("evaluate_order")
        be = self.backend
        lib = library(be, "order")
        if pairs is not None and int(pairs) < 1:
            raise ValueError("evaluate_order: pairs is the capacity of the pair lists, at least 1")
        J, M = self.jmax, self.mmax
        with be.on_device():
            rk = self._order("evaluate_order", "rank", rank)
            par = None if parents is None else self._ints(parents, 1, "evaluate_order: parents must be 1-d")
            n = self.batch if par is None else int(par.shape[0])
            sa = sb = None
            if swaps is not None:
                if isinstance(swaps, (tuple, list)) and len(swaps) == 2 and np.ndim(swaps[0]) == 1:
                    sa, sb = self._ints(swaps[0]), self._ints(swaps[1])
                else:
                    both = be.as_device(swaps, "int32")
                    if both.ndim != 2 or both.shape[1] != 2:
                        raise ValueError("evaluate_order: swaps is (a, b) with two 1-d sequences, or an (n, 2) array")
                    sa, sb = self._ints(both[:, 0]), self._ints(both[:, 1])
                if tuple(sa.shape) != (n,) or tuple(sb.shape) != (n,):
                    raise ValueError(f"evaluate_order: swaps must name one pair per candidate ({n})")
            mk = self._minus_one(n)
            st, tl = self._minus_one(n, J, M, want=start), self._minus_one(n, J, M, want=tail)
            cap = 0 if pairs is None else int(pairs)
            pa, pb, npairs = self._minus_one(n, cap, want=cap), self._minus_one(n, cap, want=cap), self._minus_one(n, want=cap)
            p = be.ptr
            arg = _abi.JssOrder(n, cap, p(rk), p(par), p(sa), p(sb), p(mk), p(st), p(tl), p(pa), p(pb), p(npairs))
            self._launch("evaluate_order", lib, "jss_order_eval", arg, n, [rk, par, sa, sb])
        out = tuple(x for x in (mk, st, tl, pa, pb, npairs) if x is not None)
        return out[0] if len(out) == 1 else out

    # -- tabu search over machine orders (jss_tabu_search, include/jss_tabu.h; jss_block_search, include/jss_block.h) ------------
    def _tabu_walk(self, what, family, fn, struct, n_info, rank, iters, tenure, target, trace, last, reach=None, log=False):
        """``tabu``, and with a ``reach`` ``tabu_blocks``: the checks, the arguments on the device, the launch, the result"""
        self._guard(what)
        be = self.backend
        lib = library(be, family)
        B, J, M, iters = self.batch, self.jmax, self.mmax, int(iters)
        if not 0 <= iters <= _abi.TABU_MAX_ITERS:
            raise ValueError(f"{what}: iters must be in [0, {_abi.TABU_MAX_ITERS}]")
        if reach is not None and not 0 <= int(reach) <= _abi.BLOCK_MAX_REACH:
            raise ValueError(f"{what}: reach must be in [0, {_abi.BLOCK_MAX_REACH}]")
        with be.on_device():
            rk = self._order(what, "rank", rank)
            tenure_of = self._per_candidate(what, "tenure", tenure, B)
            if tenure_of is None and not 0 <= int(tenure) <= _abi.TABU_MAX_TENURE:
                raise ValueError(f"{what}: tenure must be in [0, {_abi.TABU_MAX_TENURE}]")
            tgt = self._per_candidate(what, "target", target, B)
            if tgt is None and target is not None:
                tgt = be.zeros((B,), "int32")
                tgt += int(target)
            mk, best = self._minus_one(B), self._minus_one(B, J, M)
            info = be.zeros((B, n_info), "int32")
            tr, lr, ml = self._minus_one(B, iters, want=trace), self._minus_one(B, J, M, want=last), self._minus_one(B, iters, 2, want=log)
            p = be.ptr
            reach, log_out = ((), ()) if reach is None else ((int(reach),), (p(ml),))      # (the two fields JssBlock has more)
            arg = struct(iters, 0 if tenure_of is not None else int(tenure), *reach, p(rk), p(tenure_of), p(tgt), p(mk), p(best),
                         p(lr), p(info), p(tr), *log_out)
            self._launch(what, lib, fn, arg, B, [rk, tenure_of, tgt])
        return (mk, best, info) + tuple(x for x in (tr, lr, ml) if x is not None)

    def tabu(self, rank=None, iters: int = 100, tenure=8, target=None, trace: bool = False, last: bool = False):
        """One tabu walk per env, the whole walk in one launch (include/jss_tabu.h defines it; integers, the same bits on every
        backend).  ``rank`` is a machine order as ``evaluate_order`` takes it, int32 ``(B, jmax, mmax)``; ``None`` takes the env's
        own ``solution``.  A move exchanges two adjacent critical operations of different jobs on a machine: every such
        neighbour of the current order is timed, the best one that is not tabu -- or that beats the best schedule of the walk --
        is taken, also when it is worse, and its pair is tabu for the next ``tenure`` moves (an int in [0, 64], or one per env,
        ``(B,)``).  At most ``iters`` moves (up to 65536); ``target`` (None, an int or ``(B,)``) ends a walk once its best
        makespan is <= the target.  Only the instance tables are read; the batch is not touched.

        Returns ``(best_makespan, best_rank, info[, trace][, last_rank])``: ``best_makespan`` (B,) with -1 for a refused row
        (as ``evaluate_order`` refuses it, or a tenure outside [0, 64]) and -2 for a cyclic start; ``best_rank``
        (B, jmax, mmax), the best order as positions on the machines, -1 in the padding and in refused or cyclic rows; ``info``
        (B, 4): stop (0 ``iters`` moves made, 1 no neighbour left: optimal, 2 target reached, -1 / -2), moves, the move that found
        the best, neighbours evaluated; ``trace`` (B, iters): the makespan after every move, -1 behind the last; ``last_rank``:
        the order the walk ended in.  Arrays of the env's backend."""
        return self._tabu_walk("tabu", "tabu", "jss_tabu_search", _abi.JssTabu, _abi.TABU_NI, rank, iters, tenure, target, trace, last)

    def tabu_blocks(self, rank=None, iters: int = 100, tenure=8, target=None, reach: int = 0, trace: bool = False, last: bool = False,
                    log: bool = False):
        """One tabu walk per env over block insertions, the whole walk in one launch (include/jss_block.h defines it; integers,
        the same bits on every backend).  ``rank``, ``iters``, ``tenure`` and ``target`` as in ``tabu``.  A move carries a
        critical operation to the far end of its critical block on the machine (``reach`` > 0: at most that many places, so
        ``reach=1`` leaves the swaps at the blocks' ends); every candidate is scored from the heads and tails of the current
        schedule, the best estimate that is not tabu -- or that beats the best schedule of the walk -- is taken, and only that
        order is re-timed exactly.  Only the instance tables are read; the batch is not touched.

        Returns ``(best_makespan, best_rank, info[, trace][, last_rank][, move_log])``: as ``tabu`` returns them, with ``info``
        (B, 8): stop (0 ``iters`` moves made, 1 no critical machine arc left: optimal, 2 target reached, 3 every candidate
        screened, 4 never, -1 / -2), moves, the move that found the best, candidates scored, candidates screened (they could
        close a cycle), moves of distance >= 2 taken, moves whose estimate was the exact makespan, 0; ``move_log``
        (B, iters, 2): the flat indices of the operation moved and of the block end it passed, -1 behind the last move.
        Arrays of the env's backend."""
        return self._tabu_walk("tabu_blocks", "block", "jss_block_search", _abi.JssBlock, _abi.BLOCK_NI, rank, iters, tenure, target,
                               trace, last, reach, log)

    # -- path relinking between machine orders (jss_relink_walk, include/jss_relink.h) ------------------------------------------
    def relink(self, rank, guide, steps=None, until=0, margin: int = 0, trace: bool = False, last: bool = True, log: bool = False):
        """One walk per env from the machine order ``rank`` towards the machine order ``guide``, the whole walk in one launch
        (include/jss_relink.h defines it; integers, the same bits on every backend).  ``rank`` (B, jmax, mmax) as in
        ``evaluate_order`` (None: the env's own ``solution``), ``guide`` likewise.  A move swaps two operations adjacent on a
        machine that the guide has the other way round, so it lowers the distance -- the number of pairs of operations of one
        machine that the two orders put the other way round -- by one, and every order on the way has a schedule; the swap taken
        is the one with the lowest head and tail estimate among those that surely close no cycle, and only it is re-timed.  The
        walk ends on arrival, once the distance is <= ``until`` (an int or a (B,) array), or after ``steps`` moves (None:
        65 536).  ``margin``: orders nearer than that to either end do not count as the best.  Only the instance tables are read.

        Returns ``(best_makespan, best_rank, last_makespan, last_rank, info[, trace][, move_log])`` (``last=False`` leaves the
        two ``last`` entries None): the lowest makespan on the path (-1 refused, -2 an order without a schedule) and its order as
        positions, the same of the order the walk ended on, ``info`` (B, 8): stop (0 ``steps`` moves made, 1 arrived, 2 ``until``
        reached, 4 never, -1 / -2), moves, the move that gave the best (-1: no order was eligible, the last one is returned), the
        distance at the start, the distance at the end, candidates listed, moves without a sure candidate, candidates swapped
        back; ``trace`` (B, steps) the makespan after every move and ``move_log`` (B, steps, 2) the flat indices of the two
        operations swapped, -1 behind the last move.  Arrays of the env's backend."""
        self._guard("relink")
        be = self.backend
        lib = library(be, "relink")
        B, J, M, margin = self.batch, self.jmax, self.mmax, int(margin)
        steps = _abi.RELINK_MAX_STEPS if steps is None else int(steps)
        if not 0 <= steps <= _abi.RELINK_MAX_STEPS:
            raise ValueError(f"relink: steps must be in [0, {_abi.RELINK_MAX_STEPS}]")
        if margin < 0:
            raise ValueError("relink: margin must be >= 0")
        if guide is None:
            raise ValueError("relink: a guide is needed")
        with be.on_device():
            rk, gd = self._order("relink", "rank", rank), self._order("relink", "guide", guide)
            until_of = self._per_candidate("relink", "until", until, B)
            if until_of is None and int(until) < 0:
                raise ValueError("relink: until must be >= 0")
            mk, best = self._minus_one(B), self._minus_one(B, J, M)
            info = be.zeros((B, _abi.RELINK_NI), "int32")
            lm, lr = self._minus_one(B, want=last), self._minus_one(B, J, M, want=last)
            tr, ml = self._minus_one(B, steps, want=trace), self._minus_one(B, steps, 2, want=log)
            p = be.ptr
            arg = _abi.JssRelink(steps, 0 if until_of is not None else int(until), margin, p(rk), p(gd), p(until_of), p(mk),
                                 p(best), p(lm), p(lr), p(info), p(tr), p(ml))
            self._launch("relink", lib, "jss_relink_walk", arg, B, [rk, gd, until_of])
        return (mk, best, lm, lr, info) + tuple(x for x in (tr, ml) if x is not None)

    def order_distance(self, rank, guide):
        """(B,) int32: per env the number of pairs of operations of one machine that the machine orders ``rank`` and ``guide``
        (as in ``relink``) put the other way round; -1 where either is refused, -2 where either has no schedule.  It is
        ``relink`` with ``steps=0``."""
        out = self.relink(rank, guide, steps=0, last=False)
        mk, info = out[0], out[4]
        be = self.backend
        with be.on_device():
            if getattr(be, "torch", None) is not None:
                return be.torch.where(mk < 0, mk, info[:, 3])
            return np.where(mk < 0, mk, info[:, 3]).astype(np.int32)

    # -- Giffler-Thompson decoding of key tables, one BRKGA generation (include/jss_decode.h) ----------------------------------
    def decode_keys(self, keys, parents=None, delta=1.0, start: bool = False, info: bool = False):
        """Key tables decoded into schedules by Giffler and Thompson's procedure, one decode per candidate in one launch
        (include/jss_decode.h defines it; integers, the same bits on every backend).  ``keys`` is int32 ``(jmax, mmax)`` -- one
        table for every candidate -- or ``(n, jmax, mmax)``, table c for candidate c, on the host or on the device; candidate c
        decodes on the instance of env ``parents[c]`` (``None``: env c, and n == B).  Among the operations in conflict on the
        machine of the earliest possible completion, the one with the largest key goes first (the lowest job index on ties).
        ``delta`` in [0, 1], a float or an ``(n,)`` array of floats, is the delay parameter: 1 gives active schedules (the class
        that always holds an optimum), 0 non-delay schedules, in between Bierwirth and Mattfeld's hybrid; it is converted by
        ``round(delta * 65536)``.  Only the instance tables are read: no env is stepped or written.

        Returns ``makespan`` (n,) int32 (-1 refused: a parent out of range or never reset), then with ``start`` the
        ``(n, jmax, mmax)`` start times (-1 in the padding: a rank tensor for ``evaluate_order``, ``tabu_blocks`` and ``relink``),
        then with ``info`` the ``(n, 4)`` counters (iterations with more than one operation in conflict, the largest conflict
        set, iterations whose chosen operation could not start earliest, 0).  Arrays of the env's backend."""
        self._guard("decode_keys")
        be = self.backend
        lib = library(be, "decode")
        B = self.batch
        with be.on_device():
            k, tables, stride = self._tables("decode_keys", "keys", keys)
            par = None if parents is None else self._ints(parents, 1, "decode_keys: parents must have shape (n,)")
            n = int(par.shape[0]) if par is not None else tables if tables is not None else B
            if tables is not None and tables != n:
                raise ValueError(f"decode_keys: {tables} key tables for {n} candidates")
            if par is None and n != B:
                raise ValueError(f"decode_keys: without parents there is one candidate per env ({B}), got {n}")
            delta_of, delta_q16 = self._per_candidate("decode_keys", "delta", delta, n, scale=65536), 0
            if delta_of is None:
                if not 0.0 <= float(delta) <= 1.0:
                    raise ValueError("decode_keys: delta must lie in [0, 1]")
                delta_q16 = int(round(float(delta) * 65536))
            mk = self._minus_one(n)
            st = self._minus_one(n, self.jmax, self.mmax, want=start)
            nf = be.zeros((n, _abi.DECODE_NI), "int32") if info else None
            p = be.ptr
            arg = _abi.JssDecode(n, stride, delta_q16, p(par), p(k), p(delta_of), p(mk), p(st), p(nf))
            self._launch("decode_keys", lib, "jss_decode_keys", arg, n, [k, par, delta_of])
        out = tuple(x for x in (mk, st, nf) if x is not None)
        return out[0] if len(out) == 1 else out

    def evolve_keys(self, keys, fitness, pop: int, elite: int, mutants: int, rho: float = 0.7, generation: int = 1, seed=None):
        """One generation of a biased random-key genetic algorithm over key tables, on the device (``jss_keys_evolve``,
        include/jss_decode.h; integers, the same bits on every backend).  ``keys`` is int32 ``(G * pop, ...)``: G groups of
        ``pop`` individuals, every row one individual (its trailing axes are flattened); ``fitness`` int32 ``(G * pop,)``, lower
        is better, a negative value (a refused decode) behind every other.  Of every group the ``elite`` best are copied, the
        last ``mutants`` rows are drawn anew, and every row between is a crossover of a random elite and a random non-elite
        individual, each entry from the elite parent with probability ``rho``.  ``elite=0, mutants=pop`` draws an initial
        population: ``keys`` is then the shape ``(G * pop, ...)`` (or an array of that shape) and ``fitness`` may be None.
        ``seed`` None: the env's own.  Returns ``(keys_out, by_rank)``: the new rows in the shape of ``keys`` and ``(G * pop,)``
        the individuals of every group from best to worst."""
        be = self.backend
        lib = library(be, "decode")
        P, ne, nm, generation = int(pop), int(elite), int(mutants), int(generation)
        if not 0.0 <= float(rho) <= 1.0:
            raise ValueError("evolve_keys: rho must lie in [0, 1]")
        if not 1 <= P <= _abi.EVOLVE_MAX_POP:
            raise ValueError(f"evolve_keys: pop must lie in [1, {_abi.EVOLVE_MAX_POP}]")
        if ne < 0 or nm < 0 or ne + nm > P or (ne + nm < P and ne < 1):
            raise ValueError("evolve_keys: elite + mutants <= pop, and a crossover needs an elite")
        fresh = ne == 0 and nm == P
        with be.on_device():
            if fresh and (isinstance(keys, (tuple, list)) and all(isinstance(x, (int, np.integer)) for x in keys)):
                shape, k = tuple(int(x) for x in keys), None
            else:
                k = self._ints(keys)
                shape = tuple(k.shape)
            if len(shape) < 2 or shape[0] % P or int(np.prod(shape[1:])) < 1:
                raise ValueError(f"evolve_keys: keys must have shape (G * {P}, ...), got {shape}")
            G, region = shape[0] // P, int(np.prod(shape[1:]))
            fit = None
            if not fresh:
                if fitness is None:
                    raise ValueError("evolve_keys: fitness is needed unless elite == 0 and mutants == pop")
                fit = self._ints(fitness, (G * P,), f"evolve_keys: fitness must have shape {(G * P,)}")
            out = be.zeros(shape, "int32")
            by_rank = be.zeros((G * P,), "int32")
            p = be.ptr
            arg = _abi.JssEvolve(G, P, region, ne, nm, int(round(float(rho) * 65536)), generation,
                                 int(self.seed if seed is None else seed) & (2 ** 64 - 1), p(fit), p(None if fresh else k), p(out),
                                 p(by_rank))
            self._launch("evolve_keys", lib, "jss_keys_evolve", arg, G, [k, fit], with_env=False)
        return out, by_rank

    # -- one-machine relaxations of partial selections, the shifting bottleneck construction (include/jss_machine.h) ------------
    def _fixed_masks(self, fixed, n, what):
        """``fixed`` -- an int, ``(n,)`` integers or a boolean ``(n, M)`` array -- as ``(n,)`` uint64 machine masks on the host"""
        if hasattr(fixed, "detach"):
            fixed = fixed.detach().cpu().numpy()
        if isinstance(fixed, (int, np.integer)):
            if not 0 <= int(fixed) < 2 ** 64:
                raise ValueError(f"{what}: fixed must be a 64-bit machine mask")
            return np.full(n, int(fixed), np.uint64)
        a = np.asarray(fixed)
        if a.dtype == np.bool_:
            if a.ndim != 2 or a.shape[0] != n or a.shape[1] > 64:
                raise ValueError(f"{what}: a boolean fixed must have shape ({n}, M)")
            return (a.astype(np.uint64) << np.arange(a.shape[1], dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
        if a.dtype.kind not in "iu" or a.shape != (n,):
            raise ValueError(f"{what}: fixed must be an int, {(n,)} integers or a boolean ({n}, M) array")
        if a.dtype.kind == "i" and (a < 0).any() and a.dtype != np.int64:      # (a negative int64 is a mask with bit 63 set)
            raise ValueError(f"{what}: fixed must not be negative")
        return a.astype(np.int64).view(np.uint64) if a.dtype.kind == "i" else a.astype(np.uint64)

    def _machine_call_start(self, what, parents, tables, fixed):
        """what relax_machines and bottleneck have in common: the checks, the parents on the device, n"""
        self._guard(what)
        par = None if parents is None else self._ints(parents, 1, f"{what}: parents must have shape (n,)")
        fixed_n = None
        if fixed is not None and not isinstance(fixed, (int, np.integer)):
            fixed_n = int(fixed.shape[0]) if hasattr(fixed, "shape") else len(fixed)
        n = int(par.shape[0]) if par is not None else tables if tables is not None else fixed_n if fixed_n is not None else self.batch
        if par is None and n != self.batch:
            raise ValueError(f"{what}: without parents there is one candidate per env ({self.batch}), got {n}")
        return par, n

    def _selection(self, what, rank, fixed, n):
        """the machines of a partial selection as the int64 masks the libraries take, None while nothing is fixed"""
        masks = self._fixed_masks(fixed, n, what)
        if rank is None and masks.any():
            raise ValueError(f"{what}: a fixed machine needs a rank")
        return self.backend.from_numpy(masks.view(np.int64)) if masks.any() else None

    def _relaxation(self, what, family, fn, struct, rank, fixed, parents, per_machine, tables, nodes=None, proved=None):
        """``relax_machines``, and with ``nodes`` ``solve_machines``: ``per_machine`` and ``tables`` say which of the
        ``(n, mmax)`` and ``(n, jmax, mmax)`` outputs are wanted, ``proved`` -- between them -- whether its ``(n,)`` int64 is"""
        be = self.backend
        lib = library(be, family)
        if nodes is not None and not 1 <= int(nodes) <= _abi.CARLIER_MAX_NODES:
            raise ValueError(f"{what}: nodes must lie in [1, {_abi.CARLIER_MAX_NODES}]")
        with be.on_device():
            r, r_n, stride = self._tables(what, "rank", rank) if rank is not None else _NO_TABLE
            par, n = self._machine_call_start(what, parents, r_n, fixed)
            if r_n is not None and r_n != n:
                raise ValueError(f"{what}: {r_n} rank tables for {n} candidates")
            fx = self._selection(what, r, fixed, n)
            length, lower, neck = self._minus_one(n), self._minus_one(n), self._minus_one(n)
            rows = [self._minus_one(n, self.mmax, want=want) for want in per_machine] + \
                   ([] if proved is None else [be.zeros((n,), "int64") if proved else None]) + \
                   [self._minus_one(n, self.jmax, self.mmax, want=want) for want in tables]
            p = be.ptr
            arg = struct(n, stride, *(() if nodes is None else (int(nodes), 0)), p(par), p(r), p(fx), p(length), p(lower), p(neck),
                         *(p(x) for x in rows))
            self._launch(what, lib, fn, arg, n, [r, par, fx])
        return (lower, length, neck) + tuple(x for x in rows if x is not None)

    def relax_machines(self, rank=None, fixed=0, parents=None, jps: bool = False, schrage: bool = False, head: bool = False,
                       tail: bool = False, rank_out: bool = False):
        """The one-machine relaxations of a partial selection, one per candidate in one launch (include/jss_machine.h defines
        them; integers, the same bits on every backend).  Candidate c looks at the instance of env ``parents[c]`` (``None``: env
        c, and n == B).  ``fixed`` says which machines are sequenced: an int (one mask for all, bit m for machine m), ``(n,)``
        integers or a boolean ``(n, M)`` array; ``rank`` is int32 ``(jmax, mmax)`` -- one table for all -- or ``(n, jmax, mmax)``
        and orders the operations of the fixed machines as in ``evaluate_order``; it may be None while nothing is fixed.  Only
        the instance tables are read.

        Returns ``(lower_bound, length, bottleneck)``, each (n,) int32: ``length`` the longest path of the partial selection (-1
        refused, -2 cyclic), ``lower_bound`` the larger of it and the free machines' Jackson preemptive bounds, ``bottleneck``
        the free machine with the largest one (-1: none is free).  Then, each where asked for and in this order: ``jps`` and
        ``schrage`` (n, mmax), -1 for fixed and unused machines; ``head`` and ``tail`` (n, jmax, mmax); ``rank_out`` (n, jmax,
        mmax): ``rank`` with the free machines' operations at their Schrage starts, so that one more bit of ``fixed`` sequences
        that machine.  Arrays of the env's backend."""
        return self._relaxation("relax_machines", "machine", "jss_machine_relax", _abi.JssMachineRelax, rank, fixed, parents,
                                (jps, schrage), (head, tail, rank_out))

    def _build(self, what, family, fn, struct, n_info, parents, bias, reopt, rank, fixed, order, nodes=None):
        """``bottleneck``, and with ``nodes`` ``bottleneck_exact``"""
        be = self.backend
        lib = library(be, family)
        if not 0 <= int(reopt) <= _abi.BOTTLENECK_MAX_REOPT:
            raise ValueError(f"{what}: reopt must lie in [0, {_abi.BOTTLENECK_MAX_REOPT}]")
        if nodes is not None and not 1 <= int(nodes) <= _abi.CARLIER_MAX_NODES:
            raise ValueError(f"{what}: nodes must lie in [1, {_abi.CARLIER_MAX_NODES}]")
        if (rank is None) != (fixed is None):
            raise ValueError(f"{what}: rank and fixed are given together")
        J, M = self.jmax, self.mmax
        with be.on_device():
            r = None
            if rank is not None:
                r = self._ints(rank)
                if len(r.shape) != 3 or tuple(r.shape[1:]) != (J, M):
                    raise ValueError(f"{what}: rank must have shape (n, {J}, {M}), got {tuple(r.shape)}")
            par, n = self._machine_call_start(what, parents, int(r.shape[0]) if r is not None else None, fixed)
            if r is not None and int(r.shape[0]) != n:
                raise ValueError(f"{what}: {int(r.shape[0])} rank tables for {n} candidates")
            fx = None if fixed is None else be.from_numpy(self._fixed_masks(fixed, n, what).view(np.int64))
            bs = None if bias is None else self._ints(bias, (n, M), f"{what}: bias must have shape {(n, M)}", got=True)
            mk, out = self._minus_one(n), self._minus_one(n, J, M)
            info = be.zeros((n, n_info), "int32")
            fixed_order = self._minus_one(n, M, want=order)
            p = be.ptr
            arg = struct(n, int(reopt), *(() if nodes is None else (int(nodes), 0)), p(par), p(r), p(fx), p(bs), p(mk), p(out), p(info),
                         p(fixed_order))
            self._launch(what, lib, fn, arg, n, [r, par, fx, bs])
        return (mk, out, info, fixed_order) if order else (mk, out, info)

    def bottleneck(self, parents=None, bias=None, reopt: int = 1, rank=None, fixed=None, order: bool = False):
        """A shifting bottleneck construction per candidate, all in one launch (``jss_bottleneck_build``, include/jss_machine.h;
        integers, the same bits on every backend): relax, sequence the machine with the largest Jackson preemptive bound by
        Schrage's schedule, re-sequence every machine fixed before ``reopt`` times (in [0, 8]), until every machine is
        sequenced.  Candidate c builds on the instance of env ``parents[c]`` (``None``: env c, and n == B).  ``bias`` is int32
        ``(n, mmax)`` or None: added to the machines' bounds when the bottleneck is chosen, so that candidates of one instance
        build different schedules.  ``rank`` (n, jmax, mmax) and ``fixed`` (as in ``relax_machines``), given together, let a
        build go on from a partial selection.  Only the instance tables are read.

        Returns ``(makespan, rank, info)``: (n,) int32 (-1 refused, -2 a selection turned cyclic, which durations of 0 can
        cause), the (n, jmax, mmax) machine orders (a rank tensor for ``evaluate_order``, ``tabu_blocks`` and ``relink``) and the
        (n, 4) counters (machines fixed, re-sequencings tried, re-sequencings that shortened the schedule, the lower bound of the
        first relaxation); with ``order`` also the (n, mmax) machines in the order they were fixed, -1 behind them."""
        return self._build("bottleneck", "machine", "jss_bottleneck_build", _abi.JssBottleneck, _abi.BOTTLENECK_NI, parents, bias,
                           reopt, rank, fixed, order)

    # -- Carlier's one-machine search, shifting bottleneck constructions sequenced by it (include/jss_carlier.h) ----------------
    def solve_machines(self, rank=None, fixed=0, parents=None, nodes: int = 256, opt: bool = False, low: bool = False,
                       nodes_used: bool = False, proved: bool = False, head: bool = False, tail: bool = False, rank_out: bool = False):
        """``relax_machines`` with every free machine's one-machine problem solved by Carlier's branch and bound within ``nodes``
        search nodes per machine (in [1, 4096]), one candidate per wavefront in one launch (``jss_machine_solve``,
        include/jss_carlier.h defines the search; integers, the same bits on every backend).  ``rank``, ``fixed`` and ``parents``
        are ``relax_machines``'s.

        Returns ``(lower_bound, length, bottleneck)``, each (n,) int32: ``length`` as there (-1 refused, -2 cyclic),
        ``lower_bound`` the larger of it and the free machines' ``low``, ``bottleneck`` the free machine with the largest ``low``.
        Then, each where asked for and in this order: ``opt`` (the best schedule's value, the optimum where proved), ``low`` (opt
        where proved, else Jackson's preemptive bound) and ``nodes_used`` (n, mmax), -1 for fixed and unused machines; ``proved``
        (n,) int64, bit m set where machine m's search ended within the budget; ``head`` and ``tail`` (n, jmax, mmax);
        ``rank_out`` (n, jmax, mmax): ``rank`` with the free machines' operations at the starts of their best schedule.  With
        ``nodes=1`` the best schedule is Schrage's.  Arrays of the env's backend."""
        return self._relaxation("solve_machines", "carlier", "jss_machine_solve", _abi.JssMachineSolve, rank, fixed, parents,
                                (opt, low, nodes_used), (head, tail, rank_out), nodes, bool(proved))

    def bottleneck_exact(self, parents=None, bias=None, reopt: int = 1, nodes: int = 256, rank=None, fixed=None, order: bool = False):
        """``bottleneck`` with every machine sequenced by the best schedule of Carlier's branch and bound (at most ``nodes`` search
        nodes per one-machine problem, in [1, 4096]) instead of Schrage's: the shifting bottleneck procedure with exact
        one-machine solutions, all candidates in one launch (``jss_bottleneck_exact``, include/jss_carlier.h; integers, the same
        bits on every backend).  The arguments are ``bottleneck``'s; ``nodes=1`` builds what it builds.  ta01 unbiased: 1512 / 1345
        / 1352 at reopt 0 / 1 / 3 where ``bottleneck`` gives 1633 / 1475 / 1402.

        Returns ``(makespan, rank, info)`` as ``bottleneck`` does, ``info`` (n, 8): its four counters (the lower bound from the
        searches' ``low``), then the nodes of all searches, the most nodes of one problem, the problems left open by the budget and
        the sequences replaced by Schrage's because they closed a cycle; with ``order`` also the (n, mmax) machines in the order
        they were fixed."""
        return self._build("bottleneck_exact", "carlier", "jss_bottleneck_exact", _abi.JssBottleneckExact, _abi.EXACT_NI, parents, bias,
                           reopt, rank, fixed, order, nodes)

    # -- constraint propagation on operation windows (include/jss_propagate.h) -------------------------------------------------------
    def propagate(self, ub, rank=None, fixed=0, parents=None, est=None, lct=None, hyp=None, passes: int = 256, windows: bool = False):
        """Constraint propagation on the windows [earliest start, latest completion] of every operation of a partial selection
        under the trial makespan ``ub``, one candidate per wavefront in one launch (``jss_propagate``; include/jss_propagate.h
        defines the rules and their Jacobi passes; integers, the same bits on every backend).  ``rank``, ``fixed`` and ``parents``
        are ``relax_machines``'s.  ``ub`` is an int or ``(n,)``; ``est`` and ``lct``, given together, are windows to start from,
        int32 ``(jmax, mmax)`` -- one table for all -- or ``(n, jmax, mmax)``; ``hyp`` is a tuple of three ``(n,)`` arrays, the
        flat index ``j * mmax + k`` of one operation per candidate (-1: none) and the window it is held to; ``passes`` lies in
        [1, 4096].

        Returns ``(status, passes_used)``, each (n,) int32 -- status 0: a fixpoint, 1: refuted (no schedule of the selection with
        a makespan of at most ``ub`` exists under the hypothesis), 2: the budget of passes is spent, -1 refused, -2 cyclic -- and
        with ``windows`` also ``est`` and ``lct`` (n, jmax, mmax), -1 in the padding and in the rows of candidates that did not
        end with status 0 or 2.  Arrays of the env's backend."""
        be = self.backend
        lib = library(be, "propagate")
        if not 1 <= int(passes) <= _abi.PROPAGATE_MAX_PASSES:
            raise ValueError(f"propagate: passes must lie in [1, {_abi.PROPAGATE_MAX_PASSES}]")
        if (est is None) != (lct is None):
            raise ValueError("propagate: est and lct are given together")
        if hyp is not None and len(hyp) != 3:
            raise ValueError("propagate: hyp is a tuple of three (n,) arrays: the operation, its est and its lct")
        with be.on_device():
            r, r_n, r_stride = self._tables("propagate", "rank", rank) if rank is not None else _NO_TABLE
            e_in, e_n, e_stride = self._tables("propagate", "est", est) if est is not None else _NO_TABLE
            l_in, l_n, _ = self._tables("propagate", "lct", lct) if lct is not None else _NO_TABLE
            if e_n != l_n:
                raise ValueError("propagate: est and lct must have the same shape")
            counts = [c for c in (r_n, e_n) if c is not None]
            if np.ndim(ub) == 1:
                counts.append(len(ub))
            if hyp is not None:
                counts.append(len(hyp[0]))
            par, n = self._machine_call_start("propagate", parents, counts[0] if counts else None, fixed)
            if any(x != n for x in counts):
                raise ValueError(f"propagate: {counts} tables or entries for {n} candidates")
            fx = self._selection("propagate", r, fixed, n)

            def row(x, what):
                if hasattr(x, "detach") and getattr(be, "torch", None) is not None and x.dtype == be.torch.int32:
                    if tuple(x.shape) != (n,):                         # (an int32 tensor stays where it is: no copy through the host)
                        raise ValueError(f"propagate: {what} must be {(n,)} integers")
                    return be.as_device(x, "int32")
                x = np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x)
                if x.ndim == 0 and what == "ub":
                    x = np.full(n, int(x))
                if x.shape != (n,) or x.dtype.kind not in "iu":
                    raise ValueError(f"propagate: {what} must be {(n,)} integers")
                if x.size and (x.min() < -2 ** 31 or x.max() >= 2 ** 31):
                    raise ValueError(f"propagate: {what} must fit 32 bits")
                return be.from_numpy(np.ascontiguousarray(x, dtype=np.int32))

            u = row(ub, "ub")
            h = [None] * 3 if hyp is None else [row(x, "hyp") for x in hyp]
            status, used = self._minus_one(n), self._minus_one(n)
            e_out, l_out = self._minus_one(n, self.jmax, self.mmax, want=windows), self._minus_one(n, self.jmax, self.mmax, want=windows)
            p = be.ptr
            arg = _abi.JssPropagate(n, r_stride, e_stride, int(passes), p(par), p(r), p(fx), p(u), p(e_in), p(l_in), p(h[0]), p(h[1]),
                                    p(h[2]), p(status), p(used), p(e_out), p(l_out))
            self._launch("propagate", lib, "jss_propagate", arg, n, [r, par, fx, u, e_in, l_in] + h)
        return (status, used, e_out, l_out) if windows else (status, used)
