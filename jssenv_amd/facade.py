"""The single-env view with the reference's exact surface: ``JssEnv`` (JSSEnv/envs/jss_env.py: ``reset() -> obs``,
``step(a) -> (obs, reward, done, False, {})``, ``get_legal_actions()``, ``increase_time_step()``, ``render()`` and the public
attributes its tests and dispatching rules read) over a ``BatchedJssEnv`` of one env, and ``make('jss-v1', ...)``.
"""
from __future__ import annotations

import os

import numpy as np

from . import _abi
from .env import BatchedJssEnv, play_to_end
from .instances import resolve_instance


class _Snap:
    """Env 0 of a host snapshot, decoded lazily: ``step()`` needs the observation, mask, reward, done and the error
    bits; everything else (the per-job arrays the reference exposes as attributes) is unpacked when it is read."""

    def __init__(self, t, J, M, decode):
        self.t, self.J, self.M, self.c, self.decode = t, J, M, {}, decode

    def __contains__(self, k):
        return k in self.c

    def __setitem__(self, k, v):
        self.c[k] = v

    def __getitem__(self, k):
        c = self.c
        if k in c:
            return c[k]
        t, J, M = self.t, self.J, self.M
        if k in ("clock", "err", "noop_flag", "episode", "step_in_episode"):
            hdr = t["env_header"][0]
            st = int(hdr[_abi.H_STATUS])
            c.update(clock=int(hdr[_abi.H_CLOCK]), err=st & 0xFF, noop_flag=bool(st & _abi.STATUS_NOOP),
                     episode=int(hdr[_abi.H_EPISODE]), step_in_episode=int(hdr[_abi.H_STEP]))
        elif k in ("job_state", "next_op", "next2_op", "blocked"):
            js, nxt, nxt2 = self.decode(t["job_state"][0], 0)
            c.update(job_state=js, next_op=nxt, next2_op=nxt2, blocked=(js[7] & 2) != 0)
        elif k == "tm":
            c[k] = (t["machine_state"][0, :M].astype(np.int64) if "machine_state" in t else
                    BatchedJssEnv.clocks_from_jobs(self["job_state"], M))
        elif k == "mask":
            c[k] = t["action_mask"][0, :J + 1] != 0
        elif k == "obs":
            c[k] = t["real_obs"][0, :J].copy()
        elif k == "reward":
            c[k] = float(t["reward"][0])
        elif k == "done":
            c[k] = bool(t["done"][0])
        elif k == "makespan":
            c[k] = int(t["makespan"][0])
        elif k == "counters":
            c[k] = t["counters"][0].copy()
        elif k == "mask_padding":
            c[k] = t["action_mask"][0, J + 1:].copy()
        elif k == "obs_padding":
            c[k] = t["real_obs"][0, J:].copy()
        else:
            raise KeyError(k)
        return c[k]


def gymnasium_base(which: str = "Env"):
    """``gymnasium.Env`` (or ``gymnasium.vector.VectorEnv``) when gymnasium is importable and really has that class,
    ``object`` otherwise: the reference's env IS a ``gym.Env`` (jss_env.py:14) and gymnasium's wrappers assert
    ``isinstance(env, gymnasium.Env)``; without gymnasium the package works all the same."""
    try:
        import gymnasium
        base = getattr(gymnasium, "Env", None) if which == "Env" else getattr(getattr(gymnasium, "vector", None), "VectorEnv", None)
        return base if isinstance(base, type) else object
    except Exception:
        return object


class JssEnv(gymnasium_base("Env")):
    """Drop-in for ``JSSEnv.envs.jss_env.JssEnv``: one env (B = 1) on the GPU (a ``gymnasium.Env`` when gymnasium exists).

    Same constructor argument (``env_config={'instance_path': ...}``, default ta80 as at
    jss_env.py:35-38), same methods and return shapes, same public attributes (NumPy, pulled
    from the device on access).  Differences, all outside what the reference defines:
    a job action outside the mask raises ``ValueError`` (the reference corrupts its counters
    silently); the observation is float32.  ``device='cpu'`` runs the same env on the
    host-core twin (no GPU needed).
    """

    metadata = {"render_modes": ["human"]}

    def __init__(self, env_config=None, device=None, _backend=None):
        if env_config is None:
            env_config = {"instance_path": "ta80"}                         # jss_env.py:35-38
        inst = resolve_instance(env_config["instance_path"])
        self.instance = inst
        self.jobs, self.machines = inst.jobs, inst.machines                # :77
        self.instance_matrix = inst.instance_matrix                        # :78,:85
        self.jobs_length = inst.jobs_length                                # :87
        self.max_time_op = inst.max_time_op                                # :86
        self.max_time_jobs = inst.max_time_jobs                            # :89
        self.sum_op = inst.sum_op                                          # :88
        self.last_time_step = float("inf")                                 # :53
        self.last_solution = None                                          # :52
        import datetime
        import random
        self.start_timestamp = datetime.datetime.now().timestamp()         # :70 (render's time origin, :672)
        self.colors = [tuple(random.random() for _ in range(3)) for _ in range(self.machines)]   # :99-101, used by render :686
        self._alloc_log = []        # the job actions of this episode in call order (next_jobs: who queued an event first)
        self._alloc_log_ok = True   # False once the episode was advanced by a device-side rollout (no per-call log)
        # on the GPU the env's arena (state + outputs, ~1 KB) lives in page-locked host memory the kernel works on in
        # place: step() = one launch + one stream synchronisation, nothing is copied (JSSENV_AMD_HOST_ARENA=0: device
        # memory and one device -> host copy per step, the round-3 form)
        self._b = BatchedJssEnv([inst], batch=1, device=device, _backend=_backend,
                                host_arena=os.environ.get("JSSENV_AMD_HOST_ARENA", "1") != "0")
        self._cache = None
        self._act = np.zeros(1, dtype=np.int32)
        # remaining work of job j from op k on (MWR / LWR / CR on the host): suffix sums of the durations
        self._remaining = np.cumsum(inst.duration[:, ::-1], axis=1)[:, ::-1].astype(np.int64)
        self._act_pinned, self._zero_copy, self._fast = None, False, None
        be = self._b.backend
        if getattr(be, "name", "") == "hip":
            self._act_pinned = be.torch.zeros(1, dtype=be.torch.int32).pin_memory()
            # JSSENV_AMD_ZEROCOPY=1: jss_step reads the action straight from the pinned host word (one H2D copy less per step)
            self._zero_copy = os.environ.get("JSSENV_AMD_ZEROCOPY", "0") == "1"
        try:  # spaces only when gymnasium is importable (jss_env.py:97, :112-119)
            import gymnasium as gym
            self.action_space = gym.spaces.Discrete(self.jobs + 1)
            self.observation_space = gym.spaces.Dict({
                "action_mask": gym.spaces.Box(0, 1, shape=(self.jobs + 1,)),
                "real_obs": gym.spaces.Box(low=0.0, high=1.0, shape=(self.jobs, 7), dtype=float),
            })
        except ImportError:  # gymnasium is optional
            self.action_space = self.observation_space = None

    # -- host mirror of the device state ---------------------------------------------------
    def _h(self):
        if self._cache is None:                    # one device -> host copy per step (the env's arena), decoded lazily
            self._cache = _Snap(self._b.host_tensors(), self.jobs, self.machines, self._b.decode_jobs)
        return self._cache

    def _solution(self):
        h = self._h()
        if "solution" not in h:                    # the start-time table comes over only when somebody reads it
            b = self._b
            h["solution"] = b.backend.numpy(b.solution[0])[:self.jobs, :self.machines].astype(np.int64)
        return h["solution"]

    def _obs(self):
        h = self._h()
        return {"real_obs": h["obs"], "action_mask": h["mask"]}

    current_time_step = property(lambda s: s._h()["clock"])
    todo_time_step_job = property(lambda s: s._h()["job_state"][_abi.F_TODO])
    needed_machine_jobs = property(lambda s: s._h()["job_state"][_abi.F_CUR] >> 16)
    time_until_finish_current_op_jobs = property(lambda s: s._h()["job_state"][_abi.F_LEFT])
    total_perform_op_time_jobs = property(lambda s: s._h()["job_state"][_abi.F_PERF])
    total_idle_time_jobs = property(lambda s: s._h()["job_state"][_abi.F_IDLE])
    idle_time_jobs_last_op = property(lambda s: s._h()["job_state"][_abi.F_IDLE_LAST])
    time_until_available_machine = property(lambda s: s._h()["tm"])
    solution = property(lambda s: s._solution())
    legal_actions = property(lambda s: s._h()["mask"])
    action_illegal_no_op = property(lambda s: s._h()["blocked"])
    state = property(lambda s: s._h()["obs"])
    err = property(lambda s: s._h()["err"])

    @property
    def nb_legal_actions(self):            # stored counter in the reference; a popcount here
        return int(self.legal_actions[:-1].sum())

    @property
    def machine_legal(self):               # reference :173-179, :463, :632-634
        out = np.zeros(self.machines, dtype=bool)
        need = self.needed_machine_jobs
        out[need[self.legal_actions[:-1]]] = True
        return out

    @property
    def nb_machine_legal(self):
        return int(self.machine_legal.sum())

    @property
    def next_time_step(self):              # the reference's sorted event list (:449-453, :517)
        tm = self.time_until_available_machine
        return sorted({int(self.current_time_step + v) for v in tm if v > 0})

    @property
    def next_jobs(self):
        """The reference's list parallel to ``next_time_step`` (jss_env.py:56, :156, :453, :518): entry i is the job whose
        allocation QUEUED event time ``next_time_step[i]`` -- the first job allocated to finish at that time; a later job
        that finishes at the same time adds nothing (:450-453).  Derived: the running ops (start = solution[j][todo[j]],
        end = start + duration > now) sorted by end time; among ops that end together the one allocated first -- the
        earlier start, then the earlier ``step`` call of this episode (the facade logs its job actions; after a device-side
        rollout there is no log and the lower job index stands in)."""
        now = self.current_time_step
        left, todo = self.time_until_finish_current_op_jobs, self.todo_time_step_job
        running = [j for j in range(self.jobs) if left[j] > 0]
        if not running:
            return []
        sol = self._solution()
        rank = {}
        if self._alloc_log_ok:
            for pos, j in enumerate(self._alloc_log):
                rank[j] = pos                                # the LAST allocation of job j is its running op
        first = {}
        for j in running:
            end = int(now + left[j])
            key = (int(sol[j][todo[j]]), rank.get(j, len(self._alloc_log) + j), j)
            if end not in first or key < first[end][0]:
                first[end] = (key, j)
        return [first[t][1] for t in sorted(first)]

    @property
    def illegal_actions(self):             # (M, J) matrix of the reference (:171, :427, :464-467)
        out = np.zeros((self.machines, self.jobs), dtype=bool)
        need, bl = self.needed_machine_jobs, self.action_illegal_no_op
        for j in range(self.jobs):
            if bl[j] and need[j] >= 0:
                out[need[j], j] = True
        return out

    # -- reference API -----------------------------------------------------------------------
    def get_legal_actions(self):           # jss_env.py:136-143
        return self.legal_actions

    def reset(self, *, seed=None, options=None):
        """jss_env.py:145-181 -- returns the observation dict only (no info tuple)."""
        self._b.reset()
        self._cache = None
        self._alloc_log, self._alloc_log_ok = [], True
        return self._obs()

    def _raise_for(self, err, action=None):
        """Turn the kernel's per-env error bits into the reference's exceptions.  The bits are sticky on the
        device, so they are cleared here: every offending call raises, not only the first of an episode."""
        if not err:
            return
        self._b.clear_errors()
        self._cache = None
        if err & _abi.ERR_ILLEGAL_ACTION and self._alloc_log and self._alloc_log[-1] == action:
            self._alloc_log.pop()                  # the job was not allocated
        if err & _abi.ERR_BAD_ACTION:
            raise IndexError(f"action {action} out of range for {self.jobs} jobs")
        if err & _abi.ERR_NOPE_IDLE:
            raise IndexError("pop from empty list")  # what the reference raises at jss_env.py:517
        if err & _abi.ERR_ILLEGAL_ACTION:
            raise ValueError(f"job {action} is not a legal action")

    def step(self, action):
        """jss_env.py:403-481."""
        action = int(action)
        if 0 <= action < self.jobs:
            self._alloc_log.append(action)         # (an action the mask refuses raises below and queues nothing: popped there)
        if getattr(self._b, "host_arena", False):  # GPU, arena in host memory: the action word is part of it
            return self._step_host_arena(action)
        elif self._act_pinned is not None:         # GPU: the action goes out through a pinned word, nothing is allocated
            self._act_pinned[0] = action
            b = self._b
            if self._zero_copy:                    # the kernel reads the pinned word itself
                b.step_raw(self._act_pinned.data_ptr())
            else:
                b._act_in.copy_(self._act_pinned, non_blocking=True)
                b.step_raw(b._act_in.data_ptr())
        else:
            self._act[0] = action
            self._b.step(self._act)
        self._cache = None
        h = self._h()
        self._raise_for(h["err"], action)
        if h["done"]:                                                       # :649-652
            self.last_time_step = h["clock"]
            self.last_solution = self._solution()
        return self._obs(), h["reward"], h["done"], False, {}

    def _step_host_arena(self, action):
        """step() when the env's arena is page-locked host memory: the action is written into it, ONE launch works on it
        in place, one stream synchronisation (through the library: it also surfaces a kernel fault), and the results are
        read where they lie.  Everything that does not change between calls is bound once."""
        fp = self._fast
        if fp is None:
            b, be = self._b, self._b.backend
            if not b._is_reset:
                raise RuntimeError("call reset() before step()")
            lib, (d, s, o) = be.lib, b._refs()
            views = b.host_tensors()
            # torch's current stream of the env's device as a raw handle: the private accessor costs 0.3 us, building a
            # torch.cuda.Stream object to ask for its .cuda_stream 3 us (tools/gpu_facade_floor.py)
            raw = getattr(be.torch._C, "_cuda_getCurrentRawStream", None)
            index = be.device.index
            stream_of = (lambda: raw(index)) if raw is not None else (lambda: be.torch.cuda.current_stream(be.device).cuda_stream)
            fp = self._fast = (b._act_in.numpy(), lib.jss_step, lib.jss_sync_check, d, s, o, b._act_in.data_ptr(),
                               stream_of, views, lib, b)
        act, jss_step, sync_check, d, s, o, a_ptr, stream_of, views, lib, b = fp
        act[0] = action
        stream = stream_of()
        rc = jss_step(d, s, a_ptr, o, stream)
        if rc == 0:
            rc = sync_check(stream)
        if rc:
            _abi.check(lib, rc, "jss_step")
        h = self._cache = _Snap(views, self.jobs, self.machines, b.decode_jobs)
        err = h["err"]
        if err:
            self._raise_for(err, action)
        done = h["done"]
        if done:                                                            # :649-652
            self.last_time_step = h["clock"]
            self.last_solution = self._solution()
        return {"real_obs": h["obs"], "action_mask": h["mask"]}, h["reward"], done, False, {}

    def increase_time_step(self):
        """jss_env.py:495-637 -- public in the reference and called directly by its tests."""
        hole = int(self._b.backend.numpy(self._b.increase_time_step())[0])
        self._cache = None
        self._raise_for(self._h()["err"])
        return hole

    def lower_bound(self) -> int:
        """A lower bound of the makespan of every completion of the current state (``BatchedJssEnv.lower_bound``,
        include/jss_bound.h): the makespan itself once the episode is done."""
        b = self._b
        return int(b.backend.numpy(b.lower_bound())[0])

    def evaluate_order(self, rank=None, swap=None, start: bool = False, tail: bool = False, pairs=None):
        """The B = 1 form of ``BatchedJssEnv.evaluate_order`` (include/jss_order.h): the makespan of the semi-active schedule of
        the machine order ``rank`` (J x M or jmax x mmax; None: this env's finished ``solution``), optionally with the ranks of
        the two flat operation indices ``swap=(a, b)`` exchanged first; -1 refused, -2 cyclic.  ``start`` / ``tail`` / ``pairs``
        add the host arrays of the one row: ``(makespan[, start][, tail][, pair_a, pair_b, n_pairs])``."""
        b = self._b
        rank = None if rank is None else self._order_row(rank)
        swaps = None if swap is None else ([int(swap[0])], [int(swap[1])])
        out = b.evaluate_order(rank, None, swaps, start, tail, pairs)
        if not isinstance(out, tuple):
            return int(b.backend.numpy(out)[0])
        host = self._host_rows(out)
        return (int(host[0]),) + tuple(int(x) if x.ndim == 0 else x for x in host[1:])

    def tabu(self, rank=None, iters: int = 100, tenure: int = 8, target=None, trace: bool = False, last: bool = False):
        """The B = 1 form of ``BatchedJssEnv.tabu`` (include/jss_tabu.h): one tabu walk of at most ``iters`` moves from the
        machine order ``rank`` (J x M or jmax x mmax; None: this env's finished ``solution``).  Returns
        ``(best_makespan, best_rank, info[, trace][, last_rank])``: an int (-1 refused, -2 cyclic) and host arrays."""
        b = self._b
        rank = None if rank is None else self._order_row(rank)
        out = b.tabu(rank, iters, int(tenure), None if target is None else int(target), trace, last)
        host = self._host_rows(out)
        return (int(host[0]),) + tuple(host[1:])

    def tabu_blocks(self, rank=None, iters: int = 100, tenure: int = 8, target=None, reach: int = 0, trace: bool = False,
                    last: bool = False, log: bool = False):
        """The B = 1 form of ``BatchedJssEnv.tabu_blocks`` (include/jss_block.h): one tabu walk over block insertions of at most
        ``iters`` moves from the machine order ``rank`` (J x M or jmax x mmax; None: this env's finished ``solution``).  Returns
        ``(best_makespan, best_rank, info[, trace][, last_rank][, move_log])``: an int (-1 refused, -2 cyclic) and host arrays."""
        b = self._b
        rank = None if rank is None else self._order_row(rank)
        out = b.tabu_blocks(rank, iters, int(tenure), None if target is None else int(target), reach, trace, last, log)
        host = self._host_rows(out)
        return (int(host[0]),) + tuple(host[1:])

    def _order_row(self, rank, fill=-1):
        """a J x M or jmax x mmax table as the (1, jmax, mmax) int32 rank of the batch of one, ``fill`` in the padding"""
        b = self._b
        r = np.full((1, b.jmax, b.mmax), fill, np.int32)
        rank = np.asarray(rank)
        r[0, :rank.shape[-2], :rank.shape[-1]] = rank.reshape(rank.shape[-2:])
        return r

    def _host_rows(self, out):
        """row 0 of every array a call on the batch of one returned, on the host (None stays None)"""
        return [None if x is None else np.asarray(self._b.backend.numpy(x))[0] for x in out]

    def relink(self, rank, guide, steps=None, until: int = 0, margin: int = 0, trace: bool = False, last: bool = True,
               log: bool = False):
        """The B = 1 form of ``BatchedJssEnv.relink`` (include/jss_relink.h): one walk from the machine order ``rank`` (J x M or
        jmax x mmax; None: this env's finished ``solution``) towards the machine order ``guide``.  Returns ``(best_makespan,
        best_rank, last_makespan, last_rank, info[, trace][, move_log])``: ints (-1 refused, -2 no schedule) and host arrays."""
        b = self._b
        out = b.relink(None if rank is None else self._order_row(rank), self._order_row(guide), steps, int(until), margin, trace,
                       last, log)
        host = self._host_rows(out)
        return tuple(int(x) if k in (0, 2) and x is not None else x for k, x in enumerate(host))

    def order_distance(self, rank, guide) -> int:
        """The B = 1 form of ``BatchedJssEnv.order_distance``: the distance between two machine orders (-1 refused, -2 no
        schedule)."""
        b = self._b
        out = b.order_distance(None if rank is None else self._order_row(rank), self._order_row(guide))
        return int(np.asarray(b.backend.numpy(out))[0])

    def decode_keys(self, keys, delta: float = 1.0, start: bool = False, info: bool = False):
        """The B = 1 form of ``BatchedJssEnv.decode_keys`` (include/jss_decode.h): the key table ``keys`` (J x M or jmax x mmax)
        decoded by Giffler and Thompson's procedure with the delay parameter ``delta`` in [0, 1].  Returns the makespan, an int,
        then with ``start`` the (jmax, mmax) start times and with ``info`` the 4 counters, host arrays."""
        b = self._b
        k = np.zeros((b.jmax, b.mmax), np.int32)
        keys = np.asarray(keys)
        k[:keys.shape[-2], :keys.shape[-1]] = keys.reshape(keys.shape[-2:])
        out = b.decode_keys(k, None, float(delta), start, info)
        out = out if isinstance(out, tuple) else (out,)
        host = self._host_rows(out)
        return int(host[0]) if len(host) == 1 else (int(host[0]),) + tuple(host[1:])

    def _machine_row(self, rank):
        """``_order_row`` with 0 in the padding, as the one-machine calls and ``propagate`` take their tables"""
        return self._order_row(rank, 0)

    def relax_machines(self, rank=None, fixed: int = 0, jps: bool = False, schrage: bool = False, head: bool = False, tail: bool = False,
                       rank_out: bool = False):
        """The B = 1 form of ``BatchedJssEnv.relax_machines`` (include/jss_machine.h): the one-machine relaxations of the partial
        selection in which the machines of the mask ``fixed`` are sequenced by ``rank`` (J x M or jmax x mmax; None while nothing
        is fixed).  Returns ``(lower_bound, length, bottleneck)``, ints, then each where asked for ``jps``, ``schrage`` (mmax,),
        ``head``, ``tail`` and ``rank_out`` (jmax, mmax), host arrays."""
        b = self._b
        out = b.relax_machines(None if rank is None else self._machine_row(rank), int(fixed), None, jps, schrage, head, tail, rank_out)
        host = self._host_rows(out)
        return tuple(int(x) for x in host[:3]) + tuple(host[3:])

    def bottleneck(self, bias=None, reopt: int = 1, rank=None, fixed=None, order: bool = False):
        """The B = 1 form of ``BatchedJssEnv.bottleneck`` (include/jss_machine.h): one shifting bottleneck construction, from
        nothing or from the partial selection ``(rank, fixed)``; ``bias`` (mmax,) is added to the machines' bounds when the
        bottleneck is chosen.  Returns ``(makespan, rank, info[, order])``: an int (-1 refused, -2 cyclic) and host arrays."""
        b = self._b
        out = b.bottleneck(None, None if bias is None else np.asarray(bias, np.int32).reshape(1, -1), reopt,
                           None if rank is None else self._machine_row(rank), None if fixed is None else int(fixed), order)
        host = self._host_rows(out)
        return (int(host[0]),) + tuple(host[1:])

    def solve_machines(self, rank=None, fixed: int = 0, nodes: int = 256, opt: bool = False, low: bool = False, nodes_used: bool = False,
                       proved: bool = False, head: bool = False, tail: bool = False, rank_out: bool = False):
        """The B = 1 form of ``BatchedJssEnv.solve_machines`` (include/jss_carlier.h): ``relax_machines`` with the free machines'
        one-machine problems solved by Carlier's branch and bound within ``nodes`` search nodes each.  Returns ``(lower_bound,
        length, bottleneck)``, ints, then each where asked for ``opt``, ``low``, ``nodes_used`` (mmax,), ``proved`` (an int, the
        mask), ``head``, ``tail`` and ``rank_out`` (jmax, mmax), host arrays."""
        b = self._b
        out = b.solve_machines(None if rank is None else self._machine_row(rank), int(fixed), None, nodes, opt, low, nodes_used, proved,
                               head, tail, rank_out)
        host = self._host_rows(out)
        at = 3 + int(opt) + int(low) + int(nodes_used)
        if proved:
            host[at] = int(host[at]) & (2 ** 64 - 1)
        return tuple(int(x) for x in host[:3]) + tuple(host[3:])

    def bottleneck_exact(self, bias=None, reopt: int = 1, nodes: int = 256, rank=None, fixed=None, order: bool = False):
        """The B = 1 form of ``BatchedJssEnv.bottleneck_exact`` (include/jss_carlier.h): one shifting bottleneck construction with
        the machines sequenced by Carlier's branch and bound.  Returns ``(makespan, rank, info[, order])``: an int (-1 refused, -2
        cyclic) and host arrays, ``info`` with 8 entries."""
        b = self._b
        out = b.bottleneck_exact(None, None if bias is None else np.asarray(bias, np.int32).reshape(1, -1), reopt, nodes,
                                 None if rank is None else self._machine_row(rank), None if fixed is None else int(fixed), order)
        host = self._host_rows(out)
        return (int(host[0]),) + tuple(host[1:])

    def propagate(self, ub, rank=None, fixed: int = 0, est=None, lct=None, hyp=None, passes: int = 256, windows: bool = False):
        """The B = 1 form of ``BatchedJssEnv.propagate`` (include/jss_propagate.h): constraint propagation on the operation windows
        of the partial selection ``(rank, fixed)`` under the trial makespan ``ub``, from the windows ``est`` and ``lct`` (J x M or
        jmax x mmax) where given and under the hypothesis ``hyp = (flat index j * mmax + k, est, lct)`` on one operation.  Returns
        ``(status, passes_used)``, ints (status 0 a fixpoint, 1 refuted, 2 the budget is spent, -1 refused, -2 cyclic), then with
        ``windows`` ``est`` and ``lct`` (jmax, mmax), host arrays."""
        b = self._b
        out = b.propagate(int(ub), None if rank is None else self._machine_row(rank), int(fixed), None,
                          None if est is None else self._machine_row(est), None if lct is None else self._machine_row(lct),
                          None if hyp is None else tuple(np.asarray([int(x)], np.int32) for x in hyp), passes, windows)
        host = self._host_rows(out)
        return tuple(int(x) for x in host[:2]) + tuple(host[2:])

    def render(self, mode: str = "human"):
        """Gantt chart of ``solution`` (jss_env.py:655-693); needs pandas + plotly on the host."""
        from .render import gantt
        return gantt(self)

    def close(self):
        """gymnasium.Env.close(): waits for the env's outstanding device work."""
        self._b.synchronize()

    def __deepcopy__(self, memo):
        """``copy.deepcopy(env)`` as with the reference's plain Python object (MCTS / search code clones envs mid-episode):
        a new env on the same instance and device whose state is this env's, cloned on the device (``jss_clone``), plus the
        host-side attributes.  The two are independent from then on: closing or stepping one leaves the other as it was.
        The copy has this env's env id and seed, so a random rollout of the copy draws what this env's would."""
        b = self._b
        be = b.backend
        # an env that owns its backend gets a copy with a backend of its own (same device); a borrowed one is shared
        device = "cpu" if getattr(be, "name", "") == "cpu" else str(getattr(be, "device", None))
        new = type(self)(env_config={"instance_path": self.instance}, device=device if b._owns_backend else None,
                         _backend=None if b._owns_backend else be)
        memo[id(self)] = new
        new._b.seed = b.seed
        new._b.copy_from(b, [0])
        new._alloc_log, new._alloc_log_ok = list(self._alloc_log), self._alloc_log_ok
        new.last_time_step = self.last_time_step
        new.last_solution = None if self.last_solution is None else np.array(self.last_solution, copy=True)
        new.colors = list(self.colors)
        new.start_timestamp = self.start_timestamp
        return new

    def _run_rule(self, kind, explore: float = 0.0, seed=None, weights=None, keys=None, nope_key=None):
        """One whole episode of a dispatching rule, rule + step fused on the device (dispatching.py:55-75 with the
        exploration drawn from the counter RNG).  Returns (total reward, makespan) like ``run_episode``."""
        b = self._b
        if seed is not None:
            b.seed = int(seed)
        b.reset()
        b.zero_counters()
        self._alloc_log, self._alloc_log_ok = [], False      # the device picks the actions: no per-call log (next_jobs)

        def done():                                          # (from the host snapshot that the results below are read from)
            self._cache = None
            return self._h()["done"]
        play_to_end(b, kind, explore, done, "episode", weights=weights, keys=keys, nope_key=nope_key)
        h = self._h()
        self._raise_for(h["err"])
        self.last_time_step = h["clock"]
        self.last_solution = self._solution()
        return float(h["counters"][3]) / self.max_time_op, h["clock"]

    def _rule_best(self, kind, legal_actions, due_date_factor: float = 1.5):
        """arg-best of a dispatching rule over the legal jobs from the host snapshot of this step (dispatching.py's
        strict comparisons: the lowest job index wins ties); -1 when no job is legal.  Same selectors as the device's
        jss_policy (tests hold the two to each other)."""
        legal = np.asarray(legal_actions[:self.jobs], dtype=bool)
        if not legal.any():
            return -1
        h = self._h()
        if "job_state" not in h and kind in ("FIFO", "MOR", "LOR"):
            # these rank on ONE word of the job records: read it where it lies instead of decoding every record
            raw = h.t["job_state"][0][:self.jobs]
            if kind == "FIFO":
                key = raw[:, _abi.FC_IDLE_LAST if self._b.compact else _abi.F_IDLE_LAST].astype(np.float64)
            else:
                todo = raw[:, 0] & (_abi.FC_TODO_MASK if self._b.compact else _abi.TODO_MASK)
                key = ((self.machines - todo) * (1 if kind == "MOR" else -1)).astype(np.float64)
            key[~legal] = -np.inf
            return int(np.argmax(key))
        js = h["job_state"]
        todo = js[_abi.F_TODO]
        if kind == "FIFO":
            key = js[_abi.F_IDLE_LAST]
        elif kind == "SPT":
            key = -(js[_abi.F_CUR] & 0xFFFF)
        elif kind in ("MOR", "LOR"):
            key = (self.machines - todo) * (1 if kind == "MOR" else -1)
        else:
            rem = self._remaining[np.arange(self.jobs), np.minimum(todo, self.machines - 1)]
            if kind == "MWR":
                key = rem
            elif kind == "LWR":
                key = -rem
            elif kind == "CR":     # smallest (1.5 * job length - now) / remaining work, as the reference's floats (:391-398)
                with np.errstate(divide="ignore"):
                    key = -np.where(rem > 0, (self._remaining[:, 0] * due_date_factor - self._h()["clock"]) / np.maximum(rem, 1), np.inf)
            else:
                raise KeyError(kind)
        key = np.where(legal, key, -np.inf)
        return int(np.argmax(key))           # first maximum = lowest index among ties

    # on-device action selectors for the dispatching module
    def _policy(self, kind, cr_factor=None):
        return int(self._b.backend.numpy(self._b.policy(kind, cr_factor=cr_factor))[0])


def make(env_id: str = "jss-v1", env_config=None, **kwargs):
    """``gym.make('jss-v1', env_config=...)`` without gymnasium (JSSEnv/__init__.py:6-9)."""
    if env_id != "jss-v1":
        raise ValueError(f"unknown env id {env_id!r}; this package registers 'jss-v1'")
    return JssEnv(env_config=env_config, **kwargs)
