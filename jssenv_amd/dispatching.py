"""Dispatching rules with the reference's surface (JSSEnv/dispatching.py).

Same names (``ShortestProcessingTime`` ... ``CriticalRatio``, ``DISPATCHING_RULES``,
``get_rule``, ``compare_rules``), same call convention (``rule(env) -> action``,
``rule.run_episode(env) -> (total_reward, makespan)``) and the same semantics:

  * NOPE when it is the only legal action (dispatching.py:96-97 and twins);
  * arg-min / arg-max over the legal jobs with strict comparisons, so the lowest job
    index wins ties (:108, :148, ...);
  * then, if NOPE is legal, NOPE with probability 0.1 drawn from NumPy's *global* RNG
    (:113, :153, ...) -- kept on the host exactly so, which makes ``np.random.seed(s)``
    runs reproduce the reference's traces.

The arg-best itself runs on the GPU (``jss_policy``, csrc ``select_action``/``p_select``)
when ``env`` is a ``jssenv_amd.JssEnv``; any other env object exposing the reference's
attributes falls back to the attribute-reading loop of the reference rule (CriticalRatio's float
ratios with its per-episode due-date cache, :327-408, included).

For whole batches use ``BatchedJssEnv.rollout(kind)`` -- rule + step fused on the device.  Two entry points
of this module do that for you on a jssenv_amd env: ``rule.run_episode(env, device_rng=True)`` plays the whole
episode in fused launches (the 10 % NOPE exploration then comes from the device's counter RNG instead of
NumPy's global one -- same distribution, not the same stream), and ``compare_rules`` plays each rule's
``num_episodes`` episodes as ONE batch of ``num_episodes`` envs.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np

EXPLORATION_PROBABILITY = 0.1  # dispatching.py:113


class DispatchingRule:
    """Base class (dispatching.py:21-75)."""

    kind: Optional[str] = None   # name of the on-device selector
    larger_wins = False

    def __init__(self, name: str, description: str):
        self.name = name
        self.description = description

    def get_name(self) -> str:
        return self.name

    def get_description(self) -> str:
        return self.description

    # value the rule ranks job `job` by (host path)
    def _value(self, env, job: int):
        raise NotImplementedError("Subclasses must implement __call__")

    def _best_job(self, env, legal_actions) -> int:
        if self.kind is not None and hasattr(env, "_rule_best"):
            # jssenv_amd env: the state of this step is already on the host (one copy per step()); the arg-best over
            # the legal jobs is one vectorised pass over it -- no second launch / copy / sync per decision
            return env._rule_best(self.kind, legal_actions)
        if self.kind is not None and hasattr(env, "_policy"):
            a = env._policy(self.kind)            # device arg-best, lowest index wins ties
            return a if a < env.jobs else -1
        best, best_v = -1, None
        for job in range(env.jobs):
            if legal_actions[job]:
                v = self._value(env, job)
                if best_v is None or (v > best_v if self.larger_wins else v < best_v):
                    best, best_v = job, v
        return best

    def __call__(self, env) -> int:
        legal_actions = env.get_legal_actions()
        if np.sum(legal_actions) == 1 and legal_actions[-1]:
            return env.jobs
        job = self._best_job(env, legal_actions)
        if legal_actions[env.jobs] and np.random.random() < EXPLORATION_PROBABILITY:
            return env.jobs
        return job

    def run_episode(self, env, device_rng: bool = False, seed: Optional[int] = None) -> Tuple[float, int]:
        """dispatching.py:55-75.  ``device_rng=True`` (jssenv_amd envs only): rule + step fused on the device for the
        whole episode, exploration drawn from the counter RNG keyed by ``seed``."""
        if device_rng:
            if self.kind is None or not hasattr(env, "_b") or not _device_rule_ok(self):
                raise ValueError("device_rng=True needs a jssenv_amd.JssEnv and a rule with an on-device selector")
            return env._run_rule(device_kind(self), explore=EXPLORATION_PROBABILITY, seed=seed)
        env.reset()
        done = False
        total_reward = 0.0
        while not done:
            action = self(env)
            _, reward, done, _, _ = env.step(action)
            total_reward += reward
        return total_reward, env.current_time_step


def _device_rule_ok(rule) -> bool:
    """CriticalRatio's device selector takes due-date factors p / q with q a power of two (exact in the reference's
    doubles); any other factor stays on the host."""
    return device_kind(rule) is not None


def device_kind(rule):
    """What the device entry points take as `kind` for this rule (None: no on-device selector)."""
    if rule.kind is None:
        return None
    if hasattr(rule, "due_date_factor"):
        from ._abi import cr_kind
        return cr_kind(rule.due_date_factor)
    return rule.kind


def _remaining_work(env, job: int) -> int:                                # dispatching.py:187-189
    return int(sum(env.instance_matrix[job][op][1] for op in range(env.todo_time_step_job[job], env.machines)))


class ShortestProcessingTime(DispatchingRule):                            # dispatching.py:78-116
    kind, larger_wins = "SPT", False

    def __init__(self):
        super().__init__("SPT", "SPT - among the legal jobs, start the one whose current operation is shortest")

    def _value(self, env, job):
        return env.instance_matrix[job][env.todo_time_step_job[job]][1]


class FirstInFirstOut(DispatchingRule):                                   # dispatching.py:119-156
    kind, larger_wins = "FIFO", True

    def __init__(self):
        super().__init__("FIFO", "FIFO - among the legal jobs, start the one that has been idle longest since its last operation")

    def _value(self, env, job):
        return env.idle_time_jobs_last_op[job]


class MostWorkRemaining(DispatchingRule):                                 # dispatching.py:159-199
    kind, larger_wins = "MWR", True

    def __init__(self):
        super().__init__("MWR", "MWR - among the legal jobs, start the one with the largest sum of remaining durations")

    def _value(self, env, job):
        return _remaining_work(env, job)


class LeastWorkRemaining(DispatchingRule):                                # dispatching.py:202-242
    kind, larger_wins = "LWR", False

    def __init__(self):
        super().__init__("LWR", "LWR - among the legal jobs, start the one with the smallest sum of remaining durations")

    def _value(self, env, job):
        return _remaining_work(env, job)


class MostOperationsRemaining(DispatchingRule):                           # dispatching.py:245-283
    kind, larger_wins = "MOR", True

    def __init__(self):
        super().__init__("MOR", "MOR - among the legal jobs, start the one with the most operations still to do")

    def _value(self, env, job):
        return env.machines - env.todo_time_step_job[job]


class LeastOperationsRemaining(DispatchingRule):                          # dispatching.py:286-324
    kind, larger_wins = "LOR", False

    def __init__(self):
        super().__init__("LOR", "LOR - among the legal jobs, start the one with the fewest operations still to do")

    def _value(self, env, job):
        return env.machines - env.todo_time_step_job[job]


class CriticalRatio(DispatchingRule):                                     # dispatching.py:327-408
    """(due date - now) / remaining work, smallest first; due date = factor x job length, cached
    per job and dropped when ``current_time_step == 0`` (:373-374).  On a jssenv_amd env the arg-min runs on
    the device -- as an exact fraction comparison (csrc ``cr_better``) for factors p / 2^k, as the reference's float64
    expression (``cr_ratio_f64``) for any other: ``BatchedJssEnv.policy("CR", cr_factor=f)``; the float path below
    serves other envs."""

    kind, larger_wins = "CR", False

    def __init__(self, due_date_factor: float = 1.5):
        super().__init__("CR", "CR - among the legal jobs, start the one with the smallest (due date - now) / remaining work")
        self.due_date_factor = due_date_factor
        self._due_dates: Dict[int, float] = {}

    def _calculate_due_date(self, env, job: int) -> float:                # :351-363
        if job not in self._due_dates:
            total = sum(env.instance_matrix[job][op][1] for op in range(env.machines))
            self._due_dates[job] = total * self.due_date_factor
        return self._due_dates[job]

    def _best_job(self, env, legal_actions) -> int:
        # on a jssenv_amd env the arg-min comes from the host snapshot of the step (the reference's float expression,
        # vectorised) or from the device selectors: (p * job_length - q * now) / remaining compared exactly for factors
        # p / q with q a power of two (these also run inside the fused rollouts), the reference's float64 expression
        # itself for any other factor (JSS_POLICY_CR_F64, policy launches only); other envs take the loop below
        if hasattr(env, "_rule_best"):
            return env._rule_best("CR", legal_actions, due_date_factor=self.due_date_factor)
        if hasattr(env, "_policy"):
            code = device_kind(self)          # p / 2^k factors: the integer-exact selector; any other: the float64 one
            a = env._policy(code) if code is not None else env._policy("CR", cr_factor=self.due_date_factor)
            return a if a < env.jobs else -1
        saved, self.kind = self.kind, None
        try:
            return super()._best_job(env, legal_actions)
        finally:
            self.kind = saved

    def _value(self, env, job):
        remaining = _remaining_work(env, job)
        time_remaining = self._calculate_due_date(env, job) - env.current_time_step
        return time_remaining / remaining if remaining > 0 else float("inf")   # :395-398

    def __call__(self, env) -> int:
        legal_actions = env.get_legal_actions()
        if np.sum(legal_actions) == 1 and legal_actions[-1]:
            return env.jobs
        if env.current_time_step == 0:                                    # :373-374
            self._due_dates = {}
        job = self._best_job(env, legal_actions)
        if legal_actions[env.jobs] and np.random.random() < EXPLORATION_PROBABILITY:
            return env.jobs
        return job


# ---- caller-weighted rules (include/jss_rules.h) ------------------------------------------------------------------
# A rule is a row of 8 int32: weights of seven quantities of a legal job and a NOPE bias.
RW_DUR, RW_NEXT, RW_REM, RW_TOTAL, RW_OPS, RW_WAIT, RW_IDLE, RW_NOPE = range(8)
NEVER_NOPE = -2**31


def _row(**w):
    r = np.zeros(8, dtype=np.int32)
    r[RW_NOPE] = NEVER_NOPE
    for k, v in w.items():
        r[{"dur": RW_DUR, "rem": RW_REM, "ops": RW_OPS, "wait": RW_WAIT}[k]] = v
    return r


# the six linear stock rules as weight rows: each plays exactly what its stock rule plays (CriticalRatio is a ratio, not a row)
RULE_WEIGHTS = {"SPT": _row(dur=-1), "FIFO": _row(wait=1), "MWR": _row(rem=1), "LWR": _row(rem=-1), "MOR": _row(ops=1),
                "LOR": _row(ops=-1)}


def _wrap64(v: int) -> int:
    """A Python int reduced mod 2^64 and read as signed: the device's wrapping 64-bit sum."""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


class WeightedRule(DispatchingRule):
    """A dispatching rule given by integer weights: among the legal jobs, the one with the largest
    ``score(j) = sum_f weights[f] * x_f(j)`` -- x = (duration of the current op, duration of the next op or 0, remaining work,
    job length, remaining ops, idle time since the last op, total idle time) -- in wrapping signed 64-bit arithmetic, the
    lowest job index on ties; NOPE when only NOPE is legal, or when it is legal, ``weights[7]`` is not ``NEVER_NOPE`` and
    ``weights[7]`` exceeds the best score.  Then, where NOPE is legal, NOPE with probability ``explore`` (default 0: a
    weighted rule says itself when to wait).  Float weights are the caller's to quantise: scale, round.

    ``__call__`` restates this on the reference's public env attributes, so it plays any env that has them; on the device the
    same rule is ``BatchedJssEnv.policy / rollout / lookahead(kind="weighted", weights=rule.weights)``, bit for bit, and
    ``run_episode`` on a jssenv_amd env plays the episode there (``jss_rule_rollout``)."""

    kind = "weighted"

    def __init__(self, weights, name: str = "weighted", explore: float = 0.0):
        w = np.asarray(weights)
        if w.shape != (8,) or w.dtype.kind not in "iu" or (w.astype(np.int64) != w.astype(np.int64).astype(np.int32)).any():
            raise ValueError("weights: 8 integers in the int32 range")
        super().__init__(name, f"{name} - among the legal jobs, start the one with the largest weighted score")
        self.weights = w.astype(np.int32)
        self.explore = float(explore)

    def _features(self, env, job: int):
        todo, M = int(env.todo_time_step_job[job]), env.machines
        durs = [int(env.instance_matrix[job][op][1]) for op in range(M)]
        return (durs[todo], durs[todo + 1] if todo + 1 < M else 0, sum(durs[todo:]), sum(durs), M - todo,
                int(env.idle_time_jobs_last_op[job]), int(env.total_idle_time_jobs[job]))

    def _value(self, env, job: int) -> int:
        return _wrap64(sum(int(w) * x for w, x in zip(self.weights[:7], self._features(env, job))))

    def __call__(self, env) -> int:
        legal_actions = env.get_legal_actions()
        jobs = [j for j in range(env.jobs) if legal_actions[j]]
        if not jobs:
            return env.jobs if legal_actions[env.jobs] else -1
        best, best_v = -1, None
        for j in jobs:
            v = self._value(env, j)
            if best_v is None or v > best_v:
                best, best_v = j, v
        if legal_actions[env.jobs]:
            bias = int(self.weights[RW_NOPE])
            if bias != NEVER_NOPE and bias > best_v:
                best = env.jobs
            if self.explore > 0.0 and np.random.random() < self.explore:
                best = env.jobs
        return best

    def run_episode(self, env, device_rng: bool = False, seed: Optional[int] = None) -> Tuple[float, int]:
        """On a jssenv_amd env the episode is one ``jss_rule_rollout`` -- always when the rule draws nothing (``explore == 0``:
        the host loop would play the same actions), with ``device_rng=True`` otherwise; any other env takes the host loop."""
        if hasattr(env, "_b") and (device_rng or self.explore == 0.0):
            return env._run_rule("weighted", explore=self.explore, seed=seed, weights=self.weights)
        if device_rng:
            raise ValueError("device_rng=True needs a jssenv_amd.JssEnv")
        return super().run_episode(env)


def evaluate_weights(instances, weights, device=None, explore: float = 0.0, seed: int = 0, _backend=None):
    """Makespans of a population of weighted rules: ``weights`` is (P, 8) int32 -- a NumPy array, or a tensor on the host or on
    the device --, ``instances`` one instance or a list of N; one env per (weight row, instance) -- row-major, so the result,
    a NumPy int64 array, has shape (P, N) -- is reset and played to the end by one ``jss_rule_rollout``.  The inner loop of an
    evolution strategy / GA / GP over linear rules, in one call.  ``device``: as for ``BatchedJssEnv`` ('cpu' = the host twin).

    Every call builds its batch anew (allocation, upload of the instances, reset) and copies the makespans back: a loop over
    generations that wants neither keeps one ``BatchedJssEnv(instance, batch=P)`` and calls ``reset()`` and
    ``rollout("weighted", weights=w, autoreset=False)`` on it with ``w`` on the device -- the two lines this function ends in."""
    from .env import BatchedJssEnv, play_to_end
    from .instances import Instance, builtin_instance
    one = isinstance(instances, (str, Instance))
    insts = [instances] if one else list(instances)
    insts = [builtin_instance(i) if isinstance(i, str) else i for i in insts]
    w = weights if hasattr(weights, "repeat_interleave") else np.ascontiguousarray(np.asarray(weights))
    if len(w.shape) != 2 or w.shape[1] != 8 or str(w.dtype).split(".")[-1] != "int32":
        raise ValueError("weights: an int32 array or tensor of shape (P, 8)")
    P, N = int(w.shape[0]), len(insts)
    if P == 0 or N == 0:
        return np.zeros((P, N), dtype=np.int64)
    kw = {"_backend": _backend} if _backend is not None else {"device": device}
    if N == 1:
        env = BatchedJssEnv(insts[0], batch=P, seed=int(seed), **kw)
        rows = w
    else:
        env = BatchedJssEnv(insts, batch=P * N, seed=int(seed), table_of_env=np.arange(P * N, dtype=np.int32) % N, **kw)
        rows = w.repeat_interleave(N, dim=0) if hasattr(w, "repeat_interleave") else np.repeat(w, N, axis=0)
    if hasattr(rows, "repeat_interleave") and getattr(env.backend, "torch", None) is None:
        rows = rows.detach().cpu().numpy()                                # a tensor, and the host twin's NumPy memory
    env.reset()
    play_to_end(env, "weighted", explore, weights=rows)
    return env.backend.numpy(env.makespan).astype(np.int64).reshape(P, N)


# ---- per-operation priority keys (include/jss_keys.h) -------------------------------------------------------------
# A rule is a table of one int32 key per operation: among the legal jobs, the one whose CURRENT operation has the largest key.
KEY_NEVER_NOPE = -2**31


class KeyRule(DispatchingRule):
    """A dispatching rule given by a (J, M) int32 table of priorities, one per operation -- the random-key / priority-list
    encoding of a schedule: among the legal jobs, the one with the largest ``keys[job][ops the job has completed]``, the lowest
    job index on ties; NOPE when only NOPE is legal, or when it is legal and ``nope_key`` exceeds that key (``None``: never
    while a job is legal).  Then, where NOPE is legal, NOPE with probability ``explore`` (default 0).

    ``__call__`` reads only the public ``legal_actions`` and ``todo_time_step_job`` of an env, so it plays any env that has
    them; on the device the same rule is ``BatchedJssEnv.policy / rollout / lookahead(kind="keys", keys=rule.keys,
    nope_key=rule.nope_key)``, bit for bit, and ``run_episode`` on a jssenv_amd env plays the episode there
    (``jss_key_rollout``)."""

    kind = "keys"

    def __init__(self, keys, nope_key: Optional[int] = None, name: str = "keys", explore: float = 0.0):
        k = np.asarray(keys)
        if k.ndim != 2 or k.dtype.kind not in "iu" or (k.astype(np.int64) != k.astype(np.int64).astype(np.int32)).any():
            raise ValueError("keys: a (J, M) table of integers in the int32 range")
        nope = KEY_NEVER_NOPE if nope_key is None else int(nope_key)
        if not -2**31 <= nope < 2**31:
            raise ValueError("nope_key: an integer in the int32 range")
        super().__init__(name, f"{name} - among the legal jobs, start the one whose current operation has the largest key")
        self.keys = np.ascontiguousarray(k.astype(np.int32))
        self.nope_key = nope
        self.explore = float(explore)

    def __call__(self, env) -> int:
        legal_actions = env.legal_actions
        J = len(legal_actions) - 1
        todo = env.todo_time_step_job
        best, best_key = -1, None
        for j in range(J):
            if legal_actions[j]:
                key = int(self.keys[j][int(todo[j])])
                if best_key is None or key > best_key:
                    best, best_key = j, key
        if best < 0:
            return J if legal_actions[J] else -1
        if legal_actions[J]:
            if self.nope_key > best_key:
                best = J
            if self.explore > 0.0 and np.random.random() < self.explore:
                best = J
        return best

    def _device_keys(self, env):
        """the table over a jssenv_amd env's padded extents (they are the instance's own for a B = 1 view)"""
        if self.keys.shape != (env.jobs, env.machines):
            raise ValueError(f"keys of shape {self.keys.shape} on an instance of {env.jobs} x {env.machines}")
        return self.keys

    def run_episode(self, env, device_rng: bool = False, seed: Optional[int] = None) -> Tuple[float, int]:
        """On a jssenv_amd env the episode is one ``jss_key_rollout`` -- always when the rule draws nothing (``explore == 0``:
        the host loop would play the same actions), with ``device_rng=True`` otherwise; any other env takes the host loop."""
        if hasattr(env, "_b") and (device_rng or self.explore == 0.0):
            return env._run_rule("keys", explore=self.explore, seed=seed, keys=self._device_keys(env), nope_key=self.nope_key)
        if device_rng:
            raise ValueError("device_rng=True needs a jssenv_amd.JssEnv")
        return super().run_episode(env)


def _instance_of(instance):
    from .instances import builtin_instance
    return builtin_instance(instance) if isinstance(instance, str) else instance


def rule_keys(instance, rule: str) -> np.ndarray:
    """The (J, M) int32 key table that plays what the stock rule ``rule`` plays on ``instance``, for the five stock rules that
    ARE a table per operation: SPT = -duration, MWR = remaining work, LWR = -remaining work, MOR = M - k, LOR = k - M (k: the
    operation's index in its job).  FIFO and CriticalRatio rank by the clock, not by the operation: ``ValueError``."""
    inst = _instance_of(instance)
    dur = np.asarray(inst.duration, dtype=np.int64)
    J, M = dur.shape
    rem = dur[:, ::-1].cumsum(axis=1)[:, ::-1]                            # rem[j][k] = durations of ops k..M-1
    left = np.broadcast_to(M - np.arange(M, dtype=np.int64), (J, M))
    tables = {"SPT": -dur, "MWR": rem, "LWR": -rem, "MOR": left, "LOR": -left}
    if rule not in tables:
        raise ValueError(f"rule {rule!r} is no table of per-operation keys: one of {sorted(tables)}")
    return np.ascontiguousarray(tables[rule].astype(np.int32))


def keys_from_actions(instance, actions) -> np.ndarray:
    """An episode's action sequence as a (J, M) int32 key table that reproduces it: the k-th operation of job j gets the key
    ``-d``, d the index in ``actions`` of the decision that dispatched it; NOPE (``J``) and ``-1`` entries are skipped (so are
    the ``JSS_ACTION_SKIP`` entries a finished env records); operations never dispatched keep ``-len(actions)``.  ``actions``:
    one env's record, e.g. ``trajectory(...)["action"][:, i]``.

    Any episode played with NOPE taken only when no job was legal is reproduced decision for decision by
    ``rollout("keys", keys=...)``: at decision d every other legal job's current operation is dispatched later than d, so it
    holds a smaller key and the chosen job holds the largest.  An episode with voluntary NOPEs (exploration, a NOPE bias) is
    not promised: the table says which job goes first, never when to wait."""
    inst = _instance_of(instance)
    J, M = inst.jobs, inst.machines
    acts = np.asarray(actions).reshape(-1)
    keys = np.full((J, M), -len(acts), dtype=np.int64)
    done = np.zeros(J, dtype=np.int64)
    for d, a in enumerate(acts):
        a = int(a)
        if a < 0 or a >= J:
            continue
        if done[a] >= M:
            raise ValueError(f"decision {d} dispatches job {a}, which has no operation left")
        keys[a, done[a]] = -d
        done[a] += 1
    return keys.astype(np.int32)


def keys_from_floats(x):
    """The order-preserving map float32 -> int32: ``x < y`` exactly when ``keys_from_floats(x) < keys_from_floats(y)`` as
    signed integers, -0 and +0 get one key, +-inf are the largest and smallest keys in use; NaN is refused (``ValueError``).  A
    network's float priorities become key tables without losing an order relation.  NumPy arrays (anything ``np.asarray``
    takes) and torch tensors, on the device when given a device tensor; other float dtypes are rounded to float32 first."""
    if hasattr(x, "is_floating_point"):                                  # a torch tensor
        import torch
        f = x.to(torch.float32) + 0.0                                     # (-0 + 0 = +0)
        if bool(torch.isnan(f).any()):
            raise ValueError("keys_from_floats: NaN has no place in an order")
        b = f.contiguous().view(torch.int32)
        return torch.where(b >= 0, b, b ^ 0x7FFFFFFF)
    f = np.ascontiguousarray(np.asarray(x, dtype=np.float32) + np.float32(0.0))
    if np.isnan(f).any():
        raise ValueError("keys_from_floats: NaN has no place in an order")
    b = f.view(np.int32)
    return np.where(b >= 0, b, b ^ np.int32(0x7FFFFFFF)).astype(np.int32)


def keys_from_schedule(start):
    """Start times as a key table: ``-start`` as int32, 0 in the padding (the entries below 0) -- an array of any leading shape, a
    NumPy array or a tensor.  The round trip: for every schedule ``S`` that a Giffler-Thompson decode with ``delta=1`` produced
    (``BatchedJssEnv.decode_keys``, include/jss_decode.h), ``decode_keys(keys_from_schedule(S), delta=1)`` gives ``S`` back exactly.
    Such an ``S`` is an active schedule, and among the unscheduled operations of a machine the one it starts first is always in
    the conflict set, where its key, the largest, wins.  So a schedule a search has improved -- by ``tabu_blocks``, ``relink`` --
    goes back into a population of key tables as long as it is active."""
    if hasattr(start, "is_floating_point"):                              # a torch tensor
        import torch
        s = start.to(torch.int32)
        return torch.where(s < 0, torch.zeros_like(s), -s)
    s = np.asarray(start).astype(np.int32)
    return np.where(s < 0, 0, -s).astype(np.int32)


def evaluate_keys(instance, keys, nope_key: Optional[int] = None, device=None, explore: float = 0.0, seed: int = 0,
                  return_solution: bool = False, _backend=None, decoder: str = "env", delta: float = 1.0):
    """Makespans of a population of key tables: ``keys`` is (P, J, M) int32 -- a NumPy array, or a tensor on the host or on the
    device --, one chromosome per row; one env per table is reset and decoded to the end by one ``jss_key_rollout``.  Returns
    the (P,) makespans, a NumPy int64 array; with ``return_solution`` also the (P, J, M) start times of the decoded schedules
    (``start[p][j][k]``: operation k of job j).  The inner loop of a GA / BRKGA / CMA-ES over keys, in one call.  ``device``: as
    for ``BatchedJssEnv`` ('cpu' = the host twin).

    Every call builds its batch anew, as ``evaluate_weights`` does: a loop over generations keeps one
    ``BatchedJssEnv(instance, batch=P)`` and calls ``reset()`` and ``rollout("keys", keys=k, autoreset=False)`` on it.

    ``decoder="env"`` is that decode, through the env's own dynamics.  ``decoder="active"`` decodes by Giffler and Thompson's
    procedure instead (``BatchedJssEnv.decode_keys``, include/jss_decode.h) with the delay parameter ``delta`` in [0, 1] -- 1:
    active schedules, 0: non-delay schedules -- on ONE env that is only read; ``nope_key``, ``explore`` and ``seed`` play no part
    in it."""
    from .env import BatchedJssEnv, play_to_end
    if decoder not in ("env", "active"):
        raise ValueError("evaluate_keys: decoder is 'env' or 'active'")
    inst = _instance_of(instance)
    J, M = inst.jobs, inst.machines
    k = keys if hasattr(keys, "is_floating_point") else np.ascontiguousarray(np.asarray(keys))
    if len(k.shape) != 3 or tuple(k.shape[1:]) != (J, M) or str(k.dtype).split(".")[-1] != "int32":
        raise ValueError(f"keys: an int32 array or tensor of shape (P, {J}, {M})")
    P = int(k.shape[0])
    if P == 0:
        ms = np.zeros((0,), dtype=np.int64)
        return (ms, np.zeros((0, J, M), dtype=np.int64)) if return_solution else ms
    kw = {"_backend": _backend} if _backend is not None else {"device": device}
    env = BatchedJssEnv(inst, batch=1 if decoder == "active" else P, seed=int(seed), **kw)
    if hasattr(k, "is_floating_point") and getattr(env.backend, "torch", None) is None:
        k = k.detach().cpu().numpy()                                      # a tensor, and the host twin's NumPy memory
    env.reset()
    if decoder == "active":
        out = env.decode_keys(k, np.zeros(P, np.int32), delta, start=return_solution)
        if return_solution:
            return tuple(env.backend.numpy(x).astype(np.int64) for x in out)
        return env.backend.numpy(out).astype(np.int64).reshape(P)
    play_to_end(env, "keys", explore, keys=k, nope_key=nope_key)
    ms = env.backend.numpy(env.makespan).astype(np.int64).reshape(P)
    if return_solution:
        return ms, env.backend.numpy(env.solution).astype(np.int64).reshape(P, J, M)
    return ms


DISPATCHING_RULES = {                                                     # dispatching.py:412-420
    "SPT": ShortestProcessingTime(),
    "FIFO": FirstInFirstOut(),
    "MWR": MostWorkRemaining(),
    "LWR": LeastWorkRemaining(),
    "MOR": MostOperationsRemaining(),
    "LOR": LeastOperationsRemaining(),
    "CR": CriticalRatio(),
}


def get_rule(rule_name: str) -> DispatchingRule:                          # dispatching.py:423-439
    try:
        return DISPATCHING_RULES[rule_name]
    except KeyError:
        raise ValueError(f"Rule '{rule_name}' not found. Available rules: {list(DISPATCHING_RULES)}") from None


def compare_rules(env, rules: Optional[List[str]] = None, num_episodes: int = 10,
                  seed: Optional[int] = None) -> Dict[str, Dict[str, float]]:
    """Mean total reward and mean makespan of each rule over ``num_episodes`` episodes on ``env``
    (same result keys as dispatching.py:442-475).

    On a jssenv_amd env the ``num_episodes`` episodes of a rule are one batch of ``num_episodes`` envs of the same
    instance: rule + step fused in the rollout kernel, the rules' 10 % NOPE exploration drawn per env from the
    counter RNG (``seed`` keys it; default: a draw from NumPy's global RNG, so ``np.random.seed`` still makes the
    comparison reproducible).  Any other env object takes the reference's sequential loop."""
    names = list(DISPATCHING_RULES) if rules is None else list(rules)
    on_device = hasattr(env, "_b") and all(get_rule(n).kind is not None and _device_rule_ok(get_rule(n)) for n in names)
    results = {}
    if on_device and num_episodes > 0:
        from .env import BatchedJssEnv, play_to_end
        base = int(np.random.randint(0, 2**31 - 1)) if seed is None else int(seed)
        inst = env.instance
        batch = BatchedJssEnv([inst], batch=int(num_episodes), seed=base, _backend=env._b.backend)
        for k, name in enumerate(names):
            batch.seed = base + 7919 * k
            batch.reset()
            batch.zero_counters()
            rule = get_rule(name)                  # (a WeightedRule / KeyRule: its own row / table and its own exploration rate)
            own = {"keys": rule._device_keys(env), "nope_key": rule.nope_key} if rule.kind == "keys" else \
                  {"weights": getattr(rule, "weights", None)}
            play_to_end(batch, device_kind(rule), getattr(rule, "explore", EXPLORATION_PROBABILITY),
                        what=f"rule {name}: episodes", **own)
            cnt = batch.backend.numpy(batch.counters)
            results[name] = {"avg_reward": float(cnt[:, 3].sum()) / inst.max_time_op / num_episodes,
                             "avg_makespan": float(batch.backend.numpy(batch.makespan).sum()) / num_episodes}
        return results
    for name in names:
        episodes = [get_rule(name).run_episode(env) for _ in range(num_episodes)]
        results[name] = {"avg_reward": sum(r for r, _ in episodes) / num_episodes,
                         "avg_makespan": sum(m for _, m in episodes) / num_episodes}
    return results
