"""One recipe per kernel instantiation of the library (tests/test_kernel_matrix.py)."""
import ctypes as C
import re
import subprocess

import numpy as np

import logits_cases as L
import parity_cases as P
from jssenv_amd import _abi
from jssenv_amd import instances as I
from jssenv_amd.env import BatchedJssEnv, CpuBackend
from oracle import OracleEnv


def short_name(symbol):
    """'void jss::jss_kernel<1, 5, 2>(jss::Params)' -> 'jss_kernel<1, 5, 2>': a demangled kernel symbol without return type,
    namespaces and parameter list -- the same for the emulator's launch log, its symbol table and the gfx950 code object."""
    s = symbol.strip().replace("(anonymous namespace)::", "").replace("jss::", "")
    if s.startswith("void "):
        s = s[5:]
    return s.split("(", 1)[0]


_KERNEL = re.compile(r"^jss_\w*kernel\w*(<[0-9, ]+>)?$")


def library_kernels(emu_lib):
    """The kernels of the built emulator library, from its symbol table (what kernel_name() of tests/emu/hip/hip_runtime.h
    resolves a launch to): every function whose name is jss_*kernel*, with its template arguments."""
    out = subprocess.run(["nm", "-C", "--defined-only", emu_lib], capture_output=True, text=True, check=True).stdout
    names = set()
    for line in out.splitlines():
        parts = line.split(None, 2)
        if len(parts) == 3 and parts[1] in "tTwW" and _KERNEL.match(short_name(parts[2])):
            names.add(short_name(parts[2]))
    return sorted(names)


def code_object_kernels(hip_lib):
    """The same list from the gfx950 code object of the HIP library (tools/kernel_resources.py)."""
    from kernel_resources import kernel_resources
    return sorted(short_name(row[0]) for row in kernel_resources(hip_lib))


# ---- recipes ------------------------------------------------------------------------------------------------------------------
# A recipe = (kernel it claims to reach, BatchedJssEnv arguments that make the dispatch of jss_kernels.hip choose it, the call
# that runs the mode).  Generated from the dimensions flavour x table layout x mode; every recipe holds EVERY env of its batch
# to the oracle (oracle/: OracleEnv driven with the same actions / the same counter RNG) through P.assert_matches_oracle, the
# env's reward and done outputs and its counters (steps, episodes, makespan sum, the exact reward numerators) included, and
# what the mode returns (trajectory and step records, policy actions, lookahead scores) to the same oracle.
#
# Edges every recipe sits on:
#   batch     not a multiple of the envs per block (4 wavefronts): the last block has a part-filled wavefront / lane group
#             (jss_kernel_two: odd, the last wavefront holds one env)
#   J         at the flavour's limit (16, 32, 64, 128) and below it (65 for two jobs per lane): a shared-table recipe runs
#             once per shape of SHARED_SHAPES; per-env tables: ragged inside the padded rows, with a 3 x 2 env
#   NOPE/done the even envs of a batch start a few steps before the END of their first episodes, so some finish inside the
#             call: auto-reset and the frozen-when-done path both run; the odd envs start in the MIDDLE of their second
#             episodes, where with 8-16 machines NOPE is legal in about three states of ten (with 2-3 machines and many jobs
#             it hardly ever is: the reference allows NOPE only with at most four legal actions) -- the host-driven modes
#             take it half of the time it is legal, the rules explore it half of the time, the logits favour it.  Every
#             stepping recipe asserts on its oracles that an episode ended AND that a NOPE was taken inside the call
#   records   compact and medium records with durations 65 533 .. 65 535, the widest their fields take, next to ordinary
#             durations 1 .. 99 (compact: the second shape; medium: every fourth instance of the list)
#
# Warm start: the state the mode starts from is rolled out by the host-core twin (libjss_cpu.so) and loaded with
# load_state_dict -- a few hundred emulator steps per recipe saved.  The oracle makes the same rollout from the same counter
# RNG, and the comparison after the call holds the whole state to it, so nothing is taken on trust from the twin.
SEED, ID_BASE = 41, 500
TABS = {0: "shared-full", 1: "own-full", 2: "shared-compact", 3: "own-medium"}          # kTabLds, kTabGlobal, kTabLdsC, kTabGlobalM (jss_common.hpp)
SHARED = (0, 2)
MODES = {0: "reset", 1: "step", 2: "advance", 3: "policy", 4: "rollout", 5: "rollout1", 6: "trajectory", 7: "steps", 9: "logits",
         10: "lookahead"}
MODE_NUMBER = dict({name: m for m, name in MODES.items()}, session=8)
# flavour -> (kernel name prefix, shapes (jobs, machines) of the per-env tables -- the first is the padded extent --, batch,
#             BatchedJssEnv kernel=)
FLAVOURS = {
    "p16": ("jss_packed_kernel<16, ", [(16, 8), (9, 6), (3, 2), (16, 5)], 37, "auto"),
    "p32": ("jss_packed_kernel<32, ", [(32, 8), (17, 6), (3, 2), (20, 12)], 21, "auto"),
    "w1": ("jss_kernel<1, ", [(64, 8), (33, 6), (3, 2), (40, 12)], 13, "auto"),
    "w2": ("jss_kernel<2, ", [(128, 16), (65, 8), (3, 2), (70, 12)], 11, "auto"),
    "two": ("jss_kernel_two<", [(64, 8), (33, 6), (3, 2), (40, 12)], 13, "wave-2env"),
}
# the one instance of a shared-table batch: at the flavour's limit, then below it (inside the lanes' padding)
SHARED_SHAPES = {"p16": [(16, 8), (11, 8)], "p32": [(32, 8), (23, 12)], "w1": [(64, 8), (47, 16)], "w2": [(128, 16), (65, 16)]}
SESSION_KERNELS = {"p16": "jss_packed_session_kernel<16, ", "p32": "jss_packed_session_kernel<32, ", "w1": "jss_session_kernel<1, ",
                   "w2": "jss_session_kernel<2, "}
K_STEPS = 12          # iterations of the mode per recipe
STEPPING = ("step", "rollout", "rollout1", "trajectory", "steps", "session", "logits")


class Recipe:
    def __init__(self, kernel, flavour, tab, mode):
        self.kernel, self.flavour, self.tab, self.mode = kernel, flavour, tab, mode
        # (the helper kernels every session launches next to its resident kernel)
        self.also = ("jss_session_post_kernel", "jss_session_wait_kernel") if mode == "session" else ()
        self.id = f"{flavour}-{TABS[tab]}-{mode}"

    def __repr__(self):
        return self.id


def recipes():
    out = []
    for fl, (prefix, _, _, _) in FLAVOURS.items():
        for tab in TABS:
            if fl == "two":                          # pick_two: per-env tables, the one-step modes
                out += [Recipe(f"{prefix}{m}, {tab}>", fl, tab, MODES[m]) for m in (1, 5) if tab not in SHARED]
                continue
            out += [Recipe(f"{prefix}{m}, {tab}>", fl, tab, name) for m, name in MODES.items()]
            out.append(Recipe(f"{SESSION_KERNELS[fl]}{tab}>", fl, tab, "session"))
    return out


def _instance(rng, J, M, wide, name):
    if not wide:
        return P.random_instance(rng, J, M, name=name)
    machine = np.stack([rng.permutation(M) for _ in range(J)]).astype(np.int32)
    duration = (65535 - rng.integers(0, 3, size=(J, M))).astype(np.int32)
    return I.Instance(name, machine, duration)


def variants(r):
    """the runs of a recipe: one per shape of a shared-table batch, one for per-env tables"""
    return range(len(SHARED_SHAPES[r.flavour])) if r.tab in SHARED else range(1)


def recipe_env_args(r, variant=0):
    """(instances, BatchedJssEnv keyword arguments) of a recipe."""
    _, shapes, batch, kernel = FLAVOURS[r.flavour]
    rng = np.random.default_rng([r.tab, MODE_NUMBER[r.mode], variant])
    if r.tab in SHARED:
        J, M = SHARED_SHAPES[r.flavour][variant]
        insts = [_instance(rng, J, M, r.tab == 2 and variant == 0, f"{r.flavour}_shared_{J}x{M}")]
        kw = dict(compact=(r.tab == 2))
    else:
        insts = [_instance(rng, *shapes[i % len(shapes)], r.tab == 3 and i % 4 != 1, f"{r.flavour}_{i}") for i in range(batch)]
        kw = dict(records="medium" if r.tab == 3 else "full")
    return insts, dict(batch=batch, seed=SEED, env_id_base=ID_BASE, kernel=kernel, order="interleaved", **kw)


class Lockstep:
    """The oracles of a batch, one per env, what the env's counters owe (steps, episodes, makespan sum, reward numerators), the
    NOPEs taken and every env's last iteration (acted, reward, done)."""

    def __init__(self, env, insts):
        self.env = env
        self.orcs = [OracleEnv(insts[t], strict=False) for t in env.table_of_env_host]
        for o in self.orcs:
            o.reset()
        self.counters = np.zeros((env.batch, 4), dtype=np.int64)
        self.nopes = 0
        self.last = [(False, 0.0, False)] * env.batch

    def done(self, i):
        return self.orcs[i].nb_legal_actions == 0

    def first_episode_lengths(self, insts, kind="random"):
        out = []
        for i, t in enumerate(self.env.table_of_env_host):
            o, n = OracleEnv(insts[t]), 0
            o.reset()
            while o.nb_legal_actions:
                o.step(o.policy(kind, seed=SEED, env_id=ID_BASE + i, episode=1, step=n))
                n += 1
            out.append(n)
        return out

    def step(self, i, a):
        o = self.orcs[i]
        _, r, d, _, _ = o.step(int(a))
        self.nopes += int(a) == o.jobs
        self.counters[i] += (1, int(d), o.current_time_step if d else 0, o.last_reward_numerator)
        self.last[i] = (True, r, d)
        return r, d

    def policy_iteration(self, i, kind, explore, autoreset):
        """one iteration of rollout / trajectory on env i's oracle -> (action code, reward, done)"""
        o = self.orcs[i]
        if o.nb_legal_actions == 0:
            self.last[i] = (False, 0.0, True)
            if autoreset:
                o.reset()
                return _abi.ACTION_RESET, 0.0, False
            return _abi.ACTION_SKIP, 0.0, True
        a = o.policy(kind, seed=SEED, env_id=ID_BASE + i, episode=o.episode, step=o.step_in_episode, explore=explore)
        r, d = self.step(i, a)
        return a, r, d

    def given_action(self, i, a):
        """the oracle's side of a step code (job, NOPE, -1 skip, -2 reset) -> (reward, done) as jss_steps records them"""
        o = self.orcs[i]
        if a >= 0:
            return self.step(i, a)
        self.last[i] = (False, 0.0, False)
        if a == _abi.ACTION_RESET:
            o.reset()
        return 0.0, o.nb_legal_actions == 0

    def choose(self, rng, i, when_done):
        o = self.orcs[i]
        if o.nb_legal_actions == 0:
            return when_done
        legal = o.legal_actions
        if legal[-1] and rng.random() < 0.5:
            return o.jobs
        return int(rng.choice(np.flatnonzero(legal)))

    def assert_state(self, where, outputs=True, rng_position=True, fresh_col0=True):
        for i, o in enumerate(self.orcs):
            h = self.env.host_state(i)
            P.assert_matches_oracle(h, o, f"{where} env {i} ({o.instance.name})", fresh_col0=fresh_col0, check_outputs=outputs)
            if rng_position:
                assert (h["episode"], h["step_in_episode"]) == (o.episode, o.step_in_episode), f"{where} env {i}: RNG position"

    def assert_outputs(self, where, acted=None, reward=None, done=None):
        """env.reward / env.done of every env that acted in the last iteration (a skipped or restarted env keeps or clears its
        outputs as the call documents: not compared here)"""
        n = self.env.backend.numpy
        rew, dn = n(self.env.reward), n(self.env.done)
        for i in range(self.env.batch):
            a, r, d = self.last[i] if acted is None else (acted[i], reward[i], done[i])
            if a:
                assert P.reward_close(float(rew[i]), r), f"{where} env {i}: reward {rew[i]} vs {r}"
                assert bool(dn[i]) == bool(d), f"{where} env {i}: done"


def warm_start(r, backend, insts, kw):
    """env on `backend` and its oracles: the even envs about K_STEPS / 2 iterations before the median env ends its first
    episode, the odd envs restarted half an episode ago"""
    env = BatchedJssEnv(insts, _backend=backend, **kw)
    env.reset()
    ls = Lockstep(env, insts)
    lengths = sorted(ls.first_episode_lengths(insts)[0::2])       # (of the even envs: the median one of them is 4 steps from its end)
    median = lengths[len(lengths) // 2]
    half = median // 2
    first = max(0, median - 4 - half)
    odd = (np.arange(env.batch) % 2).astype(np.uint8)
    twin = BatchedJssEnv(insts, _backend=CpuBackend(), **kw)
    twin.reset()
    twin.rollout("random", n_iter=first, autoreset=True)
    twin.reset(which=odd)
    twin.rollout("random", n_iter=half, autoreset=True)
    twin.synchronize()
    env.load_state_dict(twin.state_dict())
    twin.close()
    for i, o in enumerate(ls.orcs):
        for _ in range(first):
            ls.policy_iteration(i, "random", 0.0, True)
        if odd[i]:
            o.reset()
        for _ in range(half):
            ls.policy_iteration(i, "random", 0.0, True)
    return env, ls


def run_recipe(r, backend, emulator=False):
    for variant in variants(r):
        insts, kw = recipe_env_args(r, variant)
        env, ls = warm_start(r, backend, insts, kw)
        what = f"{r.id} ({insts[0].name})" if r.tab in SHARED else r.id
        rng = np.random.default_rng([MODE_NUMBER[r.mode], r.tab, variant])
        n = backend.numpy
        before, counters0, owed0, ls.nopes = [o.episode for o in ls.orcs], n(env.counters).copy(), ls.counters.copy(), 0
        MODE_CALLS[r.mode](what, env, ls, rng, emulator, insts)
        env.synchronize()
        if r.mode in STEPPING:
            ended = sum(o.episode > e or o.nb_legal_actions == 0 for o, e in zip(ls.orcs, before))
            assert ended > 0, f"{what}: no env finished an episode inside the call -- the recipe misses its edge"
            assert ls.nopes > 0, f"{what}: no NOPE was taken inside the call -- the recipe misses its edge"
            ls.assert_outputs(what + " after the call")
        # steps, episodes, makespan sum and the exact integer reward numerators the call added
        assert np.array_equal(n(env.counters) - counters0, ls.counters - owed0), \
            f"{what}: counters\n got={(n(env.counters) - counters0).tolist()}\nwant={(ls.counters - owed0).tolist()}"
        # (a direct increase_time_step: the reference refreshes column 0 of its observation only inside step() and reset(),
        #  jss_env.py:130 -- the other six columns are compared, as in golden_util.replay)
        ls.assert_state(what, outputs=r.mode not in ("reset", "advance", "policy", "lookahead"), fresh_col0=r.mode != "advance")
        env.close()


def _mode_reset(r, env, ls, rng, emulator, insts):
    which = (np.arange(env.batch) % 3 != 1).astype(np.uint8)
    env.reset(which=which)
    for i in np.flatnonzero(which):
        ls.orcs[i].reset()
    ls.assert_state(r + " partial reset", outputs=False, rng_position=False)
    env.reset()
    for o in ls.orcs:
        o.reset()


def _mode_advance(r, env, ls, rng, emulator, insts):
    for _ in range(3):
        which = np.array([i % 2 == 0 and len(o.next_time_step) > 0 for i, o in enumerate(ls.orcs)], dtype=np.uint8)
        hole = env.backend.numpy(env.increase_time_step(which=which))
        for i in np.flatnonzero(which):
            assert int(hole[i]) == ls.orcs[i].increase_time_step(), f"{r} env {i}: hole_planning"


def _mode_policy(r, env, ls, rng, emulator, insts):
    for kind, explore in (("random", 0.0), ("FIFO", 0.0), ("SPT", 0.3), ("MWR", 0.0), ("LWR", 0.0), ("MOR", 0.0), ("LOR", 0.0), ("CR", 0.0)):
        acts = env.backend.numpy(env.policy(kind, explore=explore)).astype(np.int64)
        for i, o in enumerate(ls.orcs):
            if o.nb_legal_actions:
                want = o.policy(kind, seed=SEED, env_id=ID_BASE + i, episode=o.episode, step=o.step_in_episode, explore=explore)
                assert acts[i] == want, f"{r} env {i}: policy {kind} chose {acts[i]}, the oracle {want}"


def _mode_step(r, env, ls, rng, emulator, insts):
    B = env.batch
    for k in range(K_STEPS):
        autoreset = k < K_STEPS - 4                  # the last iterations: done envs are skipped, frozen
        acts = np.array([ls.choose(rng, i, _abi.ACTION_SKIP) for i in range(B)], dtype=np.int32)
        was_done = [ls.done(i) for i in range(B)]
        env.step(acts, autoreset=autoreset)
        rew, done = [0.0] * B, [False] * B
        for i in range(B):
            if was_done[i]:
                if autoreset:
                    ls.orcs[i].reset()
                else:
                    rew[i] = None
            else:
                rew[i], done[i] = ls.given_action(i, acts[i])
        ls.assert_outputs(f"{r} iteration {k}", [x is not None for x in rew], rew, done)


def _mode_rollout(r, env, ls, rng, emulator, insts, chunks=(K_STEPS - 4, 4)):
    for chunk, autoreset, kind, explore in ((chunks[0], True, "SPT", 0.5), (chunks[1], False, "random", 0.0)):
        env.rollout(kind, n_iter=chunk, explore=explore, autoreset=autoreset)
        for i in range(env.batch):
            for _ in range(chunk):
                ls.policy_iteration(i, kind, explore, autoreset)
        ls.assert_outputs(f"{r} after {chunk} iterations of {kind}")


def _mode_rollout1(r, env, ls, rng, emulator, insts):
    for k in range(K_STEPS):
        autoreset, kind, explore = k < K_STEPS - 4, ("random", "MWR")[k % 2], 0.5 * (k % 2)
        env.rollout(kind, n_iter=1, explore=explore, autoreset=autoreset)
        out = [ls.policy_iteration(i, kind, explore, autoreset) for i in range(env.batch)]
        ls.assert_outputs(f"{r} iteration {k}", [a >= 0 for a, _, _ in out], [x[1] for x in out], [x[2] for x in out])


def _mode_trajectory(r, env, ls, rng, emulator, insts):
    n = env.backend.numpy
    for steps, autoreset, kind, explore in ((K_STEPS - 4, True, "SPT", 0.5), (4, False, "random", 0.0)):
        tr = {k: n(v) for k, v in env.trajectory(kind, steps=steps, explore=explore, autoreset=autoreset).items()}
        for i, o in enumerate(ls.orcs):
            J = o.jobs
            for k in range(steps):
                where = f"{r} slot {k} env {i}"
                obs, mask = o.state, o.legal_actions
                a, rew, done = ls.policy_iteration(i, kind, explore, autoreset)
                assert np.abs(tr["real_obs"][k, i, :J].astype(np.float64) - obs).max() <= P.OBS_TOL, f"{where}: observation"
                assert not tr["real_obs"][k, i, J:].any(), f"{where}: padding rows"
                assert np.array_equal(tr["action_mask"][k, i, :J + 1].astype(bool), mask), f"{where}: mask"
                assert tr["action"][k, i] == a, f"{where}: action {tr['action'][k, i]} vs {a}"
                assert P.reward_close(float(tr["reward"][k, i]), rew), f"{where}: reward"
                assert bool(tr["done"][k, i]) == bool(done), f"{where}: done"


def _given_actions(ls, rng, K, B):
    """(K, B) action codes chosen against the oracles, which are stepped along: random legal jobs, NOPE half of the time it
    is legal, -2 for an env that is done (the last steps: -1), a skip now and then; and the records jss_steps owes"""
    acts = np.zeros((K, B), dtype=np.int32)
    want = []
    for k in range(K):
        row = []
        for i in range(B):
            a = ls.choose(rng, i, _abi.ACTION_RESET if k < K - 4 else _abi.ACTION_SKIP)
            if a >= 0 and rng.random() < 0.1:
                a = _abi.ACTION_SKIP
            acts[k, i] = a
            rew, done = ls.given_action(i, a)
            o = ls.orcs[i]
            row.append((o.state, o.legal_actions, rew, done))
        want.append(row)
    return acts, want


def _mode_steps(r, env, ls, rng, emulator, insts):
    n = env.backend.numpy
    acts, want = _given_actions(ls, rng, K_STEPS, env.batch)
    rec = {k: n(v) for k, v in env.steps(acts, record=("real_obs", "action_mask", "reward", "done")).items()}
    for k in range(K_STEPS):
        for i, o in enumerate(ls.orcs):
            obs, mask, rew, done = want[k][i]
            where, J = f"{r} step {k} env {i} action {acts[k, i]}", o.jobs
            assert np.abs(rec["real_obs"][k, i, :J].astype(np.float64) - obs).max() <= P.OBS_TOL, f"{where}: recorded observation"
            assert np.array_equal(rec["action_mask"][k, i, :J + 1].astype(bool), mask), f"{where}: recorded mask"
            assert P.reward_close(float(rec["reward"][k, i]), rew), f"{where}: recorded reward {rec['reward'][k, i]} vs {rew}"
            assert bool(rec["done"][k, i]) == bool(done), f"{where}: recorded done"


def _mode_session(r, env, ls, rng, emulator, insts):
    K, B = K_STEPS, env.batch
    acts, _ = _given_actions(ls, rng, K, B)       # (the session records nothing: run_recipe compares the outputs it leaves)
    # env sets per wavefront (0: the library chooses), by layout: 1 = in registers, 2 = parked in LDS between visits
    slots = {(True, _abi.NF): 0, (False, _abi.NF): 2, (True, _abi.NFC): 1, (False, _abi.NFM): 2}[(env.n_tables == 1, env.record_ints)]
    if not emulator:
        dev = (lambda a: env.backend.as_device(a, "int32")) if hasattr(env.backend, "torch") else (lambda a: a)
        with env.session(depth=K, slots=slots, timeout_ms=5000) as s:
            s.post(dev(acts[:5]))
            s.wait()
            s.post(dev(acts[5:-1]))
            s.wait()
            s.step(dev(acts[-1]))         # post + wait in one launch: jss_session_step_kernel on the GPU
        return
    # under the emulator a launch runs to completion: the mailbox is filled first, then the session opened (P.case_session_emulator)
    lib = env.backend.lib
    mail, progress, status = np.zeros((K + 1, B), dtype=np.int64), np.zeros(B, dtype=np.int32), np.zeros(4, dtype=np.int32)
    sess = _abi.JssSession(mail.ctypes.data, progress.ctypes.data, status.ctypes.data, K + 1, 2000, slots, 0)
    d, s, o = env._refs()
    a = np.ascontiguousarray(acts, dtype=np.int32)
    _abi.check(lib, lib.jss_session_post(d, C.byref(sess), a.ctypes.data, 0, K, 0, 0), "post")
    _abi.check(lib, lib.jss_session_close(d, C.byref(sess), K, 0), "close")
    _abi.check(lib, lib.jss_session_open(d, s, o, C.byref(sess), 0), "open")
    _abi.check(lib, lib.jss_session_wait(d, C.byref(sess), K, 0), "wait")
    assert status[0] == 0 and status[1] == 0 and status[2] > 0, status
    assert (progress[:status[2]] == K).all(), progress


def _mode_logits(r, env, ls, rng, emulator, insts):
    B, W = env.batch, env.jmax + 1
    for k in range(K_STEPS):
        autoreset, T = k < K_STEPS - 4, (1.0, 0.0, 0.5)[k % 3]
        logits = L.random_logits(rng, B, W, ties=(k % 4 == 3))
        odd = np.arange(1, B, 2)
        logits[odd, env.jobs_per_env[odd]] += 4.0          # NOPE favoured in the odd envs (not forced: jobs are drawn there too)
        was_done = [ls.done(i) for i in range(B)]
        ctx, act, logp, ent = L.step_and_check(env, logits, T, SEED, autoreset=autoreset, check_state=False)
        L.check_draw(ctx, logits, act, logp, ent, T, SEED, autoreset=autoreset)
        rew, done = [None] * B, [False] * B
        for i in range(B):
            if was_done[i]:
                assert act[i] == (_abi.ACTION_RESET if autoreset else _abi.ACTION_SKIP), f"{r} step {k} env {i}: {act[i]}"
                if autoreset:
                    ls.orcs[i].reset()
            else:
                assert ls.orcs[i].legal_actions[act[i]], f"{r} step {k} env {i}: drew the illegal action {act[i]}"
                rew[i], done[i] = ls.given_action(i, act[i])
        ls.assert_outputs(f"{r} iteration {k}", [x is not None for x in rew], rew, done)


def _mode_lookahead(r, env, ls, rng, emulator, insts):
    """candidates of every env: one legal job, NOPE (legal or not), a skip, an out-of-range action -- then SPT for at most
    2 * K_STEPS iterations; the oracle replays each parent (reset, the same warm rollout) and does the same"""
    par, act = [], []
    for i, o in enumerate(ls.orcs):
        legal = np.flatnonzero(o.legal_actions[:-1])
        cands = ([int(rng.choice(legal))] if len(legal) else [0]) + [o.jobs, -1, env.jmax + 1]
        par += [i] * len(cands)
        act += cands
    n_iter = 2 * K_STEPS
    ms, st, ret = env.lookahead("SPT", actions=np.array(act, np.int32), parents=np.array(par, np.int32), n_iter=n_iter, seed=SEED)
    n = env.backend.numpy
    ms, st, ret = n(ms), n(st), n(ret)
    ended = 0
    for c, (i, a) in enumerate(zip(par, act)):
        p = ls.orcs[i]
        ok = p.nb_legal_actions > 0 and (a == -1 or (0 <= a <= p.jobs and bool(p.legal_actions[a])))
        if not ok:
            assert (ms[c], st[c], ret[c]) == (-1, 0, 0), f"{r} candidate {c}: nothing to evaluate, got {(ms[c], st[c], ret[c])}"
            continue
        o = OracleEnv(insts[env.table_of_env_host[i]])
        o.reset()
        o.episode = 1
        while (o.episode, o.step_in_episode) != (p.episode, p.step_in_episode):
            if o.nb_legal_actions == 0:
                o.reset()
            else:
                o.step(o.policy("random", seed=SEED, env_id=ID_BASE + i, episode=o.episode, step=o.step_in_episode))
        steps, total = 0, 0.0
        if a != -1:
            _, rew, _, _, _ = o.step(a)
            steps, total = 1, rew
        for _ in range(n_iter):
            if o.nb_legal_actions == 0:
                break
            _, rew, _, _, _ = o.step(o.policy("SPT"))
            steps, total = steps + 1, total + rew
        done = o.nb_legal_actions == 0
        ended += done
        where = f"{r} candidate {c} (env {i}, action {a})"
        assert ms[c] == (o.current_time_step if done else -1), f"{where}: makespan {ms[c]}"
        assert st[c] == steps, f"{where}: steps {st[c]} vs {steps}"
        assert P.reward_close(float(ret[c]), total), f"{where}: return {ret[c]} vs {total}"
    assert ended, f"{r}: no candidate reached the end of its episode"


MODE_CALLS = {"reset": _mode_reset, "step": _mode_step, "advance": _mode_advance, "policy": _mode_policy, "rollout": _mode_rollout,
              "rollout1": _mode_rollout1, "trajectory": _mode_trajectory, "steps": _mode_steps, "session": _mode_session,
              "logits": _mode_logits, "lookahead": _mode_lookahead}
