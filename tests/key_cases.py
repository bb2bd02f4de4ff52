"""Backend-agnostic cases of the per-operation priority keys (include/jss_keys.h): jss_key_policy / jss_key_rollout /
jss_key_lookahead through BatchedJssEnv.policy / rollout / lookahead / pilot_step(kind="keys", keys=..., nope_key=...).  Each
case takes a backend -- the CPU twin, the kernel source under the emulator, the HIP library -- like rule_cases.py, whose
shapes these cases use."""
import ctypes as C

import numpy as np

import clone_cases as K
import lookahead_cases as L
import rule_cases as R
from jssenv_amd import BatchedJssEnv, _abi
from jssenv_amd.dispatching import keys_from_actions, rule_keys
from oracle import OracleEnv

SHAPES = R.SHAPES
STOCK = ("SPT", "MWR", "LWR", "MOR", "LOR")       # the stock rules that are a table per operation
I32_MIN, I32_MAX = -2**31, 2**31 - 1
snapshot, same, make_shape = R.snapshot, R.same, R.make_shape


def padded(env, inst, table, fill=0):
    """a (J, M) table of `inst` in the batch's padded extents; the padding holds `fill`"""
    out = np.full((env.jmax, env.mmax), fill, dtype=np.int32)
    out[:inst.jobs, :inst.machines] = table
    return out


def one_instance(per_env):
    return all(i is per_env[0] for i in per_env)


# ---- 2. the stock rules as key tables ------------------------------------------------------------------------------------------
def case_stock_tables(be, shape, rules=STOCK, explores=(0.0, 0.5), seed=7, whole=True):
    """jss_key_rollout with rule_keys(inst, rule) and jss_rollout(rule), from the same reset with the same seed: bit-identical
    state, outputs and counters after a 7-step slice from the start, a 7-step slice mid-episode and at the end of the episode
    (whole = False, the emulator's runs: the slices only); jss_key_policy == jss_policy on the mid-episode state.  Where the batch
    has one instance the shared (jmax, mmax) form and the per-env (B, jmax, mmax) form alternate; elsewhere the tables are
    built per env."""
    env_k, per_env = make_shape(be, shape)
    env_t, _ = make_shape(be, shape)
    rest = 3 * env_k.jmax * env_k.mmax
    for n, rule in enumerate(rules):
        tables = np.stack([padded(env_t, inst, rule_keys(inst, rule)) for inst in per_env])
        keys = tables[0] if one_instance(per_env) and n % 2 == 0 else tables
        for explore in explores:
            for e in (env_k, env_t):
                e.reset()
                e.zero_counters()
            for n_iter in (7, 9, 7, rest) if whole else (7, 9, 7):
                env_k.rollout(rule, n_iter=n_iter, seed=seed, explore=explore, autoreset=False)
                env_t.rollout("keys", n_iter=n_iter, seed=seed, explore=explore, autoreset=False, keys=keys)
                same(snapshot(env_k), snapshot(env_t), (shape, rule, explore, n_iter))
                if n_iter == 9:
                    a = L.host(env_k.policy(rule, seed=seed + 1, explore=explore))
                    b = L.host(env_t.policy("keys", seed=seed + 1, explore=explore, keys=keys))
                    assert np.array_equal(a, b), (shape, rule, explore)
            assert not whole or K.host(env_t, "done").all()


def case_golden(be):
    """SPT as a key table reproduces the committed golden table of the reference's rules: ta41 2499, ta01 1462"""
    for inst, want in (("ta41", 2499), ("ta01", 1462)):
        env = BatchedJssEnv(inst, batch=3, _backend=be, seed=1)
        env.reset()
        env.rollout("keys", n_iter=3 * env.jmax * env.mmax, autoreset=False, keys=rule_keys(inst, "SPT"))
        assert K.host(env, "makespan").tolist() == [want] * 3, inst


# ---- 3. random tables against the oracle -----------------------------------------------------------------------------------------
def yardstick(orc, inst, table, nope_key, trace):
    """The definition of include/jss_keys.h over OracleEnv's legal_actions and todo_time_step_job (not KeyRule, not the twin).
    table: at least (J, M).  trace: counts of NOPEs taken while a job was legal, and of choices decided by the tie rule."""
    legal = orc.legal_actions
    J = inst.jobs
    jobs = [j for j in range(J) if legal[j]]
    if not jobs:
        return J if legal[J] else -1
    todo = orc.todo_time_step_job
    key = {j: int(table[j, int(todo[j])]) for j in jobs}
    best = max(key.values())
    winners = [j for j in jobs if key[j] == best]
    if len(winners) > 1:
        trace["ties"] += 1
    if legal[J] and int(nope_key) > best:
        trace["nopes"] += 1
        return J
    return winners[0]


def random_tables(env, nope_key, seed=5):
    """one table per env from [-2, 2]: NOPE-happy under nope_key = 2 (it exceeds every key but 2); env 1's table is all 2 then,
    NOPE-free (nothing exceeds it: every choice a tie, the lowest legal index)"""
    rng = np.random.default_rng(seed)
    t = rng.integers(-2, 3, size=(env.batch, env.jmax, env.mmax)).astype(np.int32)
    if nope_key == 2:
        t[1] = 2
    return t


def play_against_yardstick(be, env, per_env, tables, nope_key, max_steps=None):
    """every action of every env, the final makespan and the solution equal the yardstick stepped through OracleEnv.step; then
    the same tables played by ONE jss_key_rollout give the same makespans.  Returns the yardstick's trace."""
    env.reset()
    orcs = [OracleEnv(inst, strict=True) for inst in per_env]
    for o in orcs:
        o.reset()
    trace = {"ties": 0, "nopes": 0}
    for step in range(4 * env.jmax * env.mmax):
        if max_steps is not None and step == max_steps:
            return trace
        want = np.array([yardstick(o, inst, tables[i], nope_key, trace) for i, (o, inst) in enumerate(zip(orcs, per_env))], np.int32)
        got = L.host(env.policy("keys", keys=tables, nope_key=nope_key))
        assert np.array_equal(got, want), (step, got, want)
        if (want < 0).all():
            break
        env.step(want)
        for o, a in zip(orcs, want):
            if a >= 0:
                o.step(int(a))
    else:
        raise AssertionError("episodes did not finish")
    sol, ms = K.host(env, "solution"), K.host(env, "makespan")
    for i, (o, inst) in enumerate(zip(orcs, per_env)):
        assert ms[i] == o.current_time_step, i
        assert np.array_equal(sol[i, :inst.jobs, :inst.machines], o.solution), i
    env.reset()
    env.rollout("keys", n_iter=4 * env.jmax * env.mmax, autoreset=False, keys=tables, nope_key=nope_key)
    assert np.array_equal(K.host(env, "makespan"), ms)
    return trace


def case_random_tables(be, shape, nope_key, max_steps=None):
    env, per_env = make_shape(be, shape)
    return play_against_yardstick(be, env, per_env, random_tables(env, nope_key), nope_key, max_steps)


# ---- 4. extremes -------------------------------------------------------------------------------------------------------------------
def poison(env, per_env, tables, value):
    """the padded entries (j >= J(env), k >= M(env)) of per-env tables overwritten with `value`: they would win if read"""
    t = tables.copy()
    for i, inst in enumerate(per_env):
        t[i, inst.jobs:, :] = value
        t[i, :, inst.machines:] = value
    return t


def case_extremes(be, shape, max_steps=None):
    """All INT32_MIN: the lowest legal index wins and NOPE is never chosen while a job is legal (nope_key INT32_MIN exceeds
    nothing); all INT32_MAX with nope_key INT32_MAX: the same actions.  INT32_MIN and INT32_MAX mixed in one env (with keys
    between, nope_key 0) is held to the yardstick.  The padded entries of ragged envs hold INT32_MAX, which would win if read."""
    env, per_env = make_shape(be, shape)
    B = env.batch
    shape3 = (B, env.jmax, env.mmax)
    for fill, nope in ((I32_MIN, None), (I32_MAX, I32_MAX)):
        t = poison(env, per_env, np.full(shape3, fill, dtype=np.int32), I32_MAX)
        env.reset()
        for step in range(4 * env.jmax * env.mmax):
            if max_steps is not None and step == max_steps:
                break
            mask = K.host(env, "action_mask")
            want = np.array([next((j for j in range(inst.jobs) if mask[i, j]), inst.jobs if mask[i, inst.jobs] else -1)
                             for i, inst in enumerate(per_env)], np.int32)
            got = L.host(env.policy("keys", keys=t, nope_key=nope))
            assert np.array_equal(got, want), (shape, fill, step, got, want)
            if (want < 0).all():
                break
            env.step(want)
        else:
            raise AssertionError("episodes did not finish")
    rng = np.random.default_rng(9)
    mixed = rng.choice(np.array([I32_MIN, I32_MIN + 1, -1, 0, 1, I32_MAX - 1, I32_MAX], dtype=np.int64), size=shape3).astype(np.int32)
    return play_against_yardstick(be, env, per_env, poison(env, per_env, mixed, I32_MAX), 0, max_steps)


# ---- 5. replay -------------------------------------------------------------------------------------------------------------------------
def case_replay(be, shape, rules=("SPT", "MWR", "FIFO")):
    """An episode of a stock rule, recorded by `trajectory`, turned into keys by keys_from_actions and played by
    rollout("keys"): solution, makespan and step count identical on every env.  Only episodes without exploration are
    replayed: one with voluntary NOPEs is outside what keys_from_actions promises (a table says which job goes first, never
    when to wait), so none is played and nothing is asserted on one."""
    env, per_env = make_shape(be, shape)
    n = 3 * env.jmax * env.mmax
    for rule in rules:
        env.reset()
        env.zero_counters()
        rec = env.trajectory(rule, steps=n, autoreset=False)
        actions = L.host(rec["action"])
        assert K.host(env, "done").all()
        want = {k: K.host(env, k).copy() for k in ("solution", "makespan", "counters")}
        tables = np.stack([padded(env, inst, keys_from_actions(inst, actions[:, i])) for i, inst in enumerate(per_env)])
        env.reset()
        env.zero_counters()
        env.rollout("keys", n_iter=n, autoreset=False, keys=tables)
        assert K.host(env, "done").all()
        assert np.array_equal(K.host(env, "solution"), want["solution"]), (shape, rule)
        assert np.array_equal(K.host(env, "makespan"), want["makespan"]), (shape, rule)
        assert np.array_equal(K.host(env, "counters")[:, 0], want["counters"][:, 0]), (shape, rule)


# ---- 6. lookahead ------------------------------------------------------------------------------------------------------------------------
def case_lookahead(be, shape="p16-J11", per_parent=None, seed=4, n_iter=None, explores=(0.0, 0.4)):
    """jss_key_lookahead == fork + step + jss_key_rollout with the parents' tables, bit for bit (makespan, steps, reward
    numerators): shared table and per-parent tables, candidates parent-major and shuffled, a done parent and illegal actions
    among them; pilot_step(keys=...) takes the arg-min action."""
    env, _ = make_shape(be, shape)
    B = env.batch
    rng = np.random.default_rng(seed)
    env.reset()
    K.drive(env, rng, 12)
    done_one = np.zeros(B, np.uint8)
    done_one[B - 1] = 1                                                  # ... and one parent played to the end
    for _ in range(4 * env.jmax * env.mmax):
        a = L.host(env.policy("SPT")).copy()
        a[done_one == 0] = -1
        if (a < 0).all():
            break
        env.step(a)
    assert K.host(env, "done")[B - 1]
    before = snapshot(env)
    par, act, legal = L.candidates(env, rng, per_parent)
    assert (~legal).any() and legal.any()
    tables = random_tables(env, 2, seed + 1)
    n_iter = 3 * env.jmax * env.mmax if n_iter is None else n_iter        # (short: candidates that do not finish score -1)
    for t, nope in ((tables, 2), (tables[0], None)):
        for order in (np.arange(len(par)), rng.permutation(len(par))):
            p, a, ok = par[order], act[order], legal[order]
            for explore in explores:
                ms, st, ret = env.lookahead("keys", actions=a, parents=p, seed=9, explore=explore, id_base=100, keys=t,
                                            nope_key=nope, n_iter=n_iter)
                f = env.fork(p, env_id_base=100)
                f.zero_counters()
                f.step(np.where(ok, a, -1).astype(np.int32))
                f.rollout("keys", n_iter=n_iter, seed=9, explore=explore, autoreset=False, keys=t if t.ndim == 2 else t[p],
                          nope_key=nope)
                done, fms, cn = K.host(f, "done"), K.host(f, "makespan"), K.host(f, "counters")
                assert np.array_equal(L.host(ms), np.where(ok & (done != 0), fms, -1)), shape
                assert np.array_equal(L.host(st), np.where(ok, cn[:, 0], 0)), shape
                mto = K.host(env, "env_const")[p, _abi.C_MAX_TIME_OP].astype(np.float64)
                want_ret = np.where(ok, cn[:, 3] / mto, 0.0).astype(np.float32)
                assert np.array_equal(L.host(ret), want_ret), shape
                assert (L.host(ms)[~ok] == -1).all() and (L.host(st)[~ok] == 0).all()
    same(before, snapshot(env), "lookahead wrote into the batch")
    if n_iter != 3 * env.jmax * env.mmax:
        return
    scores = L.host(env.lookahead("keys", keys=tables, nope_key=2)[0])
    _, _, _, _, info = env.pilot_step("keys", keys=tables, nope_key=2)
    free = scores < 0
    want = np.where(free.all(axis=1), -1, np.where(free, 2**31 - 1, scores).argmin(axis=1))
    assert np.array_equal(L.host(info["action"]), want) and np.array_equal(L.host(info["scores"]), scores)
    assert want[B - 1] == -1


# ---- 1. the boundary -----------------------------------------------------------------------------------------------------------------
def argument_rows():
    """(name, call, expected code, build(world) -> args): the argument errors of the three jss_key_* calls"""
    def parts(w, d=None, keys=None, null=()):
        desc = _abi.JssDesc(batch=2, jmax=4, mmax=3, n_tables=1, ops=w.p(), rem=w.p(), inst=w.p())
        for k, v in (d or {}).items():
            setattr(desc, k, v)
        st = _abi.JssState(*(w.p() for _ in range(6)))
        out = _abi.JssOut(*(w.p() for _ in range(5)))
        r = _abi.JssKeys(w.p(), 12, 0)
        for k, v in (keys or {}).items():
            setattr(r, k, v)
        look = _abi.JssLookahead(n=3, parent=w.p(), action=w.p(), id_base=0, makespan=w.p(), steps=w.p(), reward_num=w.p())
        return desc, st, out, (None if "keys" in null else C.byref(r)), look, w.p()

    def policy(w, **kw):
        d, s, _, r, _, acts = parts(w, **kw)
        return C.byref(d), C.byref(s), r, 0, 0, (None if kw.get("null") == ("actions",) else acts), None

    def rollout(w, n_iter=5, **kw):
        d, s, o, r, _, _ = parts(w, **kw)
        return C.byref(d), C.byref(s), C.byref(o), r, 0, 0, n_iter, 0, None

    def lookahead(w, n_iter=5, **kw):
        d, s, _, r, la, _ = parts(w, **kw)
        return C.byref(d), C.byref(s), C.byref(la), r, 0, 0, n_iter, None

    rows = []
    for call, build in (("jss_key_policy", policy), ("jss_key_rollout", rollout), ("jss_key_lookahead", lookahead)):
        rows.append((f"{call}-null-struct", call, _abi.E_NULL, lambda w, b=build: b(w, null=("keys",))))
        rows.append((f"{call}-null-keys", call, _abi.E_NULL, lambda w, b=build: b(w, keys={"keys": None})))
        rows.append((f"{call}-stride-8", call, _abi.E_SHAPE, lambda w, b=build: b(w, keys={"stride": 8})))
        rows.append((f"{call}-stride-negative", call, _abi.E_SHAPE, lambda w, b=build: b(w, keys={"stride": -12})))
        # the namesake's own checks come first, as with `kind`
        rows.append((f"{call}-shape-before-keys", call, _abi.E_SHAPE, lambda w, b=build: b(w, d={"jmax": 0}, null=("keys",))))
    rows.append(("jss_key_policy-null-actions", "jss_key_policy", _abi.E_NULL, lambda w: policy(w, null=("actions",))))
    rows.append(("jss_key_rollout-keys-before-n-iter", "jss_key_rollout", _abi.E_NULL, lambda w: rollout(w, n_iter=-1, null=("keys",))))
    rows.append(("jss_key_rollout-n-iter-negative", "jss_key_rollout", _abi.E_SHAPE, lambda w: rollout(w, n_iter=-1)))
    rows.append(("jss_key_lookahead-n-iter-before-keys", "jss_key_lookahead", _abi.E_SHAPE, lambda w: lookahead(w, n_iter=-1, null=("keys",))))
    return rows


def kind9_rows():
    """kind 9 -- the launcher's own code of the key selector -- through the stock calls: still JSS_E_KIND"""
    def desc(w):
        return _abi.JssDesc(batch=2, jmax=4, mmax=3, n_tables=1, ops=w.p(), rem=w.p(), inst=w.p())

    def policy(w):
        return "jss_policy", (C.byref(desc(w)), C.byref(_abi.JssState(*(w.p() for _ in range(6)))), 9, 0, 0, w.p(), None)

    def rollout(w):
        return "jss_rollout", (C.byref(desc(w)), C.byref(_abi.JssState(*(w.p() for _ in range(6)))),
                               C.byref(_abi.JssOut(*(w.p() for _ in range(5)))), 9, 0, 0, 5, 0, None)

    def lookahead(w):
        la = _abi.JssLookahead(n=3, parent=w.p(), action=w.p(), id_base=0, makespan=w.p(), steps=w.p(), reward_num=w.p())
        return "jss_lookahead", (C.byref(desc(w)), C.byref(_abi.JssState(*(w.p() for _ in range(6)))), C.byref(la), 9, 0, 0, 5, None)
    return policy, rollout, lookahead


# ---- 7. the host mirror ----------------------------------------------------------------------------------------------------------------
def case_mirror(be, seed=5):
    """KeyRule.__call__ on the B = 1 facade agrees with jss_key_policy on every step of one random-table episode"""
    from jssenv_amd import make
    from jssenv_amd.dispatching import KeyRule
    table = np.random.default_rng(seed).integers(-2, 3, size=(15, 15)).astype(np.int32)
    env = make("jss-v1", env_config={"instance_path": "ta01"}, _backend=be)
    rule = KeyRule(table, nope_key=2)
    env.reset()
    done, steps = False, 0
    while not done:
        a = rule(env)
        # (the facade's buffers may be pinned host memory the kernel writes in place: the backend's copy waits for it)
        assert a == int(be.numpy(env._b.policy("keys", keys=table, nope_key=2))[0]), steps
        _, _, done, _, _ = env.step(a)
        steps += 1
    assert steps >= 225
