"""Backend-agnostic cases of the caller-weighted rules (include/jss_rules.h): jss_rule_policy / jss_rule_rollout /
jss_rule_lookahead through BatchedJssEnv.policy / rollout / lookahead / pilot_step(kind="weighted", weights=...).  Each case
takes a backend -- the CPU twin, the kernel source under the emulator, the HIP library -- like lookahead_cases.py."""
import ctypes as C

import numpy as np

import clone_cases as K
import lookahead_cases as L
from jssenv_amd import BatchedJssEnv, _abi
from jssenv_amd import instances as I
from jssenv_amd.dispatching import RULE_WEIGHTS
from oracle import OracleEnv

NEVER = _abi.RW_NEVER_NOPE


# ---- shapes: the smallest that reach each selector form; every batch ends in a part-filled wavefront / lane group -----------
def _inst(J, M, k=0):
    return I.taillard_instance(J, M, 11 + 2 * k, 12 + 2 * k)


def make_shape(be, name, seed=3):
    """(env, instance of every env)"""
    if name == "p16-J16":        # 16-lane groups, shared table, compact records
        insts, kw, B = [_inst(16, 5)], {}, 13
    elif name == "p16-J11":
        insts, kw, B = [_inst(11, 5)], {}, 13
    elif name == "p32-J32":      # 32-lane groups, per-env tables, medium records
        insts, kw, B = [_inst(32, 8, k) for k in range(7)], {"records": "medium"}, 7
    elif name == "p32-ragged":
        insts, kw, B = [_inst(J, 8, k) for k, J in enumerate((20, 32, 27, 21, 30, 25, 32))], {"records": "medium"}, 7
    elif name == "w1-J64":       # one wavefront per env, one job per lane, one shared table
        insts, kw, B = [_inst(64, 8)], {}, 5
    elif name == "w1-J40-map":   # ... an env -> instance map
        insts, kw, B = [_inst(40, 8, 0), _inst(40, 8, 1)], {"table_of_env": np.array([0, 1, 1, 0, 1])}, 5
    elif name == "w2-J65":       # two jobs per lane
        insts, kw, B = [_inst(65, 4)], {}, 3
    elif name == "w2-J128":
        insts, kw, B = [_inst(128, 4, k) for k in range(3)], {}, 3
    elif name == "by-shape":     # a batch dealt out by shape class (all four): the calls run on the padded extents' kernel
        env = BatchedJssEnv(K.BY_SHAPE_SMALL, batch=10, _backend=be, seed=seed)
        assert env.order == "by_shape"
        return env, [env.instances[int(t)] for t in env.table_of_env_host]
    else:
        raise KeyError(name)
    env = BatchedJssEnv(insts[0] if len(insts) == 1 else insts, batch=B, _backend=be, seed=seed, **kw)
    toe = kw.get("table_of_env")
    per_env = [insts[0] if len(insts) == 1 else insts[int(toe[i])] if toe is not None else insts[i] for i in range(B)]
    return env, per_env


SHAPES = ("p16-J16", "p16-J11", "p32-J32", "p32-ragged", "w1-J64", "w1-J40-map", "w2-J65", "w2-J128")
STOCK = tuple(RULE_WEIGHTS)                       # SPT FIFO MWR LWR MOR LOR


def snapshot(env):
    return L.snapshot(env)


def same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


# ---- 1. the stock rules as weight rows ------------------------------------------------------------------------------------------
def case_stock_rows(be, shape, rules=STOCK, explores=(0.0, 0.5), seed=7, whole=True):
    """jss_rule_rollout with a stock rule's row and jss_rollout(kind), from the same reset with the same seed: bit-identical
    state, outputs and counters after a 7-step slice from the start, a 7-step slice mid-episode and at the end of the episode
    (whole = False, the emulator's runs: the slices only); jss_rule_policy == jss_policy on the mid-episode state.  The shared
    row (8,) and the per-env form (B, 8) alternate."""
    env_k, _ = make_shape(be, shape)
    env_w, _ = make_shape(be, shape)
    rest = 3 * env_k.jmax * env_k.mmax
    for n, rule in enumerate(rules):
        row = RULE_WEIGHTS[rule]
        w = row if n % 2 == 0 else np.tile(row, (env_w.batch, 1))
        for explore in explores:
            for e in (env_k, env_w):
                e.reset()
                e.zero_counters()
            for n_iter in (7, 9, 7, rest) if whole else (7, 9, 7):
                env_k.rollout(rule, n_iter=n_iter, seed=seed, explore=explore, autoreset=False)
                env_w.rollout("weighted", n_iter=n_iter, seed=seed, explore=explore, autoreset=False, weights=w)
                same(snapshot(env_k), snapshot(env_w), (shape, rule, explore, n_iter))
                if n_iter == 9:
                    a = L.host(env_k.policy(rule, seed=seed + 1, explore=explore))
                    b = L.host(env_w.policy("weighted", seed=seed + 1, explore=explore, weights=w))
                    assert np.array_equal(a, b), (shape, rule, explore)
            assert not whole or K.host(env_w, "done").all()


def case_golden(be):
    """the weighted path reproduces the committed golden table of the reference's rules: ta01 FIFO 1486, ta41 SPT 2499"""
    for inst, rule, want in (("ta01", "FIFO", 1486), ("ta41", "SPT", 2499)):
        env = BatchedJssEnv(inst, batch=3, _backend=be, seed=1)
        env.reset()
        env.rollout("weighted", n_iter=3 * env.jmax * env.mmax, autoreset=False, weights=RULE_WEIGHTS[rule])
        assert K.host(env, "makespan").tolist() == [want] * 3, (inst, rule)


# ---- 2. mixed rows against the oracle ------------------------------------------------------------------------------------------
def wrap64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def yardstick(orc, inst, w, trace):
    """The definition of include/jss_rules.h over OracleEnv's state and the instance's durations (not WeightedRule, not the
    twin).  trace: counts of NOPEs chosen by bias while a job was legal, and of choices decided by the tie rule."""
    legal = orc.legal_actions
    J, M = inst.jobs, inst.machines
    jobs = [j for j in range(J) if legal[j]]
    if not jobs:
        return J if legal[J] else -1
    todo, wait, idle, d = orc.todo_time_step_job, orc.idle_time_jobs_last_op, orc.total_idle_time_jobs, inst.duration
    score = {}
    for j in jobs:
        t = int(todo[j])
        x = (int(d[j, t]), int(d[j, t + 1]) if t + 1 < M else 0, int(d[j, t:].sum()), int(d[j].sum()), M - t, int(wait[j]), int(idle[j]))
        score[j] = wrap64(sum(int(w[f]) * x[f] for f in range(7)))
    best = max(score.values())
    winners = [j for j in jobs if score[j] == best]
    if len(winners) > 1:
        trace["ties"] += 1
    if legal[J] and int(w[7]) != NEVER and int(w[7]) > best:
        trace["nopes"] += 1
        return J
    return winners[0]


def mixed_rows(B, seed):
    rng = np.random.default_rng(seed)
    w = rng.integers(-8, 9, size=(B, 8)).astype(np.int32)
    w[rng.random((B, 8)) < 0.3] = 0
    w[:, 7] = np.where(np.arange(B) % 2 == 0, rng.integers(-40, 400, size=B), NEVER)
    w[1] = 0                                     # the all-zero row: every score 0, the lowest legal index
    w[1, 7] = NEVER
    return w


def case_mixed_rows(be, shape, seed=5, max_steps=None):
    """every action of every env, the final makespan and the solution equal the yardstick stepped through OracleEnv.step
    (max_steps, the emulator's runs: the actions of the first max_steps steps only)"""
    env, per_env = make_shape(be, shape)
    B = env.batch
    w = mixed_rows(B, seed)
    env.reset()
    orcs = [OracleEnv(inst, strict=True) for inst in per_env]
    for o in orcs:
        o.reset()
    trace = {"ties": 0, "nopes": 0}
    for step in range(4 * env.jmax * env.mmax):
        if max_steps is not None and step == max_steps:
            return trace
        want = np.array([yardstick(o, inst, w[i], trace) for i, (o, inst) in enumerate(zip(orcs, per_env))], np.int32)
        got = L.host(env.policy("weighted", weights=w))
        assert np.array_equal(got, want), (shape, got, want)
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
        assert ms[i] == o.current_time_step, (shape, i)
        assert np.array_equal(sol[i, :inst.jobs, :inst.machines], o.solution), (shape, i)
    # the same rows played by ONE jss_rule_rollout: the same makespans
    env.reset()
    env.rollout("weighted", n_iter=4 * env.jmax * env.mmax, autoreset=False, weights=w)
    assert np.array_equal(K.host(env, "makespan"), ms), shape
    return trace


# ---- 3. wrap-around ---------------------------------------------------------------------------------------------------------------
def wrap_instance(J=11, M=5):
    base = _inst(J, M)
    return I.Instance("wrap", base.machine.copy(), np.full((J, M), 65535, dtype=np.int32))


def case_wrap(be):
    """weights INT32_MAX / INT32_MIN on durations of 65 535, stepped against the yardstick: large products, every action equal.
    (These sums stay below 2^56; case_wrap_state is the one that crosses 2^63.)"""
    inst = wrap_instance()
    hi, lo = 2**31 - 1, -2**31 + 1
    w = np.array([[hi, hi, hi, hi, hi, hi, hi, NEVER], [lo, lo, lo, lo, lo, lo, lo, NEVER], [hi, lo, hi, lo, hi, hi, hi, 5],
                  [hi, hi, hi, hi, hi, hi, hi, hi], [lo, lo, lo, lo, lo, lo, lo, lo]], dtype=np.int32)
    env = BatchedJssEnv(inst, batch=len(w), _backend=be, seed=2)
    env.reset()
    orcs = [OracleEnv(inst, strict=True) for _ in w]
    for o in orcs:
        o.reset()
    trace = {"ties": 0, "nopes": 0}
    for _ in range(4 * inst.jobs * inst.machines):
        want = np.array([yardstick(o, inst, w[i], trace) for i, o in enumerate(orcs)], np.int32)
        got = L.host(env.policy("weighted", weights=w))
        assert np.array_equal(got, want), (got, want)
        if (want < 0).all():
            return
        env.step(want)
        for o, a in zip(orcs, want):
            if a >= 0:
                o.step(int(a))
    raise AssertionError("episodes did not finish")


# words (idle, idle_last) and the mask of the ops-done count in word 0 of a job record, by ints per record (include/jss_hip.h)
_RECORD = {_abi.NFC: (_abi.FC_IDLE, _abi.FC_IDLE_LAST, _abi.FC_TODO_MASK), _abi.NFM: (_abi.FM_IDLE, _abi.FM_IDLE_LAST, _abi.FM_TODO_MASK),
           _abi.NF: (_abi.F_IDLE, _abi.F_IDLE_LAST, _abi.TODO_MASK)}
WRAP_ROWS = np.array([[2**31 - 1, 0, 0, 0, 0, 2**31 - 1, 2**31 - 1, NEVER],          # 2 (2^31 - 1)^2 + dur 2^31 > 2^63
                      [-2**31, 0, 0, 0, 0, -2**31, -2**31, NEVER],                    # ... and below -2^63
                      [2**31 - 1, 2**31 - 1, 2**31 - 1, 2**31 - 1, 2**31 - 1, 2**31 - 1, 2**31 - 1, 2**31 - 1],
                      [-2**31, 7, -2**31, 0, 3, -2**31, -2**31, -2**31 + 1],
                      [2**31 - 1, 0, 0, 0, 0, 2**31 - 1, -2**31, 0]], dtype=np.int32)


def case_wrap_state(be, shape, seed=8):
    """Sums that cross 2^63.  A few rule steps into an episode the idle and idle_last words of every job record are overwritten,
    in the state tensor, with values within 40 of INT32_MAX; with INT32_MAX / INT32_MIN weights on DUR, WAIT and IDLE the sum
    2 (2^31 - 1)^2 + (dur - 40 .. dur) 2^31 leaves int64 for some jobs of an env and not for others.  jss_rule_policy must equal the yardstick of include/jss_rules.h computed in Python
    ints from the same fields, reduced mod 2^64 and read as signed; asserted here: unreduced sums left [-2^63, 2^63) and the
    reduction changed which job wins for at least one env.  Returns the actions (the backends are compared with each other)."""
    env, per_env = make_shape(be, shape)
    B = env.batch
    rng = np.random.default_rng(seed)
    env.reset()
    env.rollout("SPT", n_iter=6, autoreset=False)
    js = K.host(env, "job_state").copy()
    f_idle, f_last, todo_mask = _RECORD[js.shape[2]]
    js[:, :, f_idle] = 2**31 - 1 - rng.integers(0, 40, size=js.shape[:2])
    js[:, :, f_last] = 2**31 - 1 - rng.integers(0, 40, size=js.shape[:2])
    be.copy_into(env.job_state, js)
    w = WRAP_ROWS[np.arange(B) % len(WRAP_ROWS)]
    mask = K.host(env, "action_mask")
    want, crossed, changed = [], 0, 0
    for i, inst in enumerate(per_env):
        J, M, d = inst.jobs, inst.machines, inst.duration
        jobs = [j for j in range(J) if mask[i, j]]
        assert jobs, (shape, i)
        raw = {}
        for j in jobs:
            t = int(js[i, j, 0] & todo_mask)
            x = (int(d[j, t]), int(d[j, t + 1]) if t + 1 < M else 0, int(d[j, t:].sum()), int(d[j].sum()), M - t,
                 int(js[i, j, f_last]), int(js[i, j, f_idle]))
            raw[j] = sum(int(w[i, f]) * x[f] for f in range(7))
        crossed += sum(1 for v in raw.values() if not -2**63 <= v < 2**63)
        score = {j: wrap64(v) for j, v in raw.items()}
        best = max(score.values())
        a = min(j for j in jobs if score[j] == best)
        changed += a != min(j for j in jobs if raw[j] == max(raw.values()))
        if mask[i, J] and int(w[i, 7]) != NEVER and int(w[i, 7]) > best:
            a = J
        want.append(a)
    assert crossed >= 1 and changed >= 1, (shape, crossed, changed)
    got = L.host(env.policy("weighted", weights=w))
    assert np.array_equal(got, np.array(want, np.int32)), (shape, got, want)
    return got


# ---- 4. lookahead -------------------------------------------------------------------------------------------------------------------
def case_lookahead(be, shape="p16-J11", per_parent=None, seed=4, n_iter=None, explores=(0.0, 0.4)):
    """jss_rule_lookahead == fork + step + jss_rule_rollout with the parents' rows, bit for bit (makespan, steps, reward
    numerators): shared row and per-parent rows, candidates parent-major and shuffled, a done parent and illegal actions
    (-1 / 0 / 0) among them; pilot_step(weights=...) takes the arg-min action."""
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
    rows = mixed_rows(B, seed + 1)
    n_iter = 3 * env.jmax * env.mmax if n_iter is None else n_iter        # (short: candidates that do not finish score -1)
    for w in (rows, rows[2]):
        for order in (np.arange(len(par)), rng.permutation(len(par))):
            p, a, ok = par[order], act[order], legal[order]
            for explore in explores:
                ms, st, ret = env.lookahead("weighted", actions=a, parents=p, seed=9, explore=explore, id_base=100, weights=w,
                                            n_iter=n_iter)
                f = env.fork(p, env_id_base=100)
                f.zero_counters()
                f.step(np.where(ok, a, -1).astype(np.int32))
                f.rollout("weighted", n_iter=n_iter, seed=9, explore=explore, autoreset=False, weights=w if w.ndim == 1 else w[p])
                done, fms, cn = K.host(f, "done"), K.host(f, "makespan"), K.host(f, "counters")
                assert np.array_equal(L.host(ms), np.where(ok & (done != 0), fms, -1)), shape
                assert np.array_equal(L.host(st), np.where(ok, cn[:, 0], 0)), shape
                mto = K.host(env, "env_const")[p, _abi.C_MAX_TIME_OP].astype(np.float64)
                want_ret = np.where(ok, cn[:, 3] / mto, 0.0).astype(np.float32)
                assert np.array_equal(L.host(ret), want_ret), shape
                assert (L.host(ms)[~ok] == -1).all() and (L.host(st)[~ok] == 0).all()
    same(before, snapshot(env), "lookahead wrote into the batch")
    # pilot_step: the arg-min of the scores, -1 = +inf, lowest index on ties; a done env is left alone
    if n_iter != 3 * env.jmax * env.mmax:
        return
    scores = L.host(env.lookahead("weighted", weights=rows)[0])
    _, _, _, _, info = env.pilot_step("weighted", weights=rows)
    free = scores < 0
    want = np.where(free.all(axis=1), -1, np.where(free, 2**31 - 1, scores).argmin(axis=1))
    assert np.array_equal(L.host(info["action"]), want) and np.array_equal(L.host(info["scores"]), scores)
    assert want[B - 1] == -1


# ---- 5. the boundary -----------------------------------------------------------------------------------------------------------------
def argument_rows():
    """(name, call, expected code, build(world) -> args): the argument errors of the three jss_rule_* calls"""
    def parts(w, d=None, rule=None, null=()):
        desc = _abi.JssDesc(batch=2, jmax=4, mmax=3, n_tables=1, ops=w.p(), rem=w.p(), inst=w.p())
        for k, v in (d or {}).items():
            setattr(desc, k, v)
        st = _abi.JssState(*(w.p() for _ in range(6)))
        out = _abi.JssOut(*(w.p() for _ in range(5)))
        r = _abi.JssRule(w.p(), 8)
        for k, v in (rule or {}).items():
            setattr(r, k, v)
        look = _abi.JssLookahead(n=3, parent=w.p(), action=w.p(), id_base=0, makespan=w.p(), steps=w.p(), reward_num=w.p())
        return desc, st, out, (None if "rule" in null else C.byref(r)), look, w.p()

    def policy(w, **kw):
        d, s, _, r, _, acts = parts(w, **kw)
        return C.byref(d), C.byref(s), r, 0, 0, (None if kw.get("null") == ("actions",) else acts), None

    def rollout(w, n_iter=5, **kw):
        d, s, o, r, _, _ = parts(w, **kw)
        return C.byref(d), C.byref(s), C.byref(o), r, 0, 0, n_iter, 0, None

    def lookahead(w, n_iter=5, **kw):
        d, s, _, r, la, _ = parts(w, **kw)
        return C.byref(d), C.byref(s), C.byref(la), r, 0, 0, n_iter, None

    R = []
    for call, build in (("jss_rule_policy", policy), ("jss_rule_rollout", rollout), ("jss_rule_lookahead", lookahead)):
        R.append((f"{call}-null-rule", call, _abi.E_NULL, lambda w, b=build: b(w, null=("rule",))))
        R.append((f"{call}-null-weights", call, _abi.E_NULL, lambda w, b=build: b(w, rule={"weights": None})))
        R.append((f"{call}-no-rem", call, _abi.E_NULL, lambda w, b=build: b(w, d={"rem": None})))
        R.append((f"{call}-stride-4", call, _abi.E_SHAPE, lambda w, b=build: b(w, rule={"stride": 4})))
        R.append((f"{call}-weights-misaligned", call, _abi.E_SHAPE, lambda w, b=build: b(w, rule={"weights": w.p() + 4})))
        R.append((f"{call}-stride-negative", call, _abi.E_SHAPE, lambda w, b=build: b(w, rule={"stride": -8})))
        # the namesake's own checks come first, as with `kind`
        R.append((f"{call}-shape-before-rule", call, _abi.E_SHAPE, lambda w, b=build: b(w, d={"jmax": 0}, null=("rule",))))
    R.append(("jss_rule_policy-null-actions", "jss_rule_policy", _abi.E_NULL, lambda w: policy(w, null=("actions",))))
    R.append(("jss_rule_rollout-rule-before-n-iter", "jss_rule_rollout", _abi.E_NULL, lambda w: rollout(w, n_iter=-1, null=("rule",))))
    R.append(("jss_rule_rollout-n-iter-negative", "jss_rule_rollout", _abi.E_SHAPE, lambda w: rollout(w, n_iter=-1)))
    R.append(("jss_rule_lookahead-n-iter-before-rule", "jss_rule_lookahead", _abi.E_SHAPE, lambda w: lookahead(w, n_iter=-1, null=("rule",))))
    return R


def run_argument_row(lib, call, build):
    w = L._World()
    args = build(w)
    before = [b.copy() for b in w.bufs]
    rc = getattr(lib, call)(*args)
    changed = [i for i, (a, b) in enumerate(zip(before, w.bufs)) if not np.array_equal(a, b)]
    return rc, changed


def kind8_rows():
    """kind 8 -- the launcher's own code of the weighted selector -- through the stock calls: still JSS_E_KIND"""
    def desc(w):
        return _abi.JssDesc(batch=2, jmax=4, mmax=3, n_tables=1, ops=w.p(), rem=w.p(), inst=w.p())

    def policy(w):
        return "jss_policy", (C.byref(desc(w)), C.byref(_abi.JssState(*(w.p() for _ in range(6)))), 8, 0, 0, w.p(), None)

    def rollout(w):
        return "jss_rollout", (C.byref(desc(w)), C.byref(_abi.JssState(*(w.p() for _ in range(6)))),
                               C.byref(_abi.JssOut(*(w.p() for _ in range(5)))), 8, 0, 0, 5, 0, None)

    def lookahead(w):
        la = _abi.JssLookahead(n=3, parent=w.p(), action=w.p(), id_base=0, makespan=w.p(), steps=w.p(), reward_num=w.p())
        return "jss_lookahead", (C.byref(desc(w)), C.byref(_abi.JssState(*(w.p() for _ in range(6)))), C.byref(la), 8, 0, 0, 5, None)
    return policy, rollout, lookahead


# ---- 6. the host mirror ----------------------------------------------------------------------------------------------------------------
def case_mirror(be, seed=5):
    """WeightedRule.__call__ on the B = 1 facade agrees with jss_rule_policy on every step of one mixed-row episode"""
    from jssenv_amd import make
    from jssenv_amd.dispatching import WeightedRule
    row = np.array([-3, 2, 1, 0, 5, 4, -1, 60], dtype=np.int32)
    env = make("jss-v1", env_config={"instance_path": "ta01"}, _backend=be)
    rule = WeightedRule(row)
    env.reset()
    done, steps = False, 0
    while not done:
        a = rule(env)
        # (the facade's buffers may be pinned host memory the kernel writes in place: the backend's copy waits for it)
        assert a == int(be.numpy(env._b.policy("weighted", weights=row))[0]), steps
        _, _, done, _, _ = env.step(a)
        steps += 1
    assert steps >= 225
