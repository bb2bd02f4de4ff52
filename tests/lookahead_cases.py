"""Backend-agnostic cases of jss_lookahead / BatchedJssEnv.lookahead / pilot_step (candidate moves scored by rule rollouts
without clones), run against the host-core twin, the kernel source under the SIMT emulator and the HIP library.

The yardstick of a candidate is its definition in include/jss_search.h: what fork([parent], env_id_base = id_base + k),
step(action) and rollout(kind, n_iter, autoreset=False) give -- the fork's makespan output and its counters' steps and reward
numerators.  The oracle finishing an action with a rule is the yardstick with no fork involved."""
import ctypes as C

import numpy as np

import clone_cases as K
from jssenv_amd import BatchedJssEnv, _abi
from jssenv_amd import instances as I
from oracle import OracleEnv

KINDS = (("random", 0.0), ("SPT", 0.3), ("FIFO", 0.0), ("SPT", 0.0), ("MWR", 0.0), ("LWR", 0.0), ("MOR", 0.0), ("LOR", 0.0),
         ("CR", 0.0))


def host(x):
    return np.array(x.detach().cpu().numpy() if hasattr(x, "detach") else x, copy=True)


def snapshot(env):
    """every tensor of the batch a call could write: state, outputs, counters (the header is in env_header)"""
    out = K.rows_of(env)
    out["counters"] = K.host(env, "counters")
    return out


def candidates(env, rng, per_parent=None):
    """(parents, actions, legal): for every env SKIP, every job and NOPE column of its row, one padded column and two actions
    out of range; `per_parent` keeps a random subset of that many per env (emulator runs).  legal = the candidate has
    something to evaluate: the parent is not done and the action is SKIP or set in its mask."""
    mask, done = K.host(env, "action_mask"), K.host(env, "done")
    par, act, ok = [], [], []
    for i in range(env.batch):
        J = int(env.jobs_per_env[i])
        acts = [-1] + list(range(J + 1)) + [env.jmax + 1, -2, -7]
        if per_parent is not None:
            acts = list(rng.choice(acts, size=min(per_parent, len(acts)), replace=False))
        for a in acts:
            par.append(i)
            act.append(int(a))
            ok.append(not done[i] and (a == -1 or (0 <= a <= J and bool(mask[i, a]))))
    return np.array(par, np.int32), np.array(act, np.int32), np.array(ok)


def by_fork(env, parents, actions, legal, kind, seed, explore, n_iter, id_base):
    """the definition: fork every candidate (env_id_base = id_base -> fork env k has id id_base + k), step, rollout"""
    f = env.fork(parents, env_id_base=id_base)
    f.step(np.where(legal, actions, -1).astype(np.int32))
    f.rollout(kind, n_iter=n_iter, seed=seed, explore=explore, autoreset=False)
    done, ms, cn = K.host(f, "done"), K.host(f, "makespan"), K.host(f, "counters")
    makespan = np.where(legal & (done != 0), ms, -1).astype(np.int32)
    steps = np.where(legal, cn[:, 0], 0).astype(np.int32)
    reward_num = np.where(legal, cn[:, 3], 0).astype(np.int64)
    return makespan, steps, reward_num


def raw_lookahead(be, env, parents, actions, kind, seed=0, explore=0.0, n_iter=None, id_base=0):
    """jss_lookahead through the C ABI (reward numerators unscaled); returns (makespan, steps, reward_num) host arrays"""
    _abi.bind_search(be.lib)
    n = len(parents)
    n_iter = 3 * env.jmax * env.mmax if n_iter is None else n_iter
    with be.on_device():
        par, act = be.from_numpy(np.asarray(parents, np.int32)), be.from_numpy(np.asarray(actions, np.int32))
        ms, st, rn = be.zeros((n,), "int32"), be.zeros((n,), "int32"), be.zeros((n,), "int64")
        p = be.ptr
        la = _abi.JssLookahead(n, p(par), p(act), id_base, p(ms), p(st), p(rn))
        rc = be.lib.jss_lookahead(C.byref(env._desc), C.byref(env._state), C.byref(la), _abi.policy_code(kind), seed,
                                  int(round(explore * 65536)), n_iter, be.stream())
        be.sync()
    assert rc == 0, rc
    return host(ms), host(st), host(rn)


# ---- cases -------------------------------------------------------------------------------------------------------------
def case_equivalence(be, layout, kinds=KINDS, B=8, n_steps=50, seed=2, per_parent=None, by_shape=K.BY_SHAPE_SMALL):
    """every candidate's makespan, steps and reward numerators equal the fork + step + rollout counters bit for bit, for
    every kind; the batch is byte-equal before and after; nothing-to-evaluate candidates give -1 / 0 / 0.  Returns the
    results per kind."""
    rng = np.random.default_rng(seed)
    env = K.make_layout(be, layout, B, by_shape=by_shape)
    env.reset()
    env.rollout("random", n_iter=3 * env.jmax * env.mmax, autoreset=False, seed=seed)   # every env done ...
    env.reset(np.arange(B) % 3 != 0)                                    # ... every third stays done
    K.drive(env, rng, n_steps)
    assert K.host(env, "done")[::3].all() and not K.host(env, "done")[1::3].all()
    parents, actions, legal = candidates(env, rng, per_parent)
    out = {}
    for kind, explore in kinds:
        before = snapshot(env)
        ms, st, ret = env.lookahead(kind, actions=actions, parents=parents, seed=17, explore=explore, id_base=40)
        be.sync()
        after = snapshot(env)
        for name, v in before.items():
            assert np.array_equal(after[name], v), (kind, name)
        ms, st, ret = host(ms), host(st), host(ret)
        _, _, rn = raw_lookahead(be, env, parents, actions, kind, seed=17, explore=explore, id_base=40)
        want = by_fork(env, parents, actions, legal, kind, 17, explore, 3 * env.jmax * env.mmax, 40)
        assert np.array_equal(ms, want[0]), (kind, np.flatnonzero(ms != want[0])[:8])
        assert np.array_equal(st, want[1]), kind
        assert np.array_equal(rn, want[2]), kind
        assert (ms[legal] > 0).all() and (ms[~legal] == -1).all() and (st[~legal] == 0).all() and (rn[~legal] == 0).all()
        mto = K.host(env, "env_const")[parents, _abi.C_MAX_TIME_OP].astype(np.float64)
        assert np.array_equal(ret, np.where(mto > 0, rn / np.maximum(mto, 1), 0).astype(np.float32))
        out[(kind, explore)] = (ms, st, rn)
    return out


def case_every_action(be, layout="compact", B=4, seed=3):
    """parents = actions = None: a (B, jmax + 1) table, parent-major, equal to the explicit form; padded and illegal columns -1"""
    env = K.make_layout(be, layout, B)
    env.reset()
    K.drive(env, np.random.default_rng(seed), 20)
    ms, st, ret = env.lookahead("SPT")
    ms, st = host(ms), host(st)
    assert ms.shape == (B, env.jmax + 1)
    par = np.repeat(np.arange(B), env.jmax + 1).astype(np.int32)
    act = np.tile(np.arange(env.jmax + 1), B).astype(np.int32)
    m2, s2, _ = env.lookahead("SPT", actions=act, parents=par)
    assert np.array_equal(ms.ravel(), host(m2)) and np.array_equal(st.ravel(), host(s2))
    mask, done = K.host(env, "action_mask"), K.host(env, "done")
    for i in range(B):
        J = int(env.jobs_per_env[i])
        ok = mask[i].astype(bool) & (np.arange(env.jmax + 1) <= J) & (not done[i])
        assert ((ms[i] > 0) == ok).all(), i
    return ms


def case_nothing_to_evaluate(be, layout="full", B=6):
    """-1 / 0 / 0: illegal jobs, NOPE when it is not legal, actions and parents out of range, done parents, a parent that was
    never reset; an n_iter too small to finish gives -1 with the fork's counters"""
    rng = np.random.default_rng(4)
    env = K.make_layout(be, layout, B)
    env.reset()
    env.rollout("random", n_iter=3 * env.jmax * env.mmax, autoreset=False, seed=3)   # every env done
    env.reset(np.arange(B) % 2 == 0)                                    # ... but the even ones start over
    K.drive(env, rng, 6)
    mask, done = K.host(env, "action_mask"), K.host(env, "done")
    assert done[1] and not done[0]
    J0 = int(env.jobs_per_env[0])
    illegal = [a for a in range(J0) if not mask[0, a]]
    assert illegal
    par = [0] * (len(illegal) + 6) + [1, 1, -1, B, 1 << 30]
    act = illegal + [J0 + 1, env.jmax + 5, -2, -3, -1000, 1 << 30] + [0, -1, 0, 0, -1]
    if not mask[0, J0]:
        par.append(0)
        act.append(J0)
    ms, st, rn = raw_lookahead(be, env, par, act, "SPT", seed=1)
    assert (ms == -1).all() and (st == 0).all() and (rn == 0).all(), (ms, st, rn)
    # a parent that was never reset
    fresh = K.make_layout(be, layout, 2)
    fresh.reset(np.array([1, 0], np.uint8))
    ms, st, rn = raw_lookahead(be, fresh, [1, 1], [-1, 0], "SPT")
    assert (ms == -1).all() and (st == 0).all() and (rn == 0).all()
    # n_iter too small: -1, steps / reward numerators as the fork's counters
    legal = np.flatnonzero(mask[0, :J0 + 1])
    par, act = np.zeros(legal.size + 1, np.int32), np.concatenate([legal, [-1]]).astype(np.int32)
    for kind in ("SPT", "random"):
        ms, st, rn = raw_lookahead(be, env, par, act, kind, seed=5, n_iter=4, id_base=9)
        want = by_fork(env, par, act, np.ones(par.size, bool), kind, 5, 0.0, 4, 9)
        assert (ms == -1).all() and (want[0] == -1).all()
        assert np.array_equal(st, want[1]) and np.array_equal(rn, want[2]), kind
        assert (st[:-1] == 5).all() and (st[-1] == 4).all()


def spt_oracle(inst, prefix_actions, first):
    orc = OracleEnv(inst, strict=True)
    orc.reset()
    for a in prefix_actions:
        orc.step(a)
    orc.step(first)
    while orc.legal_actions.any():
        orc.step(orc.policy("SPT"))
    return orc.current_time_step


def case_oracle(be, prefix=30):
    """ta01 after `prefix` SPT steps: every candidate's makespan equals the oracle finishing that action with SPT"""
    env = BatchedJssEnv("ta01", batch=1, _backend=be, seed=0)
    env.reset()
    env.rollout("SPT", n_iter=prefix, autoreset=False)
    ms = host(env.lookahead("SPT")[0])[0]
    inst = I.resolve_instance("ta01")
    orc = OracleEnv(inst, strict=True)
    orc.reset()
    hist = []
    for _ in range(prefix):
        a = orc.policy("SPT")
        hist.append(a)
        orc.step(a)
    legal = np.flatnonzero(orc.legal_actions)
    assert np.array_equal(np.flatnonzero(ms >= 0), legal)
    for a in legal:
        assert int(ms[a]) == spt_oracle(inst, hist, int(a)), a
    return ms


def pilot_oracle(inst):
    """the pilot method on the oracle: every legal action finished with SPT (the history replayed from reset), the lowest
    makespan taken (lowest index on ties)"""
    orc = OracleEnv(inst, strict=True)
    orc.reset()
    actions = []
    while orc.legal_actions.any():
        scores = [(spt_oracle(inst, actions, int(a)), int(a)) for a in np.flatnonzero(orc.legal_actions)]
        best = min(scores)[1]
        actions.append(best)
        orc.step(best)
    return actions, orc.current_time_step


def case_pilot_small(be, seed=6):
    """a whole pilot-SPT episode on a 6 x 6 synthetic instance, action for action the oracle's pilot loop"""
    env = BatchedJssEnv(I.synthetic_packed(1, 6, 6, first=seed), batch=1, _backend=be, seed=0)
    env.reset()
    want, makespan = pilot_oracle(env.instance(0))
    got = []
    for _ in range(200):
        _, _, done, _, info = env.pilot_step("SPT")
        got.append(int(host(info["action"])[0]))
        if host(done)[0]:
            break
    assert got == want, (got, want)
    assert int(K.host(env, "makespan")[0]) == makespan
    # done: the next pilot step leaves the env alone (or resets it)
    _, _, _, _, info = env.pilot_step("SPT")
    assert int(host(info["action"])[0]) == _abi.ACTION_SKIP and (host(info["scores"]) == -1).all()
    _, _, done, _, info = env.pilot_step("SPT", autoreset=True)
    assert int(host(info["action"])[0]) == _abi.ACTION_RESET and not host(done)[0]
    return got


def case_pilot_ta01(be, batch=1):
    """pilot-SPT on ta01 finishes no later than SPT itself (the rule's own continuation stays a candidate); returns makespans"""
    env = BatchedJssEnv("ta01", batch=batch, _backend=be, seed=0)
    env.reset()
    spt = env.fork(np.arange(batch))
    spt.rollout("SPT", n_iter=3 * 15 * 15, autoreset=False)
    for _ in range(3 * 15 * 15):
        _, _, done, _, _ = env.pilot_step("SPT")
        if host(done).all():
            break
    pilot, base = K.host(env, "makespan"), K.host(spt, "makespan")
    assert K.host(env, "done").all() and (pilot <= base).all(), (pilot, base)
    return pilot, base


class _World:
    """host buffers of random bytes, one per pointer, so that any write shows (tests/test_abi_arguments.py's manner)"""

    def __init__(self):
        self.bufs = []
        self.rng = np.random.default_rng(1)

    def p(self):
        b = self.rng.integers(0, 256, size=1 << 16, dtype=np.uint8)
        self.bufs.append(b)
        return b.ctypes.data


def argument_rows():
    """(name, expected code, build(world) -> args of jss_lookahead)"""
    def call(w, d=None, s=None, la=None, kind=_abi.POLICY["SPT"], n_iter=10, null=()):
        desc = _abi.JssDesc(batch=2, jmax=4, mmax=3, n_tables=1, ops=w.p(), rem=w.p(), inst=w.p())
        for k, v in (d or {}).items():
            setattr(desc, k, v)
        st = _abi.JssState(*(w.p() for _ in range(6)))
        for k, v in (s or {}).items():
            setattr(st, k, v)
        look = _abi.JssLookahead(n=3, parent=w.p(), action=w.p(), id_base=0, makespan=w.p(), steps=w.p(), reward_num=w.p())
        for k, v in (la or {}).items():
            setattr(look, k, v)
        return (None if "desc" in null else C.byref(desc), None if "state" in null else C.byref(st),
                None if "la" in null else C.byref(look), kind, 0, 0, n_iter, None)
    R = []
    row = lambda name, code, build: R.append((name, code, build))   # noqa: E731
    row("ok-n0", 0, lambda w: call(w, la={"n": 0}))
    for what in ("desc", "state", "la"):
        row(f"null-{what}", _abi.E_NULL, lambda w, what=what: call(w, null=(what,)))
    for f in ("parent", "action", "makespan"):
        row(f"null-{f}", _abi.E_NULL, lambda w, f=f: call(w, la={f: None}))
    row("null-ops", _abi.E_NULL, lambda w: call(w, d={"ops": None}))
    row("null-job", _abi.E_NULL, lambda w: call(w, s={"job": None}))
    row("null-machine-full", _abi.E_NULL, lambda w: call(w, s={"machine": None}))
    row("n-negative", _abi.E_SHAPE, lambda w: call(w, la={"n": -1}))
    row("n-iter-negative", _abi.E_SHAPE, lambda w: call(w, n_iter=-1))
    row("batch-negative", _abi.E_SHAPE, lambda w: call(w, d={"batch": -1}))
    row("jmax-zero", _abi.E_SHAPE, lambda w: call(w, d={"jmax": 0}))
    row("mmax-too-wide", _abi.E_SHAPE, lambda w: call(w, d={"mmax": 65}))
    row("compact-n-tables", _abi.E_SHAPE, lambda w: call(w, d={"record_ints": _abi.NFC, "n_tables": 2}))
    row("kind-unknown", _abi.E_KIND, lambda w: call(w, kind=99))
    row("kind-cr-f64", _abi.E_KIND, lambda w: call(w, kind=_abi.POLICY_CR_F64, d={"cr_factor": 1.5}))
    row("kind-cr-factor-bad-q", _abi.E_KIND, lambda w: call(w, kind=_abi.POLICY["CR"] | (3 << 8) | (3 << 16)))
    row("kernel-bad", _abi.E_KIND, lambda w: call(w, d={"kernel": 8}))
    row("mwr-no-rem", _abi.E_NULL, lambda w: call(w, d={"rem": None}, kind=_abi.POLICY["MWR"]))
    return R


def run_argument_row(lib, build):
    w = _World()
    args = build(w)
    before = [b.copy() for b in w.bufs]
    rc = lib.jss_lookahead(*args)
    changed = [i for i, (a, b) in enumerate(zip(before, w.bufs)) if not np.array_equal(a, b)]
    return rc, changed
