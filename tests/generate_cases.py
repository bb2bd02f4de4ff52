"""Backend-agnostic cases of jss_generate / BatchedJssEnv.generated (Taillard instances drawn on the device into the envs' own
tables), run against the host-core twin, the kernel source under the SIMT emulator and the HIP library.

The host generator (jssenv_amd.instances.synthetic_arrays / taillard_instance) is the reference for the draws; the NumPy
mirror below restates the header's derived-seed function: 1 + rng_u32(seed ^ K_GEN, env_id, episode, 0 | 1) % (2^31 - 2)."""
import ctypes as C

import numpy as np

import logits_cases as L
from jssenv_amd import BatchedJssEnv, _abi
from jssenv_amd import instances as I

M32 = 0xFFFFFFFF
STATE = ("env_header", "env_const", "job_state", "real_obs", "action_mask", "reward", "done", "makespan", "counters", "solution")


# ---- the documented seed function, in NumPy ------------------------------------------------------------------------
def derived_seeds(seed, env_ids, episode):
    """(time_seeds, machine_seeds) of the envs `env_ids` for the episode number `episode` (the one their next reset gives
    them: the header's episode + 1)"""
    key = (int(seed) ^ _abi.GEN_SEED_XOR) & ((1 << 64) - 1)
    ep = np.asarray(episode, dtype=np.int64) & M32
    ts = 1 + L.rng_u32(key, env_ids, ep, 0).astype(np.int64) % _abi.GEN_SEED_MOD
    ms = 1 + L.rng_u32(key, env_ids, ep, 1).astype(np.int64) % _abi.GEN_SEED_MOD
    return ts, ms


def mirror_instance(seed, env_id, episode, jobs, machines, durations=(1, 99)):
    ts, ms = derived_seeds(seed, [env_id], [episode])
    machine, duration = I.synthetic_arrays(1, jobs, machines, durations=durations, seeds=(ts, ms))
    return machine[0], duration[0]


# ---- the raw call ------------------------------------------------------------------------------------------------------
def raw_generate(be, n, J, M, jmax=None, mmax=None, durations=(1, 99), seeds=None, which=None, episodes=None, env_ids=None,
                 env_id_base=0, seed=0, actions=None, fill=7, tables=None):
    """jss_generate on tables pre-filled with `fill` (or the given (ops, rem, inst) host arrays); returns (rc, ops, rem, inst)
    as host arrays after the call"""
    jmax, mmax = jmax or J, mmax or M
    if tables is None:
        tables = (np.full((n, jmax, mmax), fill, np.int32), np.full((n, jmax, mmax), fill, np.int32),
                  np.full((n, _abi.NI), fill, np.int32))
    up = lambda a, dt: None if a is None else be.from_numpy(np.ascontiguousarray(a, dtype=dt))   # noqa: E731
    with be.on_device():
        ops, rem, inst = (up(t, np.int32) for t in tables)
        hdr = np.zeros((n, _abi.NH), np.int32)
        if episodes is not None:
            hdr[:, _abi.H_EPISODE] = episodes
        hdr = up(hdr, np.int32)
        ts, ms = (None, None) if seeds is None else (up(seeds[0], np.int64), up(seeds[1], np.int64))
        w, a, ids = up(which, np.uint8), up(actions, np.int32), up(env_ids, np.int64)
        p = be.ptr
        d = _abi.JssDesc(n, jmax, mmax, n, p(ops), p(rem), p(inst), None, p(ids), env_id_base)
        s = _abi.JssState(p(hdr), None, None, None, None, None)
        g = _abi.JssGen(p(ops), p(rem), p(inst), p(ts), p(ms), p(a), seed & ((1 << 64) - 1), J, M, *durations)
        rc = be.lib.jss_generate(C.byref(d), C.byref(s), C.byref(g), p(w), be.stream())
        be.sync()
        return rc, be.numpy(ops), be.numpy(rem), be.numpy(inst)


def expected_tables(n, J, M, jmax, mmax, durations, seeds):
    pk = I.synthetic_packed(n, J, M, durations=durations, seeds=seeds)
    ops, rem = np.zeros((n, jmax, mmax), np.int32), np.zeros((n, jmax, mmax), np.int32)
    ops[:, :J, :M], rem[:, :J, :M] = pk.ops, pk.rem
    return ops, rem, pk.inst


# ---- cases ---------------------------------------------------------------------------------------------------------------
def case_matches_host_generator(be, n, J, M, durations=(1, 99), pad=(0, 0)):
    """explicit seeds 1 + 2i / 2 + 2i give synthetic_packed(n, J, M) bit for bit; padding rows / columns written as zeros"""
    jmax, mmax = J + pad[0], M + pad[1]
    idx = np.arange(n, dtype=np.int64)
    rc, ops, rem, inst = raw_generate(be, n, J, M, jmax, mmax, durations, seeds=(1 + 2 * idx, 2 + 2 * idx))
    assert rc == 0
    eo, er, ei = expected_tables(n, J, M, jmax, mmax, durations, None)
    assert np.array_equal(ops, eo) and np.array_equal(rem, er) and np.array_equal(inst, ei)
    return inst


def case_published_ta01(be):
    rc, ops, rem, inst = raw_generate(be, 2, 15, 15, seeds=([840612802, 840612802], [398197754, 398197754]))
    assert rc == 0
    ta01 = I.builtin_instance("ta01")
    for i in range(2):
        assert np.array_equal(ops[i], ta01.packed())
        assert np.array_equal(inst[i], I.instance_record(ta01))
    assert np.array_equal(ops[0], I.taillard_instance(15, 15, 840612802, 398197754).packed())


def case_derived_seeds(be, n=40, J=6, M=5, seed=0x1234_5678_9ABC_DEF0):
    """derived seeds = the mirror of the header's function of (seed, global env id, header episode + 1), with explicit
    env ids, env_id_base and episodes that wrap"""
    rng = np.random.default_rng(3)
    eps = rng.integers(-5, 1 << 20, n).astype(np.int32)
    eps[:3] = (2**31 - 1, -1, 0)
    for ids, base in ((None, 0), (None, 1 << 40), (rng.integers(0, 1 << 62, n).astype(np.int64), 0)):
        rc, ops, rem, inst = raw_generate(be, n, J, M, episodes=eps, env_ids=ids, env_id_base=base, seed=seed)
        assert rc == 0
        gid = ids if ids is not None else base + np.arange(n, dtype=np.int64)
        eo, er, ei = expected_tables(n, J, M, J, M, (1, 99), derived_seeds(seed, gid.astype(np.uint64), eps.astype(np.int64) + 1))
        assert np.array_equal(ops, eo) and np.array_equal(rem, er) and np.array_equal(inst, ei)


def case_sharding(be, n=48, J=7, M=4, seed=5):
    """a batch generated as two shards (env_id_base 0 and n / 2) equals the batch generated at once"""
    eps = np.arange(n, dtype=np.int32) % 7
    whole = raw_generate(be, n, J, M, episodes=eps, seed=seed)
    h = n // 2
    lo = raw_generate(be, h, J, M, episodes=eps[:h], seed=seed, env_id_base=0)
    hi = raw_generate(be, n - h, J, M, episodes=eps[h:], seed=seed, env_id_base=h)
    for k in (1, 2, 3):
        assert np.array_equal(whole[k], np.concatenate([lo[k], hi[k]]))


def case_which_and_padding(be, n=150, J=9, M=6, pad=(3, 2)):
    """only flagged envs (which[i] != 0, or actions[i] == -2) are written; every byte of the others, padding included, is
    untouched; the flagged ones' padding is zero.  Out-of-range explicit seeds leave the env untouched."""
    rng = np.random.default_rng(8)
    jmax, mmax = J + pad[0], M + pad[1]
    tables = tuple(rng.integers(-2**31, 2**31 - 1, shape, dtype=np.int64).astype(np.int32)
                   for shape in ((n, jmax, mmax), (n, jmax, mmax), (n, _abi.NI)))
    which = (rng.random(n) < 0.1).astype(np.uint8)
    actions = rng.integers(-3, 4, n).astype(np.int32)
    idx = np.arange(n, dtype=np.int64)
    ts, ms = 1 + 2 * idx, 2 + 2 * idx
    ts[5], ms[6], ts[7] = 0, _abi.LCG_M, -3                 # outside [1, 2^31 - 2]: those envs are not written
    which[5:8] = 1
    eo, er, ei = expected_tables(n, J, M, jmax, mmax, (1, 99), (np.where(ts < 1, 1, np.minimum(ts, _abi.LCG_M - 1)),
                                                             np.minimum(ms, _abi.LCG_M - 1)))
    for w, a in ((which, None), (None, actions), (which, actions)):
        flagged = np.zeros(n, bool)
        if w is not None:
            flagged |= w != 0
        if a is not None:
            flagged |= a == _abi.ACTION_RESET
        written = flagged.copy()
        written[5:8] = False
        rc, ops, rem, inst = raw_generate(be, n, J, M, jmax, mmax, seeds=(ts, ms), which=w, actions=a, tables=tables)
        assert rc == 0
        for got, exp, old in ((ops, eo, tables[0]), (rem, er, tables[1]), (inst, ei, tables[2])):
            assert np.array_equal(got[written], exp[written])
            assert np.array_equal(got[~written], old[~written])
        assert not ops[written][:, J:].any() and not ops[written][:, :, M:].any() and not rem[written][:, J:].any()
        assert written.sum() > 3


def case_argument_errors(lib):
    """the documented error codes; nothing is launched (valid pointers are never dereferenced on the host side of the HIP
    library)"""
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p).value

    def call(batch=4, jmax=15, mmax=15, n_tables=None, toe=None, J=15, M=15, lo=1, hi=99, ts=None, ms=None, ops=p,
             state=True, env=p, gen=True):
        d = _abi.JssDesc(batch, jmax, mmax, batch if n_tables is None else n_tables, p, p, p, toe, None, 0)
        s = _abi.JssState(env, p, p, p, p, p)
        g = _abi.JssGen(ops, p, p, ts, ms, None, 0, J, M, lo, hi)
        return lib.jss_generate(C.byref(d), C.byref(s) if state else None, C.byref(g) if gen else None, None, None)

    E_SHAPE, E_NULL = _abi.E_SHAPE, _abi.E_NULL
    for kw in ({"J": 0}, {"J": 16}, {"M": 0}, {"M": 16}, {"jmax": 129, "J": 129}, {"mmax": 65, "M": 65}, {"jmax": 0, "J": 0},
               {"mmax": 0, "M": 0}, {"lo": 0}, {"hi": 65536}, {"lo": 50, "hi": 49}, {"n_tables": 1}, {"n_tables": 5},
               {"toe": p}, {"batch": -1, "n_tables": -1}):
        assert call(**kw) == E_SHAPE, kw
    for kw in ({"gen": False}, {"ops": None}, {"ts": p}, {"ms": p}, {"state": False}, {"env": None}):
        assert call(**kw) == E_NULL, kw
    assert lib.jss_generate(None, None, None, None, None) == E_NULL
    assert call(batch=0, n_tables=0) == 0                    # an empty batch launches nothing


def _host(env, name):
    return np.array(env.backend.numpy(getattr(env, name)), copy=True)


def case_same_trajectory_as_host_generator(be, B=24, J=5, M=4, steps=160, seed=9, instance_seed=77, **kw):
    """fresh=False: a generated batch steps exactly like BatchedJssEnv(synthetic_packed(...)) of the same instances"""
    env = BatchedJssEnv.generated(J, M, B, instance_seed=instance_seed, fresh=False, seed=seed, _backend=be, **kw)
    pk = I.synthetic_packed(B, J, M, seeds=derived_seeds(instance_seed, np.arange(B, dtype=np.uint64), np.ones(B, np.int64)))
    ref = BatchedJssEnv(pk, seed=seed, _backend=be, **kw)
    assert (env.record_ints, env.kernel) == (ref.record_ints, ref.kernel)
    assert np.array_equal(env.packed.ops, pk.ops) and np.array_equal(env.packed.inst, pk.inst)
    env.reset(), ref.reset()
    for _ in range(steps):
        env.step(env.policy("random"), autoreset=True)
        ref.step(ref.policy("random"), autoreset=True)
    for name in STATE:
        assert np.array_equal(_host(env, name), _host(ref, name)), name
    if steps > 2 * J * M:
        assert env.stats()["episodes"] > B                   # episodes did end and restart (on the same instances)
    assert np.array_equal(env.packed.ops, pk.ops)


class FreshChecker:
    """every env plays the mirror's instance of its current episode; a restarted env a new one"""

    def __init__(self, env):
        self.env = env
        self.ids = env.env_id_base + np.arange(env.batch)
        self.eps = _host(env, "env_header")[:, _abi.H_EPISODE].copy()
        self.inst = {i: self.check(i) for i in range(env.batch)}
        self.changes = 0

    def check(self, i):
        e = self.env
        m, d = mirror_instance(e.instance_seed, int(self.ids[i]), int(self.eps[i]), int(e.jobs_per_env[i]),
                               int(e.machines_per_env[i]), e._gen["durations"])
        inst = e.instance(i)
        assert np.array_equal(inst.machine, m) and np.array_equal(inst.duration, d), (i, int(self.eps[i]))
        return inst

    def after_call(self):
        eps = _host(self.env, "env_header")[:, _abi.H_EPISODE]
        for i in np.flatnonzero(eps != self.eps):
            assert eps[i] == self.eps[i] + 1
            self.eps[i] = eps[i]
            old, new = self.inst[i], self.check(i)
            assert not (np.array_equal(old.machine, new.machine) and np.array_equal(old.duration, new.duration))
            self.inst[i] = new
            self.changes += 1


def case_fresh_instances(be, path, B=6, J=3, M=2, steps=60, seed=4, instance_seed=11):
    """fresh=True: after an env finishes and is restarted, env.instance(i) is the mirror's instance of its new episode (and
    differs from the one before): through step(autoreset), step_logits(autoreset), explicit -2, reset(which), JssVectorEnv"""
    from jssenv_amd.vector import JssVectorEnv
    rng = np.random.default_rng(seed)
    if path.startswith("vector"):
        venv = JssVectorEnv.generated(J, M, B, instance_seed=instance_seed, to_numpy=True, _backend=be)
        venv.reset(seed=seed)
        env = venv.env
    else:
        env = BatchedJssEnv.generated(J, M, B, instance_seed=instance_seed, fresh=True, seed=seed, _backend=be)
        env.reset()
    chk = FreshChecker(env)
    before = {i: env.instance(i) for i in range(B)}
    for it in range(steps):
        if path == "step":
            env.step(env.policy("random"), autoreset=True)
        elif path == "step_logits":
            env.step_logits(rng.standard_normal((B, env.jmax + 1)).astype(np.float32), autoreset=True)
        elif path == "reset_action":                          # -2 for the done envs, no autoreset
            a = np.array(env.backend.numpy(env.policy("random")), copy=True)
            a[_host(env, "done") != 0] = _abi.ACTION_RESET
            env.step(a)
        elif path == "reset_which":
            done = _host(env, "done")
            if done.any():
                env.reset(which=done)
            else:
                env.step(env.policy("random"))
        elif path == "vector_step":
            venv.step(env.policy("random"))
        elif path == "vector_step_logits":
            venv.step_logits(rng.standard_normal((B, env.jmax + 1)).astype(np.float32))
        chk.after_call()
    assert chk.changes >= B, chk.changes                      # every env went through several episodes
    changed = sum(not np.array_equal(before[i].duration, env.instance(i).duration) for i in range(B))
    assert changed == B


def case_refusals(be):
    env = BatchedJssEnv.generated(4, 3, 8, _backend=be)
    env.reset()
    for call in (lambda: env.rollout(n_iter=3), lambda: env.rollout_steps(steps=2), lambda: env.policy_step_steps(steps=2),
                 lambda: env.trajectory(steps=3), lambda: env.bind_rollout_steps(steps=2),
                 lambda: env.steps(np.full((2, 8), _abi.ACTION_RESET, np.int32)), lambda: env.session()):
        try:
            call()
        except RuntimeError as e:
            assert "fresh" in str(e)
        else:
            raise AssertionError("a multi-step restart under fresh=True was not refused")
    env.rollout(n_iter=1)                                     # one iteration restarts exactly the done envs: allowed
    env.steps(np.zeros((2, 8), np.int32))                     # no -2: no restart
    env.rollout(n_iter=3, autoreset=False)
    fixed = BatchedJssEnv.generated(4, 3, 8, fresh=False, _backend=be)
    fixed.reset()
    fixed.rollout(n_iter=3)
    try:
        BatchedJssEnv("ta01", batch=2, _backend=be).generate()
    except ValueError:
        pass
    else:
        raise AssertionError("generate() on a batch of fixed instances")
    for bad in (([0] * 8, [1] * 8), ([1] * 8, [2**31 - 1] * 8), ([1] * 7, [1] * 7)):
        try:
            fixed.generate(time_seed=np.array(bad[0]), machine_seed=np.array(bad[1]))
        except ValueError:
            pass
        else:
            raise AssertionError("bad explicit seeds accepted")


def case_checkpoint(be, tmp_path=None, B=10, J=4, M=3, seed=2):
    """a checkpoint of a generated batch carries its tables and instance seed: resumed, it continues bit for bit"""
    mk = lambda s: BatchedJssEnv.generated(J, M, B, instance_seed=s, seed=seed, _backend=be)   # noqa: E731
    env = mk(31)
    env.reset()
    for _ in range(25):
        env.step(env.policy("random"), autoreset=True)
    if tmp_path is None:
        ck = env.state_dict()
    else:
        ck = str(tmp_path / "gen.npz")
        env.save_checkpoint(ck)
    other = mk(99)                                            # other tables, other key: both restored
    other.load_checkpoint(ck) if tmp_path is not None else other.load_state_dict(ck)
    assert other.instance_seed == 31 and np.array_equal(other.packed.ops, env.packed.ops)
    for _ in range(40):
        env.step(env.policy("random"), autoreset=True)
        other.step(other.policy("random"), autoreset=True)
    for name in STATE:
        assert np.array_equal(_host(env, name), _host(other, name)), name
    assert np.array_equal(other.packed.ops, env.packed.ops) and np.array_equal(other.packed.inst, env.packed.inst)
    try:
        BatchedJssEnv(I.synthetic_packed(B, J, M), _backend=be).load_state_dict(env.state_dict())
    except ValueError:
        pass
    else:
        raise AssertionError("a generated batch's checkpoint loaded into a batch of fixed instances")
