"""Backend-agnostic cases of jss_clone / BatchedJssEnv.fork / copy_from / JssEnv.__deepcopy__ (env states cloned on the
device for search), run against the host-core twin, the kernel source under the SIMT emulator and the HIP library.

What a clone copies is include/jss_hip.h's list: every state and output row of the env and its instance assignment, byte for
byte; not the counters, not the global env id.  The oracle replaying an env's whole action history is the reference for
what a clone does next."""
import copy
import ctypes as C

import numpy as np

import golden_util as GU
from jssenv_amd import BatchedJssEnv, _abi
from jssenv_amd import instances as I
from oracle import OracleEnv

ROWS = ("env_header", "env_const", "job_state", "machine_state", "solution", "real_obs", "action_mask", "reward", "done",
        "makespan")
BY_SHAPE_SMALL = [f"ta{i:02d}" for i in range(1, 81, 10)]          # one instance of every ten: all four shape classes
BY_SHAPE_FULL = [f"ta{i:02d}" for i in range(1, 81)]


def host(env, name):
    return np.ascontiguousarray(env.backend.numpy(getattr(env, name)))


def rows_of(env):
    """the copied tensors as host arrays (machine clocks only where the batch stores them), plus the instance assignment"""
    out = {k: host(env, k) for k in ROWS if k != "machine_state" or not env.no_clocks}
    if env._table_of_env is not None:
        out["table_of_env"] = host(env, "_table_of_env")
    elif env._table_kind() == "own":
        out.update(ops=host(env, "_ops"), rem=host(env, "_rem"), inst=host(env, "_inst"))
    return out


def make_layout(be, name, B, seed=5, by_shape=BY_SHAPE_SMALL):
    if name == "compact":
        return BatchedJssEnv("ta01", batch=B, _backend=be, seed=seed)
    if name in ("full", "medium"):
        toe = np.arange(B) % 3
        return BatchedJssEnv(["ta01", "ta21", "ta41"], batch=B, table_of_env=toe, records=name, _backend=be, seed=seed)
    if name == "synthetic":
        return BatchedJssEnv(I.synthetic_packed(B, 15, 15), batch=B, _backend=be, seed=seed)
    if name == "generated":
        return BatchedJssEnv.generated(20, 15, B, fresh=True, _backend=be, seed=seed, instance_seed=9)
    if name == "by_shape":
        return BatchedJssEnv(by_shape, batch=B, _backend=be, seed=seed)
    raise KeyError(name)


LAYOUTS = ("compact", "full", "medium", "synthetic", "generated", "by_shape")


def drive(env, rng, n_steps, hist=None):
    """random legal actions chosen on the host, every env stopping at a step count of its own (a third never stop early):
    mixed episode positions, some envs done.  `hist[i]` collects env i's actions."""
    B = env.batch
    stop = np.where(rng.random(B) < 0.33, n_steps, rng.integers(0, n_steps, B))
    hist = hist if hist is not None else [[] for _ in range(B)]
    for t in range(n_steps):
        mask, done = host(env, "action_mask"), host(env, "done")
        acts = np.full(B, -1, np.int32)
        for i in range(B):
            if t >= stop[i] or done[i]:
                continue
            legal = np.flatnonzero(mask[i, :int(env.jobs_per_env[i]) + 1])
            acts[i] = rng.choice(legal)
            hist[i].append(int(acts[i]))
        if (acts == -1).all():
            break
        env.step(acts)
    return hist


def check_copy(parent, before, fork, index):
    got = rows_of(fork)
    for k, v in before.items():
        if k == "table_of_env" or k in ("ops", "rem", "inst"):
            continue
        want = v[index]
        if k == "env_const" and "ops" in before:        # one table per env: env index[k]'s table is the fork's table k
            want = want.copy()
            want[:, _abi.C_TABLE] = np.arange(len(index))
        assert np.array_equal(got[k], want), k
    if "table_of_env" in before:
        assert np.array_equal(got["table_of_env"], before["table_of_env"][index])
    if "ops" in before:
        for k in ("ops", "rem", "inst"):
            assert np.array_equal(got[k], before[k][index]), k
    assert not host(fork, "counters").any()


# ---- cases -------------------------------------------------------------------------------------------------------------
def case_exact_copy(be, layout, B=12, n_steps=60, seed=1, by_shape=BY_SHAPE_SMALL):
    """fork with a random index holding duplicates: every copied row of fork env k is the parent's row index[k]; then the
    parent and the fork step on with the same actions until the episodes end and stay bit-identical (continuation), and
    equal the oracle replaying every env's whole action history"""
    rng = np.random.default_rng(seed)
    env = make_layout(be, layout, B, by_shape=by_shape)
    env.reset()
    hist = drive(env, rng, n_steps)
    index = rng.integers(0, B, B + 3)
    index[1] = index[0]
    before = rows_of(env)
    f = env.fork(index, env_id_base=1000)
    be.sync()
    check_copy(env, before, f, index)
    assert rows_of(env).keys() == before.keys() and all(np.array_equal(rows_of(env)[k], v) for k, v in before.items())
    if layout == "by_shape" and (np.diff(env._class_of_table[env.table_of_env_host[index]]) >= 0).all():
        assert f.steps_by_shape_class
    # continuation: the parent's rows index[k] and the fork's row k take the same actions; the parent's extra envs skip
    cont = [list(hist[i]) for i in index]
    for _ in range(4000):
        mask, done = host(f, "action_mask"), host(f, "done")
        acts = np.full(f.batch, -1, np.int32)
        for k in range(f.batch):
            if not done[k]:
                legal = np.flatnonzero(mask[k, :int(f.jobs_per_env[k]) + 1])
                acts[k] = legal[(len(cont[k]) * 7 + k) % legal.size]
        if (acts == -1).all():
            break
        # the parent takes the fork's actions: for duplicates only the first copy's (the parent has one env per index)
        pa = np.full(B, -1, np.int32)
        first = {}
        for k in range(f.batch):
            first.setdefault(int(index[k]), k)
        for i, k in first.items():
            pa[i] = acts[k]
        for k in range(f.batch):
            if acts[k] >= 0:
                cont[k].append(int(acts[k]))
        f.step(acts)
        env.step(pa)
    else:
        raise AssertionError("episodes did not end")
    fr, pr = rows_of(f), rows_of(env)
    for k in range(f.batch):
        i = int(index[k])
        if first[i] != k:
            continue
        for name in ("env_header", "env_const", "job_state", "solution", "real_obs", "action_mask", "reward", "done",
                     "makespan"):
            a, b = fr[name][k].copy(), pr[name][i].copy()
            if name == "env_const" and "ops" in fr:      # (the table word names each batch's own table)
                assert (a[_abi.C_TABLE], b[_abi.C_TABLE]) == (k, i)
                a[_abi.C_TABLE] = b[_abi.C_TABLE] = 0
            assert np.array_equal(a, b), (name, k, i)
    assert fr["done"].all()
    # the oracle replays every fork env's whole history
    for k in range(f.batch):
        inst = f.instance(k)
        orc = OracleEnv(inst, strict=True)
        orc.reset()
        for a in cont[k]:
            orc.step(a)
        J, M = inst.jobs, inst.machines
        assert int(fr["makespan"][k]) == orc.current_time_step, k
        assert np.array_equal(fr["solution"][k][:J, :M], orc.solution), k
    return f


def case_facade_deepcopy(device=None, backend=None):
    """published ta01: half the trace, deepcopy, the copy finishes it (schedule and makespan 1231 of tests/golden); the
    original is untouched by the copy's steps, then finishes too; closing the original leaves the copy working"""
    from jssenv_amd import make
    g = GU.load("published_ta01")
    kw = {"_backend": backend} if backend is not None else {"device": device}
    env = make("jss-v1", env_config={"instance_path": "ta01"}, **kw)
    acts = [int(a) for a in g["action"]]
    half = len(acts) // 2

    def play(e, seq):
        for a in seq:
            if a == -2:
                e.reset()
            elif a == -1:
                e.increase_time_step()
            else:
                e.step(a)

    env.reset()
    play(env, acts[:half])
    snap = {k: np.array(v, copy=True) for k, v in env._b.host_tensors().items() if k != "counters"}
    sol = np.array(env.solution, copy=True)
    c = copy.deepcopy(env)
    assert c is not env and c._b is not env._b and c._b._arena is not env._b._arena
    assert c.current_time_step == env.current_time_step and np.array_equal(c.solution, sol)
    assert c._alloc_log == env._alloc_log and c._alloc_log is not env._alloc_log
    play(c, acts[half:])
    assert c.last_time_step == GU.PUBLISHED_MAKESPAN["ta01"] == int(g["makespan"])
    assert np.array_equal(c.solution, g["solution"]) and np.array_equal(c.last_solution, g["solution"])
    now = env._b.host_tensors()
    for k, v in snap.items():
        assert np.array_equal(now[k], v), k
    assert np.array_equal(env.solution, sol)
    play(env, acts[half:])
    assert env.last_time_step == 1231 and np.array_equal(env.solution, g["solution"])
    # closing the original leaves the copy working
    c2 = copy.deepcopy(env)
    env.close()
    del env
    c2.reset()
    play(c2, acts[:40])
    assert c2.current_time_step == int(g["clock"][39])
    c.close()
    c2.close()


def case_copy_from(be):
    """-1 entries, in-place disjoint clones, refusals (layout, tables, overlap, open session, by-shape class)"""
    rng = np.random.default_rng(3)
    env = make_layout(be, "full", 9)
    env.reset()
    drive(env, rng, 40)
    other = make_layout(be, "full", 6, seed=8)
    other.reset()
    drive(other, rng, 25)
    before, src = rows_of(env), rows_of(other)
    idx = np.array([-1, 2, -1, 0, 5, -1, 1, -1, 3], np.int32)
    env.copy_from(other, idx)
    after = rows_of(env)
    for k, i in enumerate(idx):
        for name, v in after.items():
            want = before[name][k] if i < 0 else src[name][i]
            assert np.array_equal(v[k], want), (name, k)
    assert env.table_of_env_host.tolist() == [before["table_of_env"][k] if i < 0 else src["table_of_env"][i]
                                              for k, i in enumerate(idx)]
    # in place, disjoint: a slot pool
    before = rows_of(env)
    idx = np.full(9, -1, np.int32)
    idx[[0, 4, 8]] = [3, 3, 6]
    env.copy_from(env, idx)
    after = rows_of(env)
    for k in range(9):
        i = idx[k] if idx[k] >= 0 else k
        for name, v in after.items():
            assert np.array_equal(v[k], before[name][i]), (name, k)
    for bad in ([1, 2, -1, -1, -1, -1, -1, -1, -1], [-1, 2, 1, -1, -1, -1, -1, -1, -1], [0] + [-1] * 8):
        try:
            env.copy_from(env, bad)
        except ValueError:
            pass
        else:
            raise AssertionError("an overlapping in-place clone was accepted")
    # layout and table mismatches
    refusals = [make_layout(be, "medium", 9), make_layout(be, "compact", 9), make_layout(be, "synthetic", 9),
                BatchedJssEnv(["ta02", "ta21", "ta41"], batch=9, table_of_env=np.arange(9) % 3, records="full", _backend=be)]
    for r in refusals:
        r.reset()
        try:
            env.copy_from(r, np.zeros(9, np.int32))
        except ValueError:
            pass
        else:
            raise AssertionError("a mismatched source was accepted")
    for bad in (np.zeros(8, np.int32), np.full(9, 9, np.int32), np.full(9, -2, np.int32)):
        try:
            env.copy_from(other if bad.size == 9 and bad[0] == 9 else env, bad)
        except ValueError:
            pass
        else:
            raise AssertionError("a bad index was accepted")
    # by shape: an env keeps its class
    bs = make_layout(be, "by_shape", 12)
    bs.reset()
    cls = bs._class_of_table[bs.table_of_env_host]
    ok = np.array([int(np.flatnonzero(cls == cls[k])[-1]) for k in range(12)], np.int32)
    bs.copy_from(bs.fork(np.arange(12)), ok)
    assert bs.steps_by_shape_class
    wrong = np.full(12, -1, np.int32)
    wrong[0] = int(np.flatnonzero(cls != cls[0])[0])
    try:
        bs.copy_from(bs.fork(np.arange(12)), wrong)
    except ValueError:
        pass
    else:
        raise AssertionError("a by-shape class violation was accepted")


def raw_clone(be, dst, src, index, dst_tables=None):
    """jss_clone through the C ABI; `index` a host array (uploaded)"""
    p = be.ptr
    with be.on_device():
        w = be.from_numpy(np.ascontiguousarray(index, dtype=np.int32))
        dt = dst_tables if dst_tables is not None else _abi.JssCloneDst(p(dst._table_of_env), p(dst._ops), p(dst._rem),
                                                                        p(dst._inst))
        rc = be.lib.jss_clone(C.byref(dst._desc), C.byref(dst._state), C.byref(dst._out), C.byref(dt) if dt else None,
                              C.byref(src._desc), C.byref(src._state), C.byref(src._out), p(w), be.stream())
        be.sync()
    return rc


def case_abi_errors(be):
    """JSS_E_SHAPE / JSS_E_NULL from the library; out-of-range entries set JSS_ERR_BAD_INDEX and touch nothing else"""
    full, medium = make_layout(be, "full", 6), make_layout(be, "medium", 6)
    comp, syn = make_layout(be, "compact", 6), make_layout(be, "synthetic", 6)
    toe5 = BatchedJssEnv(["ta01", "ta21", "ta41", "ta02"], batch=6, table_of_env=np.arange(6) % 4, records="full", _backend=be)
    for e in (full, medium, comp, syn, toe5):
        e.reset()
    z = np.zeros(6, np.int32)
    assert raw_clone(be, full, medium, z) == _abi.E_SHAPE          # record layout
    assert raw_clone(be, full, toe5, z) == _abi.E_SHAPE            # n_tables of a table_of_env batch
    assert raw_clone(be, comp, syn, z) == _abi.E_SHAPE             # one shared table vs one table per env
    assert raw_clone(be, syn, syn.fork(np.arange(6)), z, dst_tables=_abi.JssCloneDst()) == _abi.E_SHAPE
    assert raw_clone(be, full, full.fork(np.arange(6)), z, dst_tables=_abi.JssCloneDst()) == _abi.E_SHAPE
    p = be.ptr
    rc = be.lib.jss_clone(C.byref(full._desc), C.byref(full._state), C.byref(full._out), None, C.byref(full._desc),
                          C.byref(full._state), C.byref(full._out), None, be.stream())
    assert rc == _abi.E_NULL
    assert be.lib.jss_clone(None, C.byref(full._state), C.byref(full._out), None, C.byref(full._desc),
                            C.byref(full._state), C.byref(full._out), p(full._act_in), be.stream()) == _abi.E_NULL
    # bad entries: the env is untouched but for the status bit; the good entries are copied
    drive(full, np.random.default_rng(2), 20)
    src = full.fork([5, 4, 3, 2, 1, 0])
    drive(src, np.random.default_rng(4), 10)
    before, s = rows_of(full), rows_of(src)
    idx = np.array([6, -2, 1, 1 << 30, -1, 0], np.int32)
    assert raw_clone(be, full, src, idx) == 0
    after = rows_of(full)
    for k, i in enumerate(idx):
        for name, v in after.items():
            if 0 <= i < 6:
                assert np.array_equal(v[k], s[name][i]), (name, k)
            elif name == "env_header" and i != -1:
                want = before[name][k].copy()
                want[_abi.H_STATUS] |= _abi.ERR_BAD_INDEX
                assert np.array_equal(v[k], want), k
            else:
                assert np.array_equal(v[k], before[name][k]), (name, k)


def case_session_refused(be):
    env = make_layout(be, "full", 6)
    env.reset()
    other = env.fork(np.arange(6))

    class _Open:
        closed = False
    env._session = _Open()
    for call in (lambda: env.fork([0]), lambda: env.copy_from(other, np.zeros(6, np.int32)),
                 lambda: other.copy_from(env, np.zeros(6, np.int32))):
        try:
            call()
        except RuntimeError:
            pass
        else:
            raise AssertionError("a clone with an open session was accepted")
    env._session = None


def case_divergence(be, steps=40):
    """two clones of one parent draw different random actions (their global ids differ); returns their rows"""
    env = make_layout(be, "compact", 4, seed=11)
    env.reset()
    env.rollout("random", n_iter=20, autoreset=False)
    f = env.fork([2, 2], env_id_base=0)
    f.rollout_steps("random", steps=steps, n_sub=1, autoreset=False)
    r = rows_of(f)
    assert not np.array_equal(r["job_state"][0], r["job_state"][1])
    return r


def case_pilot(be, n_parents=1, children=None, prefix=30, seed=0, check_oracle=True):
    """the pilot method on ta01: after `prefix` SPT steps (parents > 1: random steps, different per parent), one child per
    legal action (or `children` per parent, legal actions taken cyclically), each child steps its action and finishes with
    SPT.  Returns (fork rows, actions)."""
    env = BatchedJssEnv("ta01", batch=n_parents, _backend=be, seed=seed)
    env.reset()
    env.rollout("SPT" if n_parents == 1 else "random", n_iter=prefix, autoreset=False)
    mask = host(env, "action_mask")
    if children is None:
        legal = np.flatnonzero(mask[0])
        index, acts = np.zeros(legal.size, np.int64), legal.astype(np.int32)
    else:
        index = np.repeat(np.arange(n_parents), children)
        acts = np.empty(index.size, np.int32)
        for i in range(n_parents):
            legal = np.flatnonzero(mask[i])
            acts[i * children:(i + 1) * children] = legal[np.arange(children) % legal.size]
    f = env.fork(index)
    f.step(acts)
    f.rollout("SPT", n_iter=15 * 15 * 3, autoreset=False)
    r = rows_of(f)
    assert r["done"].all()
    if check_oracle:
        inst = I.resolve_instance("ta01")
        for k in range(f.batch):
            orc = OracleEnv(inst, strict=True)
            orc.reset()
            for _ in range(prefix):
                if not orc.legal_actions.any():
                    break
                orc.step(orc.policy("SPT"))
            orc.step(int(acts[k]))
            while orc.legal_actions.any():
                orc.step(orc.policy("SPT"))
            assert int(r["makespan"][k]) == orc.current_time_step, k
            assert np.array_equal(r["solution"][k], orc.solution), k
    return r, acts
