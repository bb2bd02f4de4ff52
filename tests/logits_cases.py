"""Backend-agnostic cases of BatchedJssEnv.step_logits / jss_step_logits (the masked categorical draw from the caller's
logits fused into the step), run against the host-core twin, the kernel source under the SIMT emulator and the HIP library.

The NumPy mirror below restates the draw exactly as include/jss_hip.h documents it: the random policy's counter RNG keyed
with seed ^ K_LOGITS, one fmix32 per action index, u = ((r >> 8) + 0.5) 2^-24, Gumbel noise -log(-log(u)), argmax of
l / T + g over the legal entries, lowest index on ties -- in float32."""
import numpy as np

import parity_cases as P
from jssenv_amd import BatchedJssEnv, _abi
from jssenv_amd import instances as I
from oracle import OracleEnv

M32 = 0xFFFFFFFF
NEAR_TIE = 1e-5
LOGP_TOL = 2e-5


# ---- the documented formula, in NumPy ------------------------------------------------------------------------------
def fmix32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def rng_u32(seed, env_id, episode, step):
    """oracle/jss_oracle.c orc_rng_u32, vectorised over env_id / episode / step"""
    seed = int(seed) & ((1 << 64) - 1)
    env_id = np.asarray(env_id, dtype=np.uint64)
    episode = np.asarray(episode, dtype=np.int64).astype(np.uint64) & M32
    step = np.asarray(step, dtype=np.int64).astype(np.uint64) & M32
    a = (np.uint64(seed & M32) + (env_id & M32) * np.uint64(0x9E3779B9) + episode * np.uint64(0x85EBCA6B)
         + step * np.uint64(0xC2B2AE35)) & M32
    b = np.uint64(seed >> 32) ^ (((env_id >> np.uint64(32)) * np.uint64(0x27D4EB2F)) & M32)
    return fmix32(fmix32(a) ^ b)


def legal_entries(mask, jobs):
    """(B, W) bool: the entries that take part -- the mask row holds the legal jobs and NOPE at J(env), zeros behind it"""
    W = mask.shape[1]
    return (mask != 0) & (np.arange(W)[None, :] <= np.asarray(jobs)[:, None])


def mirror(logits, part, T, seed, env_ids, episode, step):
    """(actions, scores, gap): the mirror's choice per env, its perturbed scores (-inf where an entry does not take part)
    and the gap between its two best scores (inf with a single entry)."""
    l = np.asarray(logits, dtype=np.float32)
    l = np.where(np.isnan(l) | (l == np.inf), np.float32(-np.inf), l)
    B, W = l.shape
    if T > 0:
        r = rng_u32(seed ^ _abi.LOGITS_SEED_XOR, env_ids, episode, step)[:, None]
        ra = fmix32(r + np.arange(W, dtype=np.uint64)[None, :] * np.uint64(0x9E3779B9))
        u = ((ra >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
        with np.errstate(divide="ignore"):
            g = -np.log(-np.log(u))
        score = (l / np.float32(T)).astype(np.float32) + g.astype(np.float32)
    else:
        score = l.copy()
    score = np.where(part, score, np.float32(-np.inf))
    score_sel = np.where(part, score, np.nan)
    best = np.full(B, -1)
    any_part = part.any(axis=1)
    # lowest index among the maxima (nan-aware: entries that do not take part never win)
    mx = np.nanmax(np.where(any_part[:, None], score_sel, 0.0), axis=1)
    best[any_part] = np.argmax((score_sel == mx[:, None]) & part, axis=1)[any_part]
    srt = np.sort(np.where(part, score, -np.inf), axis=1)
    with np.errstate(invalid="ignore"):
        gap = np.where(part.sum(axis=1) >= 2, srt[:, -1] - srt[:, -2], np.inf)
    return best, score, gap


def reference_logp_entropy(logits, part, actions, T):
    """float64 masked log_softmax / entropy of logits / T (T = 0: T = 1) at `actions` (rows with an action >= 0)"""
    x = np.asarray(logits, dtype=np.float64) / (T if T > 0 else 1.0)
    x = np.where(part, x, -np.inf)
    m = x.max(axis=1, keepdims=True)
    z = np.exp(x - m)
    s = z.sum(axis=1, keepdims=True)
    logp_all = x - m - np.log(s)
    p = z / s
    with np.errstate(invalid="ignore"):
        ent = -(np.where(p > 0, p * logp_all, 0.0)).sum(axis=1)
    rows = np.arange(len(actions))
    return logp_all[rows, np.maximum(actions, 0)], ent


# ---- driving one call -----------------------------------------------------------------------------------------------
def context(env):
    """what the draw of the next call depends on: mask, J(env), the RNG key words, the done flags"""
    n = env.backend.numpy
    hdr = n(env.env_header)
    ids = n(env._env_ids) if env._env_ids is not None else env.env_id_base + np.arange(env.batch)
    return {"mask": n(env.action_mask).copy(), "jobs": np.asarray(env.jobs_per_env), "episode": hdr[:, _abi.H_EPISODE].copy(),
            "step": hdr[:, _abi.H_STEP].copy(), "done": n(env.done).copy(), "env_ids": np.asarray(ids, dtype=np.uint64)}


def to_backend(env, x):
    """host logits (B, W) float32 -> what the env's backend takes"""
    be = env.backend
    if hasattr(be, "torch"):
        return be.torch.as_tensor(np.ascontiguousarray(x), device=be.device)
    return np.ascontiguousarray(x, dtype=np.float32)


def step_and_check(env, logits, T, seed, autoreset=False, status_mask=0xFF, check_state=True):
    """step_logits on `env` with host logits (B, W) -- then the same state restored and stepped with step(actions):
    every state and output tensor must end bit-equal (`status_mask`: the status bits that must agree; a bad logit flags
    JSS_ERR_BAD_LOGITS, which a plain step does not).  Returns (ctx, action, logp, entropy)."""
    n = env.backend.numpy
    ctx = context(env)
    start = P._state_snapshot(env)
    _, _, _, _, info = env.step_logits(to_backend(env, logits) if isinstance(logits, np.ndarray) else logits,
                                       temperature=T, seed=seed, autoreset=autoreset, logp=True, entropy=True)
    act = n(info["action"]).astype(np.int64).copy()
    logp, ent = n(info["logp"]).copy(), n(info["entropy"]).copy()
    if check_state:
        after = P._state_snapshot(env)
        P._restore(env, start, start["solution"])
        env.step(act.astype(np.int32), autoreset=autoreset)
        again = P._state_snapshot(env)
        for k in after:
            a, b = after[k], again[k]
            if k == "env_header":
                a, b = a.copy(), b.copy()
                a[:, _abi.H_STATUS] &= ~0xFF | status_mask
                b[:, _abi.H_STATUS] &= ~0xFF | status_mask
            assert np.array_equal(a, b), f"step_logits != step(action): {k}"
        if status_mask != 0xFF:                        # leave the env as step_logits left it
            P._restore(env, after, after["solution"])
    return ctx, act, logp, ent


def check_draw(ctx, logits, act, logp, ent, T, seed, autoreset=False, stats=None):
    """the codes, legality, the mirror's choice (near-ties excepted, counted in stats) and logp / entropy"""
    part = legal_entries(ctx["mask"], ctx["jobs"])
    W = part.shape[1]
    lg = np.asarray(logits, dtype=np.float32)[:, :W]
    reset = (ctx["done"] != 0) & autoreset
    none = ~part.any(axis=1)
    assert (act[reset] == _abi.ACTION_RESET).all()
    assert (act[none & ~reset] == _abi.ACTION_SKIP).all()
    live = ~reset & ~none
    assert (logp[~live] == 0).all() and (ent[~live] == 0).all()
    rows = np.flatnonzero(live)
    assert (act[rows] >= 0).all() and (act[rows] <= ctx["jobs"][rows]).all()
    assert part[rows, act[rows]].all(), "an action outside the legal set"
    want, _, gap = mirror(lg, part, T, seed, ctx["env_ids"], ctx["episode"], ctx["step"])
    diff = rows[act[rows] != want[rows]]
    assert (gap[diff] <= NEAR_TIE).all(), f"draws differ from the mirror away from a near-tie: envs {diff[gap[diff] > NEAR_TIE][:8]}"
    if stats is not None:
        stats["draws"] = stats.get("draws", 0) + rows.size
        stats["near_tie_diff"] = stats.get("near_tie_diff", 0) + diff.size
    finite = rows[np.isfinite(np.where(part[rows], lg[rows], -np.inf)).any(axis=1)]
    rl, re_ = reference_logp_entropy(lg[finite], part[finite], act[finite], T)
    assert np.abs(logp[finite] - rl).max(initial=0) <= LOGP_TOL, np.abs(logp[finite] - rl).max()
    assert np.abs(ent[finite] - re_).max(initial=0) <= LOGP_TOL, np.abs(ent[finite] - re_).max()
    return want


def random_logits(rng, B, W, ties=False, scale=2.0):
    if ties:
        return rng.integers(-2, 3, size=(B, W)).astype(np.float32)
    return (rng.standard_normal((B, W)) * scale).astype(np.float32)


class Replay:
    """OracleEnv per env, driven with the actions the env took (reset on -2, nothing on -1)"""

    def __init__(self, env):
        self.env = env
        self.orcs = [OracleEnv(env.instances[env.instance_of_env(i)], strict=True) for i in range(env.batch)]
        for o in self.orcs:
            o.reset()

    def step(self, act):
        for i, o in enumerate(self.orcs):
            if act[i] == _abi.ACTION_RESET:
                o.reset()
            elif act[i] != _abi.ACTION_SKIP:
                o.step(int(act[i]))

    def check(self, where):
        for i, o in enumerate(self.orcs):
            P.assert_matches_oracle(self.env.host_state(i), o, f"{where} env {i}")


# ---- the cases ------------------------------------------------------------------------------------------------------
def case_greedy(backend, insts, batch, steps, order=None, seed=3):
    """T = 0 with ties injected: the masked argmax, lowest index; state == step(action); every env against the oracle"""
    env = BatchedJssEnv(insts, batch=batch, seed=seed, env_id_base=40, order=order, _backend=backend)
    env.reset()
    orc = Replay(env)
    rng = np.random.default_rng(seed)
    W = env.jmax + 1
    for it in range(steps):
        logits = random_logits(rng, batch, W, ties=True)
        ctx, act, logp, ent = step_and_check(env, logits, 0.0, seed)
        part = legal_entries(ctx["mask"], ctx["jobs"])
        rows = np.flatnonzero(part.any(axis=1))
        want = np.argmax(np.where(part, logits, -np.inf), axis=1)
        assert np.array_equal(act[rows], want[rows]), f"iter {it}: greedy"
        check_draw(ctx, logits, act, logp, ent, 0.0, seed)
        orc.step(act)
    orc.check("greedy")
    return env


def case_sampled(backend, insts, batch, steps, T, order=None, seed=5, stats=None):
    """T > 0: legal, logp / entropy against float64, the mirror's draws, state == step(action)"""
    env = BatchedJssEnv(insts, batch=batch, seed=seed, env_id_base=7, order=order, _backend=backend)
    env.reset()
    rng = np.random.default_rng(seed + 1)
    stats = {} if stats is None else stats
    for it in range(steps):
        logits = random_logits(rng, batch, env.jmax + 1)
        ctx, act, logp, ent = step_and_check(env, logits, T, seed + it, autoreset=True)
        check_draw(ctx, logits, act, logp, ent, T, seed + it, autoreset=True, stats=stats)
    assert stats["near_tie_diff"] <= 0.001 * stats["draws"], stats
    return env


def case_nope_and_padding(backend, steps=40, seed=9):
    """a huge logit behind J(env) or on an illegal job is never taken; NOPE (index J(env)) is taken when it is legal and
    dominant -- ragged, padded batch"""
    insts = [P.random_instance(np.random.default_rng(s), j, m) for s, (j, m) in enumerate(((3, 3), (5, 4), (4, 2), (7, 3)))]
    env = BatchedJssEnv(insts, batch=8, seed=seed, order="interleaved", _backend=backend)
    env.reset()
    rng = np.random.default_rng(seed)
    B, W = env.batch, env.jmax + 1
    J = np.asarray(env.jobs_per_env)
    nope_taken = 0
    for it in range(steps):
        ctx = context(env)
        part = legal_entries(ctx["mask"], J)
        logits = random_logits(rng, B, W)
        cols = np.arange(W)[None, :]
        logits[cols > J[:, None]] = 1e30                                  # behind J(env): the padding of the row
        illegal_job = (cols < J[:, None]) & ~part
        logits[illegal_job] = 1e30
        dominant = it % 2 == 0
        if dominant:
            logits[np.arange(B), J] = 60.0
        ctx, act, logp, ent = step_and_check(env, logits, 1.0, seed + it, autoreset=True)
        live = act >= 0
        assert (act[live] <= J[live]).all() and part[live, act[live]].all()
        if dominant:
            nope_legal = live & part[np.arange(B), J]
            assert (act[nope_legal] == J[nope_legal]).all(), f"iter {it}: NOPE legal and dominant but not taken"
            nope_taken += int(nope_legal.sum())
    assert nope_taken > 0, "no state with NOPE legal was reached"


def case_nope_fold(backend, jobs, machines, batch=4, steps=30, seed=31):
    """an instance whose J fills the lanes of its env -- J == 16 / 32 in 16- / 32-lane groups, J == 64 / 128 with one / two jobs
    per lane -- has NOPE's entry behind the lanes, folded in after the reduction.  NOPE is made dominant in the even envs
    only, so that within one wavefront some envs take NOPE and others a job: every draw against the
    mirror, every state against step(action), and NOPE must have been taken (the machine counts are ones at which NOPE
    becomes legal within the first steps)"""
    inst = P.random_instance(np.random.default_rng(seed), jobs, machines)
    env = BatchedJssEnv(inst, batch=batch, seed=seed, env_id_base=3, _backend=backend)
    env.reset()
    rng = np.random.default_rng(seed)
    B, W = env.batch, env.jmax + 1
    assert W == jobs + 1
    stats, nope_taken, job_taken = {}, 0, 0
    for it in range(steps):
        logits = random_logits(rng, B, W)
        logits[0::2, jobs] = 60.0
        ctx, act, logp, ent = step_and_check(env, logits, 1.0, seed + it, autoreset=True)
        check_draw(ctx, logits, act, logp, ent, 1.0, seed + it, autoreset=True, stats=stats)
        nope_taken += int((act == jobs).sum())
        job_taken += int(((act >= 0) & (act < jobs)).sum())
    assert nope_taken > 0 and job_taken > 0, (nope_taken, job_taken)
    assert stats["near_tie_diff"] <= 0.001 * stats["draws"], stats


def case_signed_zero_ties(backend, inst="ta01", batch=4):
    """greedy ties are float comparisons: -0 ties with +0 and the lower index wins, whichever of the two is -0"""
    env = BatchedJssEnv(inst, batch=batch, seed=1, _backend=backend)
    env.reset()
    W = env.jmax + 1
    for lo, hi in ((-0.0, 0.0), (0.0, -0.0)):
        logits = np.full((batch, W), -5.0, dtype=np.float32)
        logits[:, 2], logits[:, 7] = lo, hi
        ctx, act, logp, ent = step_and_check(env, logits, 0.0, 1)
        part = legal_entries(ctx["mask"], ctx["jobs"])
        assert part[:, 2].all() and part[:, 7].all()
        assert (act == 2).all(), act
        env.reset()


def case_broadcast_row(backend, inst="ta01", batch=64):
    """one logits row broadcast over the batch (stride 0 between rows) is a view the env accepts: it draws what the same
    row repeated in memory draws"""
    env = BatchedJssEnv(inst, batch=batch, seed=2, _backend=backend)
    env.reset()
    n = env.backend.numpy
    W = env.jmax + 1
    row = np.full(W, -1.0, dtype=np.float32)
    row[3] = 50.0
    start = P._state_snapshot(env)
    want = n(env.step_logits(to_backend(env, np.tile(row, (batch, 1))), temperature=0.0)[4]["action"]).copy()
    assert (want == 3).all()
    if hasattr(env.backend, "torch"):
        views = [env.backend.torch.as_tensor(row, device=env.backend.device).expand(batch, -1)]
    else:
        import torch
        views = [np.broadcast_to(row, (batch, W)), torch.from_numpy(row).expand(batch, -1)]
    for v in views:
        P._restore(env, start, start["solution"])
        got = n(env.step_logits(v, temperature=0.0)[4]["action"]).copy()
        assert np.array_equal(got, want), (type(v), got)


def case_determinism(backend, inst="ta01", batch=8, seed=13):
    """same seed + same state -> same actions; another seed, the next step, another env_id_base -> other draws"""
    env = BatchedJssEnv(inst, batch=batch, seed=seed, env_id_base=0, _backend=backend)
    other = BatchedJssEnv(inst, batch=batch, seed=seed, env_id_base=1000, _backend=backend)
    env.reset()
    other.reset()
    n = env.backend.numpy
    logits = np.zeros((batch, env.jmax + 1), dtype=np.float32)      # uniform: the draw is all noise
    start = P._state_snapshot(env)

    def draw(e, sd):
        return n(e.step_logits(to_backend(e, logits), seed=sd)[4]["action"]).copy()
    a1 = draw(env, 1)
    P._restore(env, start, start["solution"])
    assert np.array_equal(draw(env, 1), a1), "same seed, same state"
    P._restore(env, start, start["solution"])
    assert not np.array_equal(draw(env, 2), a1), "another seed"
    assert not np.array_equal(draw(other, 1), a1), "another env_id_base"
    ctx = context(env)                                              # the next step: its key differs (a step further)
    a2 = draw(env, 1)
    part = legal_entries(ctx["mask"], ctx["jobs"])
    want, _, _ = mirror(logits, part, 1.0, 1, ctx["env_ids"], ctx["episode"], ctx["step"])
    assert np.array_equal(a2, want)
    stale, _, _ = mirror(logits, part, 1.0, 1, ctx["env_ids"], ctx["episode"], ctx["step"] - 1)
    assert not np.array_equal(want, stale)


def case_autoreset_and_done(backend, steps=45, seed=17):
    """small instances, so that episodes end: with autoreset a done env records -2 (logp 0) and is reset as
    step_autoreset resets it; without, it records -1 (logp 0) and stays as a SKIP leaves it"""
    insts = [P.random_instance(np.random.default_rng(s), 3, 2) for s in range(2)]
    for autoreset in (True, False):
        env = BatchedJssEnv(insts, batch=6, seed=seed, order="interleaved", _backend=backend)
        env.reset()
        rng = np.random.default_rng(seed)
        codes = set()
        for it in range(steps):
            logits = random_logits(rng, env.batch, env.jmax + 1)
            ctx, act, logp, ent = step_and_check(env, logits, 1.0, seed, autoreset=autoreset)
            check_draw(ctx, logits, act, logp, ent, 1.0, seed, autoreset=autoreset)
            codes |= set(act[act < 0].tolist())
        assert codes == ({_abi.ACTION_RESET} if autoreset else {_abi.ACTION_SKIP}), codes


def case_bf16_and_stride(backend, inst="ta41", batch=6, steps=8, seed=21):
    """bf16 logits draw exactly what f32 logits holding the same bf16-rounded values draw; a row stride wider than
    jmax + 1 reads the same rows"""
    import torch
    env = BatchedJssEnv(inst, batch=batch, seed=seed, _backend=backend)
    env.reset()
    n = env.backend.numpy
    dev = env.backend.device if hasattr(env.backend, "torch") else "cpu"
    g = torch.Generator().manual_seed(seed)
    W = env.jmax + 1
    for it in range(steps):
        x = (torch.randn(batch, W, generator=g) * 3).to(torch.bfloat16)
        wide = torch.full((batch, W + 9), float("nan"))
        wide[:, :W] = x.float()
        start = P._state_snapshot(env)
        runs = []
        for lg in (x.to(dev), x.float().to(dev), wide.to(dev)[:, :W]):
            P._restore(env, start, start["solution"])
            info = env.step_logits(lg, temperature=0.7, seed=seed, autoreset=True, entropy=True)[4]
            runs.append((n(info["action"]).copy(), n(info["logp"]).copy(), n(info["entropy"]).copy(), P._state_snapshot(env)))
        for r in runs[1:]:
            assert np.array_equal(r[0], runs[0][0]) and np.array_equal(r[1], runs[0][1]) and np.array_equal(r[2], runs[0][2])
            for k in r[3]:
                assert np.array_equal(r[3][k], runs[0][3][k]), k


def case_bad_logits(backend, inst="ta01", batch=6, seed=4):
    """NaN / +inf on a legal entry: flagged, read as -inf; every legal entry -inf: the lowest legal action, logp -inf;
    argument errors of the C call"""
    import ctypes as C
    env = BatchedJssEnv(inst, batch=batch, seed=seed, _backend=backend)
    env.reset()
    n = env.backend.numpy
    ctx = context(env)
    part = legal_entries(ctx["mask"], ctx["jobs"])
    first = np.argmax(part, axis=1)
    logits = np.zeros((batch, env.jmax + 1), dtype=np.float32)
    logits[0, first[0]] = np.nan
    logits[1, first[1]] = np.inf
    logits[2] = -np.inf                                                # every entry -inf
    logits[3, first[3]] = 1e4                                          # (a clean env: chosen, no flag)
    ctx, act, logp, ent = step_and_check(env, logits, 1.0, seed, status_mask=0xFF & ~_abi.ERR_BAD_LOGITS)
    err = n(env.env_header)[:, _abi.H_STATUS] & 0xFF
    assert err[0] & _abi.ERR_BAD_LOGITS and err[1] & _abi.ERR_BAD_LOGITS, err
    assert not (err[2:] & _abi.ERR_BAD_LOGITS).any(), err
    assert act[0] != first[0] and act[1] != first[1]
    assert act[2] == first[2] and logp[2] == -np.inf and ent[2] == 0
    assert act[3] == first[3]
    # argument errors
    d, s, o = env._refs()
    lib = env.backend.lib
    buf = to_backend(env, logits)
    ptr = buf.data_ptr() if hasattr(buf, "data_ptr") else buf.ctypes.data
    outa = env.backend.ptr(env._lg_action)

    def rc(**kw):
        a = dict(logits=ptr, row=0, dtype=_abi.LOGITS_F32, temperature=1.0, action=outa, logp=None, entropy=None)
        a.update(kw)
        lg = _abi.JssLogits(a["logits"], a["row"], a["dtype"], a["temperature"], a["action"], a["logp"], a["entropy"])
        r = lib.jss_step_logits(d, s, C.byref(lg), 1, 0, o, env.backend.stream())
        env.backend.sync()
        return r
    assert rc(logits=None) == _abi.E_NULL and rc(action=None) == _abi.E_NULL
    assert lib.jss_step_logits(d, s, None, 1, 0, o, env.backend.stream()) == _abi.E_NULL
    assert rc(row=env.jmax) == _abi.E_SHAPE
    assert rc(dtype=2) == _abi.E_KIND and rc(temperature=-1.0) == _abi.E_KIND and rc(temperature=float("nan")) == _abi.E_KIND


def chi_square_p(counts, probs):
    from scipy.stats import chisquare
    keep = probs > 0
    return chisquare(counts[keep], probs[keep] / probs[keep].sum() * counts.sum()).pvalue


def case_distribution(backend, batch=4096, inst="ta01", seed=77, T=1.0):
    """envs that share one instance just after reset take one logits row: the empirical distribution of the actions is
    softmax(logits / T) over the legal entries (chi-square at a fixed seed)"""
    env = BatchedJssEnv(inst, batch=batch, seed=seed, _backend=backend)
    env.reset()
    n = env.backend.numpy
    ctx = context(env)
    part = legal_entries(ctx["mask"], ctx["jobs"])
    assert (part == part[0]).all()
    W = env.jmax + 1
    row = np.linspace(-1.5, 1.5, W).astype(np.float32)
    logits = np.tile(row, (batch, 1))
    act = n(env.step_logits(to_backend(env, logits), temperature=T, seed=seed)[4]["action"])
    counts = np.bincount(act, minlength=W).astype(np.float64)
    assert counts[~part[0]].sum() == 0
    x = np.where(part[0], row.astype(np.float64) / T, -np.inf)
    p = np.exp(x - x.max())
    p /= p.sum()
    pv = chi_square_p(counts, p)
    assert pv > 1e-3, (pv, counts, p * batch)
    return pv


def case_full_size(hip_backend, label, kw, steps=200, checks=(0, 50, 199), seed=29, sample=256):
    """step_logits with random logits (autoreset) on a full-size batch: the host twin, driven with HIP's actions, holds the
    same state at the checkpoints on every env; the twin's own draws agree with HIP's except near-ties; `sample` envs spread
    over the batch (every shape class of a by-shape batch) replayed through the oracle at the end -- the oracle steps one env
    per call from Python, so all of them would take minutes; every env is held to the oracle through the twin instead"""
    from jssenv_amd.env import CpuBackend
    torch = hip_backend.torch
    hip = BatchedJssEnv(seed=seed, env_id_base=11, _backend=hip_backend, **kw)
    twin = BatchedJssEnv(seed=seed, env_id_base=11, _backend=CpuBackend(), kernel=hip.kernel, **kw)   # (same record layout)
    hip.reset()
    twin.reset()
    B, W = hip.batch, hip.jmax + 1
    pick = np.linspace(0, B - 1, sample).astype(np.int64)
    history = []
    g = torch.Generator(device=hip_backend.device).manual_seed(seed)
    stats = {"draws": 0, "near_tie_diff": 0}
    n = hip_backend.numpy
    for it in range(steps):
        logits = torch.randn(B, W, generator=g, device=hip_backend.device) * 2
        info = hip.step_logits(logits, seed=seed, autoreset=True)[4]
        act = n(info["action"]).astype(np.int32)
        host_logits = logits.cpu().numpy()
        if it in checks:
            start = P._state_snapshot(twin)
            own = twin.step_logits(host_logits, seed=seed, autoreset=True)[4]["action"].copy()
            P._restore(twin, start, start["solution"])
            live = own >= 0
            diff = np.flatnonzero(live & (own != act))
            ctx = context(twin)
            part = legal_entries(ctx["mask"], ctx["jobs"])
            _, _, gap = mirror(host_logits, part, 1.0, seed, ctx["env_ids"], ctx["episode"], ctx["step"])
            assert (gap[diff] <= NEAR_TIE).all(), f"{label} iter {it}: twin and HIP draw apart away from near-ties"
            stats["draws"] += int(live.sum())
            stats["near_tie_diff"] += diff.size
        twin.step(act, autoreset=True)
        history.append(act[pick].copy())
        if it in checks:
            a, b = P._state_snapshot(hip), P._state_snapshot(twin)
            for k in a:
                assert np.array_equal(a[k], b[k]), f"{label} iter {it}: {k} differs from the twin"
    assert stats["near_tie_diff"] <= 0.001 * stats["draws"], stats
    orcs = [OracleEnv(hip.instances[hip.instance_of_env(int(i))], strict=True) for i in pick]
    for o in orcs:
        o.reset()
    for acts in history:
        for o, a in zip(orcs, acts):
            if a == _abi.ACTION_RESET:
                o.reset()
            elif a != _abi.ACTION_SKIP:
                o.step(int(a))
    for o, i in zip(orcs, pick):
        P.assert_matches_oracle(hip.host_state(int(i)), o, f"{label} env {i}")


def ragged_by_shape():
    return [I.builtin_instance(n) for n in ("ta01", "ta31", "ta51", "ta71")]
