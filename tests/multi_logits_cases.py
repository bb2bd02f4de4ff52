"""Backend-agnostic cases of jss_multi_step_logits: BucketedJssEnv.step_logits and BatchedJssEnv.step_logits on a batch dealt out
by shape class, both one launch of the fused multi-set grid's kLogits bodies -- run against the host-core twin, the kernel
source under the SIMT emulator and the HIP library.  The draw itself is held to the NumPy mirror of logits_cases.py."""
import ctypes as C

import numpy as np

import logits_cases as L
import parity_cases as P
from jssenv_amd import BatchedJssEnv, _abi
from jssenv_amd import instances as I
from jssenv_amd.bucketed import BucketedJssEnv

TEMPERATURES = (1.0, 0.0, 0.5)


def ragged_population(seed=7):
    """every shape class, an instance that fills its lane group in each (J = 16, 32, 64: NOPE's entry behind the lanes; the
    first two reach states with NOPE legal within a few steps), one with more than 64 jobs, and a 3 x 2 instance whose episodes
    end within a few steps (autoreset)"""
    rng = np.random.default_rng(seed)
    return [P.random_instance(rng, j, m, max_dur=20) for j, m in ((3, 2), (16, 4), (32, 8), (40, 3), (64, 16), (70, 3))]


def as_logits(env, x, bf16=False):
    """host float32 logits -> (the tensor the env's backend takes, the float32 values it holds: bf16-rounded for bf16)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if bf16:
        t = t.to(torch.bfloat16)
    host = t.float().numpy()
    if hasattr(env.backend, "torch"):
        t = t.to(env.backend.device)
    return t, host


def step_logits_of(env, x, it, jobs=None):
    """logits for step `it`: normal, with NOPE made dominant on every other step in every other env, the even and the odd ones
    in turn (so that full lane groups fold NOPE in and take it, next to envs that take a job) -- and the schedule of
    temperatures and dtypes the cases cycle through"""
    x = x.copy()
    if it % 2 == 0:
        J = np.asarray(env.jobs_per_env if jobs is None else jobs)
        rows = np.arange((it // 2) % 2, len(J), 2)
        x[rows, J[rows]] = 60.0
    return x, TEMPERATURES[it % len(TEMPERATURES)], it % 3 == 2


def outputs(env):
    n = env.backend.numpy
    return n(env._lg_action).copy(), n(env._lg_logp).copy(), n(env._lg_entropy).copy()


def assert_same_state(a, b, what):
    sa, sb = P._state_snapshot(a), P._state_snapshot(b)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), f"{what}: {k}"


def call_ranges(env, t, T, seed, autoreset):
    """what BatchedJssEnv.step_logits launched on a by-shape batch before the fused grid had kLogits bodies: one single-set
    jss_step_logits per range of `env._ranges()` (below 64 jobs / the rest), each JssLogits at its range's first env"""
    be = env.backend
    flags = _abi.ROLLOUT_AUTORESET if autoreset else 0
    with be.on_device():
        arg = env._logits_arg(t)
        for d, s, o, a in env._ranges():
            lg = env._logits_struct(arg, T, True, True, a)
            assert be.lib.jss_step_logits(d, s, C.byref(lg), seed, flags, o, be.stream()) == 0
    be.sync()


# ---- (a) the bucketed grid against each bucket's own single-set call --------------------------------------------------
def case_bucketed_vs_buckets(backend, insts=None, batch=12, steps=12, seed=3, full_groups=True):
    """BucketedJssEnv.step_logits (one grid over the classes) and, on a twin object, every bucket's own
    BatchedJssEnv.step_logits: the same device function at the same group width, so action, logp, entropy and every state
    and output tensor are bit-identical; the draws and logp / entropy against the NumPy mirror"""
    insts = ragged_population() if insts is None else insts
    kw = dict(batch=batch, seed=seed, env_id_base=50, _backend=backend)
    grid, solo = BucketedJssEnv(insts, **kw), BucketedJssEnv(insts, **kw)
    assert grid._n_sets >= 2
    grid.reset()
    solo.reset()
    rng = np.random.default_rng(seed)
    stats, codes, nope_full = {}, set(), set()
    for it in range(steps):
        per, host, T, ctx = {}, {}, 0.0, {}
        for k, b in grid._each():
            x, T, bf16 = step_logits_of(b, L.random_logits(rng, b.batch, b.jmax + 1), it)
            per[k], host[k] = as_logits(b, x, bf16)
            ctx[k] = L.context(b)
        res = grid.step_logits(per, temperature=T, seed=seed + it, autoreset=True, entropy=True)
        assert set(res) == {k for k, _ in grid._each()}
        for k, b in solo._each():
            b.step_logits(per[k], temperature=T, seed=seed + it, autoreset=True, entropy=True)
        for k, b in grid._each():
            got, want = outputs(b), outputs(solo.buckets[k])
            for name, g, w in zip(("action", "logp", "entropy"), got, want):
                assert np.array_equal(g, w), f"iter {it} class {k}: {name} of the grid != the bucket's own call"
            assert np.array_equal(backend.numpy(res[k][4]["action"]), got[0])
            assert_same_state(b, solo.buckets[k], f"iter {it} class {k}")
            L.check_draw(ctx[k], host[k], got[0].astype(np.int64), got[1], got[2], T, seed + it, autoreset=True, stats=stats)
            codes |= set(got[0][got[0] < 0].tolist())
            J = np.asarray(b.jobs_per_env)
            nope_full |= set(J[(got[0] == J) & np.isin(J, (16, 32, 64))].tolist())
    assert _abi.ACTION_RESET in codes, "no env was reset: autoreset never reached the grid"
    if full_groups:
        assert {16, 32} <= nope_full, f"NOPE taken by full lane groups of J = {sorted(nope_full)} only"
    assert stats["near_tie_diff"] <= 0.001 * stats["draws"], stats
    return grid


# ---- (b) the by-shape batch: the grid against the per-range launches it replaces ----------------------------------------
def case_by_shape_vs_ranges(backend, insts=None, batch=12, steps=12, seed=5):
    """BatchedJssEnv(order='by_shape').step_logits (one grid) against, on a twin object, the per-range jss_step_logits launches
    it replaces: actions and every state and output tensor bit-identical; logp / entropy to float32 rounding (the grid reduces
    the small classes over 16- / 32-lane groups where the per-range launch uses a wavefront on the padded rows)"""
    insts = ragged_population() if insts is None else insts
    kw = dict(batch=batch, seed=seed, env_id_base=9, order="by_shape", _backend=backend)
    grid, ranged = BatchedJssEnv(insts, **kw), BatchedJssEnv(insts, **kw)
    assert grid._classes is not None and grid._classes["n"] >= 3
    grid.reset()
    ranged.reset()
    rng = np.random.default_rng(seed)
    stats = {}
    for it in range(steps):
        x, T, bf16 = step_logits_of(grid, L.random_logits(rng, batch, grid.jmax + 1), it)
        t, host = as_logits(grid, x, bf16)
        ctx = L.context(grid)
        grid.step_logits(t, temperature=T, seed=seed + it, autoreset=True, entropy=True)
        call_ranges(ranged, t, T, seed + it, True)
        (ga, gl, ge), (ra, rl, re_) = outputs(grid), outputs(ranged)
        assert np.array_equal(ga, ra), f"iter {it}: actions of the grid != the per-range launches"
        assert np.abs(gl - rl).max(initial=0) <= L.LOGP_TOL and np.abs(ge - re_).max(initial=0) <= L.LOGP_TOL, it
        assert np.array_equal(gl == -np.inf, rl == -np.inf)
        assert_same_state(grid, ranged, f"iter {it}")
        L.check_draw(ctx, host, ga.astype(np.int64), gl, ge, T, seed + it, autoreset=True, stats=stats)
    assert stats["near_tie_diff"] <= 0.001 * stats["draws"], stats
    return grid


# ---- (c) bucketed against padded -------------------------------------------------------------------------------------
def case_bucketed_vs_padded(backend, insts=None, n_envs=16, steps=30, seed=13):
    """BucketedJssEnv and BatchedJssEnv(order='interleaved') on the same instances, seed and per-env logits rows: both key the
    draw by the global env id, so they take the same actions at every step and hold the same env states"""
    insts = ragged_population() if insts is None else insts
    padded = BatchedJssEnv(insts, batch=n_envs, seed=seed, env_id_base=500, order="interleaved", _backend=backend)
    bucketed = BucketedJssEnv(insts, batch=n_envs, seed=seed, env_id_base=500, _backend=backend)
    padded.reset()
    bucketed.reset()
    rng = np.random.default_rng(seed)
    n = backend.numpy
    for it in range(steps):
        x, T, bf16 = step_logits_of(padded, L.random_logits(rng, n_envs, padded.jmax + 1), it)
        padded.step_logits(as_logits(padded, x, bf16)[0], temperature=T, seed=seed + it, autoreset=True, entropy=True)
        per = {k: as_logits(b, x[bucketed.members[k], :b.jmax + 1], bf16)[0] for k, b in bucketed._each()}
        bucketed.step_logits(per, temperature=T, seed=seed + it, autoreset=True, entropy=True)
        pa, pl, pe = outputs(padded)
        for k, b in bucketed._each():
            m = bucketed.members[k]
            ba, bl, be_ = outputs(b)
            assert np.array_equal(ba, pa[m]), f"iter {it} class {k}: bucketed and padded draw apart"
            assert np.abs(bl - pl[m]).max(initial=0) <= L.LOGP_TOL and np.abs(be_ - pe[m]).max(initial=0) <= L.LOGP_TOL
    padded.synchronize()
    bucketed.synchronize()
    for i in range(n_envs):
        a, b = padded.host_state(i), bucketed.host_state(i)
        assert a["clock"] == b["clock"] and a["episode"] == b["episode"] and (a["job_state"] == b["job_state"]).all(), f"env {i}"
        assert (a["solution"] == b["solution"]).all() and (a["mask"] == b["mask"]).all() and (a["tm"] == b["tm"]).all(), f"env {i}"
        assert np.abs(a["obs"] - b["obs"]).max() == 0, f"env {i}"
    assert padded.stats() == bucketed.stats()
    assert int(n(padded.env_header)[:, _abi.H_EPISODE].max()) > 1, "no episode ended"


# ---- (d) sets without a grid body, and argument errors ------------------------------------------------------------------
def case_fallback_and_errors(backend, steps=4, seed=4):
    """jss_multi_step_logits over sets the caller picked: sets that all have a body in the grid, and combinations that fall
    back to one plain launch per set (a shared-instance set, medium records on a one-wavefront-per-env shape, more than 6
    sets) -- each set's result that of its own jss_step_logits on a twin object; every argument error of the call"""
    be = backend
    D, S, O, LG = C.POINTER(_abi.JssDesc), C.POINTER(_abi.JssState), C.POINTER(_abi.JssOut), C.POINTER(_abi.JssLogits)
    groups = {"fused grid": [dict(instances=["ta01", "ta02", "ta03"], batch=9), dict(instances=["ta21", "ta31"], batch=5),
                             dict(instances=["ta51", "ta61"], batch=3, records="full"), dict(instances=["ta71", "ta52"], batch=4)],
              "shared instance": [dict(instances="ta01", batch=6), dict(instances=["ta11", "ta12"], batch=4)],
              "medium records, one wavefront per env": [dict(instances=["ta51", "ta61"], batch=3, records="medium"), dict(instances=["ta01", "ta02"], batch=5)],
              "seven sets": [dict(instances=["ta01", "ta02"], batch=3 + i % 3) for i in range(7)]}
    rng = np.random.default_rng(seed)
    for what, kws in groups.items():
        a = [BatchedJssEnv(seed=seed, env_id_base=100 * i, order="interleaved", _backend=be, **kw) for i, kw in enumerate(kws)]
        b = [BatchedJssEnv(seed=seed, env_id_base=100 * i, order="interleaved", _backend=be, **kw) for i, kw in enumerate(kws)]
        if what == "medium records, one wavefront per env":
            assert a[0].record_ints == _abi.NFM and a[0].jmax > 32
        n = len(a)
        sets = ((D * n)(*[C.pointer(e._desc) for e in a]), (S * n)(*[C.pointer(e._state) for e in a]), (O * n)(*[C.pointer(e._out) for e in a]))
        for e in a + b:
            e.reset()
        for it in range(steps):
            T = TEMPERATURES[it % len(TEMPERATURES)]
            ts = [as_logits(e, L.random_logits(rng, e.batch, e.jmax + 1), it % 2 == 1)[0] for e in a]
            with be.on_device():
                args = [e._logits_arg(t) for e, t in zip(a, ts)]
                lgs = [e._logits_struct(x, T, True, True) for e, x in zip(a, args)]
                assert be.lib.jss_multi_step_logits(n, sets[0], sets[1], (LG * n)(*[C.pointer(x) for x in lgs]), seed + it,
                                                    _abi.ROLLOUT_AUTORESET, sets[2], be.stream()) == 0
            for e, t in zip(b, ts):
                e.step_logits(t, temperature=T, seed=seed + it, autoreset=True, entropy=True)
            for i, (x, y) in enumerate(zip(a, b)):
                (xa, xl, xe), (ya, yl, ye) = outputs(x), outputs(y)
                assert np.array_equal(xa, ya), f"{what}, set {i}, iter {it}: actions"
                if what == "fused grid":        # (the grid's two-jobs-per-lane body has no narrow path for ta52's 50 jobs)
                    assert np.abs(xl - yl).max() <= L.LOGP_TOL and np.abs(xe - ye).max() <= L.LOGP_TOL
                else:                           # the very same plain launch
                    assert np.array_equal(xl, yl) and np.array_equal(xe, ye), f"{what}, set {i}, iter {it}: logp / entropy"
                assert_same_state(x, y, f"jss_multi_step_logits ({what}), set {i}, iter {it}")
    # argument errors (the last group, seven sets): nothing is stepped
    before = [P._state_snapshot(e) for e in a]
    with be.on_device():
        args = [e._logits_arg(as_logits(e, np.zeros((e.batch, e.jmax + 1), np.float32))[0]) for e in a]

        def rc(k=0, lgs=True, n_sets=None, descs=True, **over):
            ls = [e._logits_struct(x, 1.0, True, True) for e, x in zip(a, args)]
            for f, v in over.items():
                setattr(ls[k], f, v)
            arr = (LG * n)(*[C.pointer(x) for x in ls])
            if lgs == "null entry":
                arr[k] = LG()
            r = be.lib.jss_multi_step_logits(n if n_sets is None else n_sets, sets[0] if descs else None, sets[1],
                                             arr if lgs else None, 1, 0, sets[2], be.stream())
            be.sync()
            return r
        assert rc(n_sets=0) == _abi.E_SHAPE and rc(n_sets=17) == _abi.E_SHAPE
        assert rc(descs=False) == _abi.E_NULL and rc(lgs=False) == _abi.E_NULL and rc(k=3, lgs="null entry") == _abi.E_NULL
        assert rc(k=2, logits=None) == _abi.E_NULL and rc(k=5, action=None) == _abi.E_NULL
        assert rc(k=1, row=a[1].jmax) == _abi.E_SHAPE and rc(k=6, row=(1 << 24) + 1) == _abi.E_SHAPE
        assert rc(k=4, dtype=2) == _abi.E_KIND and rc(k=0, temperature=-1.0) == _abi.E_KIND
        assert rc(k=6, temperature=float("nan")) == _abi.E_KIND
    for e, snap in zip(a, before):
        now = P._state_snapshot(e)
        assert all(np.array_equal(now[k], snap[k]) for k in snap), "a refused call stepped a set"


# ---- (e) the edge cases of the draw, through the grid -------------------------------------------------------------------
def case_edges_through_grid(backend, insts=None, batch=12, steps=16, seed=11):
    """a by-shape batch and a BucketedJssEnv over a ragged population with full lane groups (J = 16, 32, 64): autoreset
    (-2, logp 0, entropy 0), T = 0 (greedy), bf16 logits and NOPE taken where it is folded in after the reduction -- every
    draw against the mirror, the state against step(action)"""
    insts = ragged_population() if insts is None else insts
    env = BatchedJssEnv(insts, batch=batch, seed=seed, env_id_base=3, order="by_shape", _backend=backend)
    env.reset()
    rng = np.random.default_rng(seed)
    J = np.asarray(env.jobs_per_env)
    stats, codes, nope_full, greedy = {}, set(), set(), 0
    for it in range(steps):
        x, T, bf16 = step_logits_of(env, L.random_logits(rng, batch, env.jmax + 1), it)
        t, host = as_logits(env, x, bf16)
        ctx, act, logp, ent = L.step_and_check(env, t, T, seed + it, autoreset=True)
        L.check_draw(ctx, host, act, logp, ent, T, seed + it, autoreset=True, stats=stats)
        if T == 0:
            part = L.legal_entries(ctx["mask"], ctx["jobs"])
            live = np.flatnonzero((act >= 0))
            assert np.array_equal(act[live], np.argmax(np.where(part, host, -np.inf), axis=1)[live]), f"iter {it}: greedy"
            greedy += live.size
        codes |= set(act[act < 0].tolist())
        nope_full |= set(J[(act == J) & np.isin(J, (16, 32, 64))].tolist())
    assert _abi.ACTION_RESET in codes and greedy > 0
    assert {16, 32} <= nope_full, f"NOPE taken by full lane groups of J = {sorted(nope_full)} only"   # (64 x 16: late, if at all)
    assert stats["near_tie_diff"] <= 0.001 * stats["draws"], stats


# ---- (g) full size on the MI355X ---------------------------------------------------------------------------------------
def case_config5_full_size(hip_backend, batch=32768, steps=50, seed=29, sample=512):
    """BASELINE config 5 dealt out by shape (ta01-ta80 x 32 768), 215 random steps in, then step_logits through the grid with
    autoreset at T = 1: every
    env's state equals a clone stepped with step(info["action"]) (checked along the way and at the end); on a sample spread over
    every class the draws against the mirror and logp / entropy against float64 -- and the BucketedJssEnv of the same population
    against each bucket's own single-set call"""
    torch = hip_backend.torch
    insts = [I.builtin_instance(f"ta{k:02d}") for k in range(1, 81)]
    kw = dict(instances=insts, batch=batch, seed=seed, env_id_base=11, order="by_shape", _backend=hip_backend)
    env, clone = BatchedJssEnv(**kw), BatchedJssEnv(**kw)
    assert env._classes is not None and env._classes["n"] == 4
    env.reset()
    clone.reset()
    for e in (env, clone):           # to near the end of the 15 x 15 episodes: envs finish, and are reset, within the steps
        e.rollout("random", n_iter=215)
    B, W = env.batch, env.jmax + 1
    pick = np.linspace(0, B - 1, sample).astype(np.int64)
    g = torch.Generator(device=hip_backend.device).manual_seed(seed)
    n = hip_backend.numpy
    stats, resets = {"draws": 0, "near_tie_diff": 0}, 0
    for it in range(steps):
        logits = torch.randn(B, W, generator=g, device=hip_backend.device) * 2
        ctx = {k: v[pick] for k, v in L.context(env).items()}
        info = env.step_logits(logits, seed=seed, autoreset=True, entropy=True)[4]
        act = n(info["action"]).astype(np.int32)
        resets += int((act == _abi.ACTION_RESET).sum())
        L.check_draw(ctx, logits.cpu().numpy()[pick], act[pick].astype(np.int64), n(info["logp"])[pick], n(info["entropy"])[pick],
                     1.0, seed, autoreset=True, stats=stats)
        clone.step(act, autoreset=True)
        if it in (0, steps // 2, steps - 1):
            assert_same_state(env, clone, f"config 5 x {B} iter {it}")
    assert stats["near_tie_diff"] <= 0.001 * stats["draws"], stats
    assert resets > 0, "no episode ended: autoreset not exercised"
    del env, clone
    grid, solo = (BucketedJssEnv(insts, batch=batch, seed=seed, env_id_base=11, _backend=hip_backend) for _ in range(2))
    grid.reset()
    solo.reset()
    for it in range(steps // 5):
        per = {k: torch.randn(b.batch, b.jmax + 1, generator=g, device=hip_backend.device) * 2 for k, b in grid._each()}
        grid.step_logits(per, seed=seed + it, autoreset=True, entropy=True)
        for k, b in solo._each():
            b.step_logits(per[k], seed=seed + it, autoreset=True, entropy=True)
        for k, b in grid._each():
            for name, x, y in zip(("action", "logp", "entropy"), outputs(b), outputs(solo.buckets[k])):
                assert np.array_equal(x, y), f"bucketed config 5 iter {it} class {k}: {name}"
    for k, b in grid._each():
        assert_same_state(b, solo.buckets[k], f"bucketed config 5 class {k}")
