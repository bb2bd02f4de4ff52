"""One fixed list of calls of BatchedJssEnv's fourteen search methods, of the refusals of the wrapper classes and of the
argument errors of the drivers in jssenv_amd.search, for tests/test_search_calls.py: every argument form a method accepts, every
optional output, one call per ``raise``.  ``run(backend)`` makes the calls and returns ``{name: record}`` -- of a call that
returns, the shape, dtype and SHA-256 of every returned array; of a call that raises, the exception's class and its message.
The integer arrays of a call go in as lists and as NumPy arrays, and on a backend with torch as int32 and int64 device tensors
too: every form must give the same record.

The batch: four envs over a 6 x 6 and a 3 x 4 instance (so jmax = mmax = 6 and every padding branch is live), reset and played to
the end with SPT; ``lookahead`` and ``lower_bound`` read a second batch of the same make, a few SPT steps into its episodes."""
import dataclasses
import hashlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE)]

from jssenv_amd import BatchedJssEnv, BucketedJssEnv, JssVectorEnv, search  # noqa: E402
from jssenv_amd.instances import PackedBatch, pack_batch, taillard_instance  # noqa: E402

B, J, M = 4, 6, 6
A = J + 1
REFUSED = ("evaluate_order", "tabu", "tabu_blocks", "relink", "order_distance", "decode_keys", "evolve_keys", "relax_machines",
           "bottleneck", "solve_machines", "bottleneck_exact", "propagate")

_TWIN = []


def twin_backend():
    if not _TWIN:
        from jssenv_amd.env import CpuBackend
        _TWIN.append(CpuBackend())
    return _TWIN[0]


def instances():
    return [taillard_instance(6, 6, 21, 22), taillard_instance(3, 4, 11, 12)]


def batch(be, played=True):
    env = BatchedJssEnv(instances(), batch=B, table_of_env=[0, 1, 0, 1], order="interleaved", seed=1, _backend=be)
    env.reset()
    env.rollout("SPT", n_iter=3 * J * M if played else 5, autoreset=False)
    return env


# ---- the forms an integer array goes in as -------------------------------------------------------------------------------------
def forms(be):
    """name -> the function that gives an integer (or boolean) array to a call"""
    def as_list(x, dtype=None):
        return np.asarray(x).tolist()

    def as_numpy(x, dtype=None):
        return np.array(x, dtype=dtype if dtype is not None else (np.bool_ if np.asarray(x).dtype == np.bool_ else np.int32))

    out = {"list": as_list, "numpy": as_numpy}
    t = getattr(be, "torch", None)
    if t is not None:
        def tensor(width):
            def as_tensor(x, dtype=None):
                a = np.asarray(x)
                return t.as_tensor(a, device=be.device) if a.dtype == np.bool_ else \
                    t.as_tensor(a.astype(np.int64), device=be.device).to(width)
            return as_tensor
        out["int32 tensor"], out["int64 tensor"] = tensor(t.int32), tensor(t.int64)
    return out


# ---- the calls ---------------------------------------------------------------------------------------------------------------------
class Setup:
    """the batches of a backend and the host arrays the calls are made of"""

    def __init__(self, be):
        self.be = be
        self.env, self.early = batch(be), batch(be, played=False)
        self.never = BatchedJssEnv(instances(), batch=B, table_of_env=[0, 1, 0, 1], order="interleaved", seed=1, _backend=be)
        self.busy = batch(be)
        self.busy._session = types.SimpleNamespace(closed=False)          # (what an open StepSession looks like to the guards)
        host = lambda x: np.asarray(be.numpy(x))   # noqa: E731
        self.sol = host(self.env.solution).astype(np.int32).copy()
        assert host(self.env.done).all() and host(self.env.makespan).tolist() == [521, 235, 521, 235]
        rng = np.random.default_rng(7)
        self.keys2 = rng.integers(0, 1000, (J, M)).astype(np.int32)
        self.keys3 = rng.integers(0, 1000, (5, J, M)).astype(np.int32)
        self.keys4 = rng.integers(0, 1000, (B, J, M)).astype(np.int32)
        self.guide = host(self.env.decode_keys(self.keys4, start=True)[1]).astype(np.int32).copy()
        self.pop = rng.integers(0, 1 << 20, (2 * 4, J, M)).astype(np.int32)
        self.fit = rng.integers(100, 900, (2 * 4,)).astype(np.int32)
        self.bias = rng.integers(0, 50, (5, M)).astype(np.int32)
        # windows to start a propagation from: those of the empty selection under a generous makespan
        out = self.env.propagate(2000, windows=True)
        self.est, self.lct = (host(x).astype(np.int32).copy() for x in out[2:])


PAR5 = [0, 1, 2, 3, 1]            # five candidates over the four envs
ALL = (1 << M) - 1


def valid_calls():
    """(name, f(s, F)): s the Setup, F the form of the integer arrays"""
    c = []

    def add(name, f):
        c.append((name, f))

    # lookahead / lower_bound: the batch a few steps in
    add("lookahead()", lambda s, F: s.early.lookahead("SPT"))
    add("lookahead(MWR, seed, explore)", lambda s, F: s.early.lookahead("MWR", seed=5, explore=0.25, id_base=3, n_iter=40))
    add("lookahead(parents, actions)", lambda s, F: s.early.lookahead("SPT", F([0, 1, 5, 6, 2, -1, 7]), F([0, 1, 2, 3, 1, 0, 9])))
    add("lookahead(n=0)", lambda s, F: s.early.lookahead("SPT", F([]), F([])))
    add("lookahead(done)", lambda s, F: s.env.lookahead("SPT"))
    add("lower_bound()", lambda s, F: s.early.lower_bound())
    add("lower_bound(all)", lambda s, F: s.early.lower_bound("all"))
    add("lower_bound(all, outputs)", lambda s, F: s.early.lower_bound("all", job_bound=True, est_start=True))
    add("lower_bound(parents, actions)", lambda s, F: s.early.lower_bound(F([0, 1, 5, 6, 2, -1, 7]), F([0, 1, 2, 3, 1, 0, 9]), job_bound=True))
    add("lower_bound(illegal too)", lambda s, F: s.early.lower_bound(F([0, 1, 5, 6, 2, -1]), F([0, 1, 2, 3, 1, 0]), legal_only=False, est_start=True))
    add("lower_bound(n=0)", lambda s, F: s.early.lower_bound(F([]), F([]), job_bound=True, est_start=True))
    add("lower_bound(done)", lambda s, F: s.env.lower_bound(est_start=True))
    # evaluate_order
    add("evaluate_order()", lambda s, F: s.env.evaluate_order())
    add("evaluate_order(unfinished)", lambda s, F: s.early.evaluate_order())
    add("evaluate_order(rank, outputs)", lambda s, F: s.env.evaluate_order(F(s.guide), start=True, tail=True, pairs=3))
    add("evaluate_order(parents)", lambda s, F: s.env.evaluate_order(None, F(PAR5 + [4, -1]), start=True))
    add("evaluate_order(swaps pair)", lambda s, F: s.env.evaluate_order(F(s.sol), F(PAR5), (F([0, 1, -1, 2, 40]), F([6, 7, -1, 3, 1])), tail=True))
    add("evaluate_order(swaps n x 2)", lambda s, F: s.env.evaluate_order(None, None, F([[0, 6], [1, 7], [-1, -1], [2, 3]]), pairs=8))
    add("evaluate_order(n=0)", lambda s, F: s.env.evaluate_order(None, F([]), start=True, tail=True, pairs=2))
    # tabu / tabu_blocks
    for name, walk in (("tabu", lambda e: e.tabu), ("tabu_blocks", lambda e: e.tabu_blocks)):
        add(f"{name}()", lambda s, F, walk=walk: walk(s.env)(None, 20, 3))
        add(f"{name}(rank, per env)", lambda s, F, walk=walk: walk(s.env)(F(s.guide), 12, F([0, 2, 5, 64]), F([480, 235, 1, 400]), trace=True, last=True))
        add(f"{name}(target)", lambda s, F, walk=walk: walk(s.env)(None, 30, 4, 470, trace=True))
        add(f"{name}(iters=0)", lambda s, F, walk=walk: walk(s.env)(None, 0, 0, None, trace=True, last=True))
        add(f"{name}(tenure refused)", lambda s, F, walk=walk: walk(s.env)(None, 5, F([1, 65, -1, 2])))
    add("tabu_blocks(reach, log)", lambda s, F: s.env.tabu_blocks(F(s.guide), 15, 2, None, 1, True, True, True))
    # relink / order_distance
    add("relink()", lambda s, F: s.env.relink(None, F(s.guide)))
    add("relink(steps, per env)", lambda s, F: s.env.relink(F(s.guide), F(s.sol), 6, F([0, 1, 2, 100]), margin=1, trace=True, log=True))
    add("relink(until)", lambda s, F: s.env.relink(F(s.sol), F(s.guide), None, 3, last=False, trace=False))
    add("relink(steps=0)", lambda s, F: s.env.relink(None, F(s.guide), 0, 0, trace=True, log=True))
    add("order_distance()", lambda s, F: s.env.order_distance(F(s.sol), F(s.guide)))
    add("order_distance(None)", lambda s, F: s.env.order_distance(None, F(s.sol)))
    # decode_keys / evolve_keys
    add("decode_keys(one table)", lambda s, F: s.env.decode_keys(F(s.keys2)))
    add("decode_keys(tables, outputs)", lambda s, F: s.env.decode_keys(F(s.keys4), None, 0.5, start=True, info=True))
    add("decode_keys(parents)", lambda s, F: s.env.decode_keys(F(s.keys3), F(PAR5), 0.0, info=True))
    add("decode_keys(one table, parents)", lambda s, F: s.env.decode_keys(F(s.keys2), F(PAR5 + [4, -1]), 1.0, start=True))
    add("decode_keys(delta list)", lambda s, F: s.env.decode_keys(F(s.keys3), F(PAR5), [0.0, 0.25, 0.5, 0.75, 1.0], start=True))
    add("decode_keys(delta array)", lambda s, F: s.env.decode_keys(F(s.keys4), None, np.array([1.0, 0.0, 0.3, 0.9]), start=True))
    add("decode_keys(n=0)", lambda s, F: s.env.decode_keys(F(s.keys2), F([]), start=True, info=True))
    add("evolve_keys(fresh, shape)", lambda s, F: s.env.evolve_keys((8, J, M), None, 4, 0, 4, generation=0))
    add("evolve_keys(fresh, array)", lambda s, F: s.env.evolve_keys(F(s.pop), None, 4, 0, 4, generation=0, seed=9))
    add("evolve_keys()", lambda s, F: s.env.evolve_keys(F(s.pop), F(s.fit), 4, 1, 1, 0.6, 3, seed=11))
    add("evolve_keys(flat rows)", lambda s, F: s.env.evolve_keys(F(s.pop.reshape(8, J * M)), F(s.fit), 8, 2, 0))
    add("evolve_keys(G=0)", lambda s, F: s.env.evolve_keys(np.zeros((0, J, M), np.int32), F([]), 4, 1, 1))
    # relax_machines / solve_machines
    for name, call, more in (("relax_machines", lambda e: e.relax_machines, dict(jps=True, schrage=True)),
                             ("solve_machines", lambda e: e.solve_machines, dict(opt=True, low=True, nodes_used=True, proved=True, nodes=64))):
        rest = dict(more, head=True, tail=True, rank_out=True)
        add(f"{name}()", lambda s, F, call=call: call(s.env)())
        add(f"{name}(outputs)", lambda s, F, call=call, rest=rest: call(s.env)(**rest))
        add(f"{name}(one table, mask)", lambda s, F, call=call, rest=rest: call(s.env)(F(s.sol[0]), 0b000101, **rest))
        add(f"{name}(tables, masks)", lambda s, F, call=call, rest=rest: call(s.env)(F(s.sol), F([1, 3, ALL, 0]), **rest))
        add(f"{name}(int64 masks)", lambda s, F, call=call: call(s.env)(F(s.guide), np.array([1, 2, 4, 8], np.int64), head=True))
        add(f"{name}(uint64 masks)", lambda s, F, call=call: call(s.env)(F(s.guide), np.array([1, 2, 4, 1 << 63], np.uint64)))
        add(f"{name}(boolean matrix)", lambda s, F, call=call: call(s.env)(F(s.sol), F(np.arange(B * M).reshape(B, M) % 3 == 0), rank_out=True))
        add(f"{name}(parents)", lambda s, F, call=call, rest=rest: call(s.env)(F(s.sol[[0, 1, 2, 3, 1]]), F([1, 2, 0, ALL, 5]), F(PAR5), **rest))
        add(f"{name}(parents out of range)", lambda s, F, call=call: call(s.env)(None, 0, F([0, 4, -1, 1])))
        add(f"{name}(n from fixed)", lambda s, F, call=call: call(s.env)(F(s.sol[0]), F([1, 2, 3, 4, 5]), F(PAR5)))
        add(f"{name}(n=0)", lambda s, F, call=call, rest=rest: call(s.env)(None, 0, F([]), **rest))
    add("solve_machines(nodes=1)", lambda s, F: s.env.solve_machines(nodes=1, opt=True, low=True, proved=True))
    # bottleneck / bottleneck_exact
    for name, call, more in (("bottleneck", lambda e: e.bottleneck, {}), ("bottleneck_exact", lambda e: e.bottleneck_exact, dict(nodes=32))):
        add(f"{name}()", lambda s, F, call=call: call(s.env)())
        add(f"{name}(parents, bias)", lambda s, F, call=call, more=more: call(s.env)(F(PAR5), F(s.bias), 2, order=True, **more))
        add(f"{name}(bias)", lambda s, F, call=call, more=more: call(s.env)(None, F(s.bias[:B]), 0, **more))
        add(f"{name}(from a selection)", lambda s, F, call=call, more=more: call(s.env)(None, None, 1, rank=F(s.sol), fixed=F([1, 3, 0, ALL]), order=True, **more))
        add(f"{name}(from a selection, parents)", lambda s, F, call=call, more=more: call(s.env)(F(PAR5), F(s.bias), 1, rank=F(s.sol[[0, 1, 2, 3, 1]]), fixed=5, **more))
        add(f"{name}(n=0)", lambda s, F, call=call, more=more: call(s.env)(F([]), None, 1, order=True, **more))
    # propagate
    add("propagate(ub)", lambda s, F: s.env.propagate(600))
    add("propagate(tight ub, windows)", lambda s, F: s.env.propagate(300, windows=True))
    add("propagate(ub per env)", lambda s, F: s.env.propagate(F([501, 235, 400, 200]), windows=True, passes=3))
    add("propagate(selection)", lambda s, F: s.env.propagate(F([501, 235, 520, 234]), F(s.sol), F([ALL, ALL, 3, ALL]), windows=True))
    add("propagate(one table, mask)", lambda s, F: s.env.propagate(700, F(s.sol[0]), 0b11, windows=True))
    add("propagate(boolean matrix)", lambda s, F: s.env.propagate(700, F(s.sol), F(np.arange(B * M).reshape(B, M) % 2 == 0), windows=True))
    add("propagate(parents)", lambda s, F: s.env.propagate(F([600, 300, 600, 300, 250]), None, 0, F(PAR5), windows=True))
    add("propagate(windows in, one table)", lambda s, F: s.env.propagate(2000, est=F(s.est[0]), lct=F(s.lct[0]), windows=True))
    add("propagate(windows in, tables)", lambda s, F: s.env.propagate(F([600, 300, 550, 280]), est=F(s.est), lct=F(s.lct), windows=True))
    add("propagate(hyp)", lambda s, F: s.env.propagate(F([600, 300, 600, 300]), hyp=(F([0, 1, -1, 7]), F([50, 0, 0, 100]), F([600, 40, 0, 300])), windows=True))
    add("propagate(hyp, everything)", lambda s, F: s.env.propagate(
        F([600, 300, 600, 300, 300]), F(s.sol[[0, 1, 2, 3, 1]]), F([1, 2, 4, 8, 0]), F(PAR5), F(s.est[[0, 1, 2, 3, 1]]), F(s.lct[[0, 1, 2, 3, 1]]),
        (F([0, 1, -1, 7, 2]), F([50, 0, 0, 100, 10]), F([600, 40, 0, 300, 250])), 64, True))
    add("propagate(n=0)", lambda s, F: s.env.propagate(np.zeros(0, np.int32), parents=F([]), windows=True))
    return c


def bad_calls():
    """(name, f(s)): one call per raise of the fourteen methods"""
    c = []

    def add(name, f):
        c.append((name, f))

    wrong = np.zeros((B, J, M + 1), np.int32)
    for name in ("lookahead", "lower_bound", "evaluate_order", "tabu", "tabu_blocks", "decode_keys", "relax_machines", "bottleneck",
                 "solve_machines", "bottleneck_exact"):
        args = (np.zeros((J, M), np.int32),) if name == "decode_keys" else ()
        add(f"{name}: never reset", lambda s, name=name, args=args: getattr(s.never, name)(*args))
        add(f"{name}: open session", lambda s, name=name, args=args: getattr(s.busy, name)(*args))
    for name in ("relink", "order_distance"):
        add(f"{name}: never reset", lambda s, name=name: getattr(s.never, name)(None, s.guide))
        add(f"{name}: open session", lambda s, name=name: getattr(s.busy, name)(None, s.guide))
    add("propagate: never reset", lambda s: s.never.propagate(600))
    add("propagate: open session", lambda s: s.busy.propagate(600))
    # what fires before those guards today stays in front of them
    add("relax_machines: rank shape before never reset", lambda s: s.never.relax_machines(wrong))
    add("bottleneck: reopt before never reset", lambda s: s.never.bottleneck(reopt=9))
    add("propagate: passes before open session", lambda s: s.busy.propagate(600, passes=0))
    add("tabu: never reset before iters", lambda s: s.never.tabu(None, -1))
    add("evolve_keys: runs never reset", lambda s: s.never.evolve_keys((8, J, M), None, 4, 0, 4, generation=0))

    add("lookahead: parents alone", lambda s: s.early.lookahead("SPT", None, [0]))
    add("lookahead: unequal", lambda s: s.early.lookahead("SPT", [0, 1], [0, 1, 2]))
    add("lookahead: 2-d", lambda s: s.early.lookahead("SPT", [[0, 1]], [[0, 1]]))
    add("lower_bound: a word", lambda s: s.early.lower_bound("every"))
    add("lower_bound: all with parents", lambda s: s.early.lower_bound("all", [0]))
    add("lower_bound: actions alone", lambda s: s.early.lower_bound([0]))
    add("lower_bound: unequal", lambda s: s.early.lower_bound([0, 1], [0]))
    add("evaluate_order: pairs", lambda s: s.env.evaluate_order(pairs=0))
    add("evaluate_order: rank shape", lambda s: s.env.evaluate_order(wrong))
    add("evaluate_order: parents 2-d", lambda s: s.env.evaluate_order(None, [[0, 1]]))
    add("evaluate_order: swaps shape", lambda s: s.env.evaluate_order(None, None, np.zeros((B, 3), np.int32)))
    add("evaluate_order: swaps count", lambda s: s.env.evaluate_order(None, [0, 1, 2], ([0, 1], [6, 7])))
    for name in ("tabu", "tabu_blocks"):
        add(f"{name}: iters", lambda s, name=name: getattr(s.env, name)(None, 65537))
        add(f"{name}: rank shape", lambda s, name=name: getattr(s.env, name)(wrong))
        add(f"{name}: tenure shape", lambda s, name=name: getattr(s.env, name)(None, 5, [1, 2, 3]))
        add(f"{name}: tenure", lambda s, name=name: getattr(s.env, name)(None, 5, 65))
        add(f"{name}: target shape", lambda s, name=name: getattr(s.env, name)(None, 5, 3, [1, 2, 3, 4, 5]))
    add("tabu_blocks: reach", lambda s: s.env.tabu_blocks(None, 5, 3, None, -1))
    add("tabu_blocks: iters before reach", lambda s: s.env.tabu_blocks(None, -1, 3, None, -1))
    add("relink: steps", lambda s: s.env.relink(None, s.guide, 65537))
    add("relink: margin", lambda s: s.env.relink(None, s.guide, margin=-1))
    add("relink: no guide", lambda s: s.env.relink(None, None))
    add("relink: rank shape", lambda s: s.env.relink(wrong, s.guide))
    add("relink: guide shape", lambda s: s.env.relink(None, wrong))
    add("relink: until", lambda s: s.env.relink(None, s.guide, until=-1))
    add("relink: until shape", lambda s: s.env.relink(None, s.guide, until=[1, 2, 3]))
    add("order_distance: guide shape", lambda s: s.env.order_distance(None, wrong))
    add("decode_keys: keys shape", lambda s: s.env.decode_keys(wrong))
    add("decode_keys: parents 2-d", lambda s: s.env.decode_keys(s.keys2, [[0, 1]]))
    add("decode_keys: table count", lambda s: s.env.decode_keys(s.keys3, [0, 1]))
    add("decode_keys: one per env", lambda s: s.env.decode_keys(s.keys3))
    add("decode_keys: delta", lambda s: s.env.decode_keys(s.keys2, None, 1.5))
    add("decode_keys: delta shape", lambda s: s.env.decode_keys(s.keys2, None, [0.5, 0.5]))
    add("decode_keys: delta entries", lambda s: s.env.decode_keys(s.keys2, None, [0.5, 0.5, -0.1, 1.0]))
    add("evolve_keys: rho", lambda s: s.env.evolve_keys(s.pop, s.fit, 4, 1, 1, 1.5))
    add("evolve_keys: pop", lambda s: s.env.evolve_keys(s.pop, s.fit, 0, 0, 0))
    add("evolve_keys: elite and mutants", lambda s: s.env.evolve_keys(s.pop, s.fit, 4, 0, 2))
    add("evolve_keys: keys shape", lambda s: s.env.evolve_keys(s.pop, s.fit, 3, 1, 1))
    add("evolve_keys: keys 1-d", lambda s: s.env.evolve_keys(s.fit, s.fit, 4, 1, 1))
    add("evolve_keys: no fitness", lambda s: s.env.evolve_keys(s.pop, None, 4, 1, 1))
    add("evolve_keys: fitness shape", lambda s: s.env.evolve_keys(s.pop, s.fit[:4], 4, 1, 1))
    for name in ("relax_machines", "solve_machines", "propagate"):
        head = (600,) if name == "propagate" else ()
        call = lambda s, *a, name=name, head=head, **k: getattr(s.env, name)(*head, *a, **k)   # noqa: E731
        add(f"{name}: rank shape", lambda s, call=call: call(s, wrong))
        add(f"{name}: parents 2-d", lambda s, call=call: call(s, None, 0, [[0, 1]]))
        add(f"{name}: one per env", lambda s, call=call: call(s, s.sol[:3], 1))
        add(f"{name}: table count", lambda s, call=call: call(s, s.sol, 1, [0, 1]))
        add(f"{name}: mask range", lambda s, call=call: call(s, s.sol, -1))
        add(f"{name}: mask too wide", lambda s, call=call: call(s, s.sol, 2 ** 64))
        add(f"{name}: boolean shape", lambda s, call=call: call(s, s.sol, np.zeros((3, M), bool), [0, 1, 2, 3]))
        add(f"{name}: boolean width", lambda s, call=call: call(s, s.sol, np.zeros((B, 65), bool)))
        add(f"{name}: float masks", lambda s, call=call: call(s, s.sol, np.zeros(B)))
        add(f"{name}: masks shape", lambda s, call=call: call(s, s.sol, np.zeros((B, 2), np.int32)))
        add(f"{name}: negative masks", lambda s, call=call: call(s, s.sol, np.array([1, -1, 0, 0], np.int32)))
        add(f"{name}: fixed without rank", lambda s, call=call: call(s, None, 1))
    add("solve_machines: nodes", lambda s: s.env.solve_machines(nodes=0))
    add("solve_machines: nodes above", lambda s: s.env.solve_machines(nodes=4097))
    for name in ("bottleneck", "bottleneck_exact"):
        call = lambda s, *a, name=name, **k: getattr(s.env, name)(*a, **k)   # noqa: E731
        add(f"{name}: reopt", lambda s, call=call: call(s, reopt=-1))
        add(f"{name}: rank alone", lambda s, call=call: call(s, rank=s.sol))
        add(f"{name}: fixed alone", lambda s, call=call: call(s, fixed=1))
        add(f"{name}: rank shape", lambda s, call=call: call(s, rank=s.sol[0], fixed=1))
        add(f"{name}: parents 2-d", lambda s, call=call: call(s, [[0, 1]]))
        add(f"{name}: one per env", lambda s, call=call: call(s, rank=s.sol[:3], fixed=1))
        add(f"{name}: table count", lambda s, call=call: call(s, [0, 1], rank=s.sol, fixed=1))
        add(f"{name}: mask range", lambda s, call=call: call(s, rank=s.sol, fixed=-1))
        add(f"{name}: masks shape", lambda s, call=call: call(s, [0, 1, 2, 3], rank=s.sol, fixed=[1, 2, 3]))
        add(f"{name}: bias shape", lambda s, call=call: call(s, None, s.bias))
    add("bottleneck_exact: nodes", lambda s: s.env.bottleneck_exact(nodes=0))
    add("bottleneck_exact: reopt before nodes", lambda s: s.env.bottleneck_exact(reopt=9, nodes=0))
    add("propagate: passes", lambda s: s.env.propagate(600, passes=4097))
    add("propagate: est alone", lambda s: s.env.propagate(600, est=s.est))
    add("propagate: hyp length", lambda s: s.env.propagate(600, hyp=([0] * B, [0] * B)))
    add("propagate: est shape", lambda s: s.env.propagate(600, est=wrong, lct=s.lct))
    add("propagate: lct shape", lambda s: s.env.propagate(600, est=s.est, lct=wrong))
    add("propagate: est and lct differ", lambda s: s.env.propagate(600, est=s.est, lct=s.lct[0]))
    add("propagate: counts", lambda s: s.env.propagate([600, 600, 600], est=s.est, lct=s.lct))
    add("propagate: hyp count", lambda s: s.env.propagate(600, hyp=([0] * 3, [0] * 3, [9] * 3)))
    add("propagate: ub floats", lambda s: s.env.propagate(np.full(B, 600.0)))
    add("propagate: ub 2-d", lambda s: s.env.propagate(np.full((B, 1), 600)))
    add("propagate: ub width", lambda s: s.env.propagate([600, 600, 600, 2 ** 31]))
    add("propagate: hyp rows", lambda s: s.env.propagate(600, hyp=([0] * B, [0.5] * B, [9] * B)))
    add("propagate: hyp row shape", lambda s: s.env.propagate(600, hyp=([0] * B, [0] * 3, [9] * B)))
    return c


def refusal_calls():
    c = []
    for cls in (BucketedJssEnv, JssVectorEnv):
        for name in REFUSED:
            c.append((f"{cls.__name__}.{name}", lambda s, cls=cls, name=name: getattr(object.__new__(cls), name)(None, 1, x=2)))
    return c


def driver_calls():
    """(name, f(s)): the drivers' argument errors, and one small run of each driver for every way it finds its target"""
    c = []

    def add(name, f):
        c.append((name, f))

    S = search
    two = instances()
    packed = pack_batch(two)
    assert isinstance(packed, PackedBatch)
    for name, f in (("tabu_search", S.tabu_search), ("relink_search", S.relink_search), ("brkga_search", S.brkga_search),
                    ("bottleneck_search", S.bottleneck_search), ("beam_search", S.beam_search), ("destructive_bound", S.destructive_bound)):
        add(f"{name}: a packed batch", lambda s, f=f: f(packed, _backend=s.be))
        add(f"{name}: a batch", lambda s, f=f: f(s.env, _backend=s.be))
        if name != "beam_search":
            add(f"{name}: a wrapper", lambda s, f=f: f(object.__new__(JssVectorEnv), _backend=s.be))
            add(f"{name}: a bucketed batch", lambda s, f=f: f(object.__new__(BucketedJssEnv), _backend=s.be))
        add(f"{name}: no instance", lambda s, f=f: f([], _backend=s.be))
    add("improve: a packed batch", lambda s: S.improve(packed, _backend=s.be))
    add("improve: a wrapper", lambda s: S.improve(object.__new__(JssVectorEnv), _backend=s.be))
    add("improve: no instance", lambda s: S.improve([], _backend=s.be))
    add("improve: pair_cap", lambda s: S.improve(two, pair_cap=0, _backend=s.be))
    add("improve: unfinished", lambda s: S.improve(s.early))
    add("tabu_search: walkers", lambda s: S.tabu_search(two, walkers=0, _backend=s.be))
    add("tabu_search: moves", lambda s: S.tabu_search(two, moves="shift", _backend=s.be))
    add("tabu_search: reach", lambda s: S.tabu_search(two, reach=1, _backend=s.be))
    add("tabu_search: tenure", lambda s: S.tabu_search(two, tenure=(5, 3), _backend=s.be))
    add("tabu_search: target", lambda s: S.tabu_search(two, walkers=2, target="best", _backend=s.be))
    add("relink_search: walkers", lambda s: S.relink_search(two, walkers=0, _backend=s.be))
    add("relink_search: rounds", lambda s: S.relink_search(two, rounds=-1, _backend=s.be))
    add("relink_search: share", lambda s: S.relink_search(two, share=(3, 2), _backend=s.be))
    add("relink_search: reach", lambda s: S.relink_search(two, reach=-1, _backend=s.be))
    add("relink_search: tenure", lambda s: S.relink_search(two, tenure=65, _backend=s.be))
    add("relink_search: target", lambda s: S.relink_search(two, walkers=2, target="best", _backend=s.be))
    add("brkga_search: population", lambda s: S.brkga_search(two, population=0, _backend=s.be))
    add("brkga_search: generations", lambda s: S.brkga_search(two, generations=-1, _backend=s.be))
    add("brkga_search: rho", lambda s: S.brkga_search(two, rho=1.5, _backend=s.be))
    add("brkga_search: elite and mutants", lambda s: S.brkga_search(two, population=8, elite=0.6, mutants=0.6, _backend=s.be))
    add("brkga_search: tenure", lambda s: S.brkga_search(two, tenure=65, _backend=s.be))
    add("brkga_search: seed rules", lambda s: S.brkga_search(two, population=1, elite=0.5, mutants=0.0, _backend=s.be))
    add("brkga_search: target", lambda s: S.brkga_search(two, population=8, target="best", _backend=s.be))
    add("bottleneck_search: nodes", lambda s: S.bottleneck_search(two, nodes=4097, _backend=s.be))
    add("bottleneck_search: walkers", lambda s: S.bottleneck_search(two, walkers=0, _backend=s.be))
    add("bottleneck_search: reopt", lambda s: S.bottleneck_search(two, reopt=9, _backend=s.be))
    add("bottleneck_search: spread", lambda s: S.bottleneck_search(two, spread=-1, _backend=s.be))
    add("bottleneck_search: tenure", lambda s: S.bottleneck_search(two, tenure=65, _backend=s.be))
    add("bottleneck_search: target", lambda s: S.bottleneck_search(two, target="best", _backend=s.be))
    add("bottleneck_search: exact target without nodes", lambda s: S.bottleneck_search(two, target="one_machine_exact", _backend=s.be))
    add("beam_search: width", lambda s: S.beam_search(two, width=0, _backend=s.be))
    add("beam_search: check_every", lambda s: S.beam_search(two, check_every=0, _backend=s.be))
    add("destructive_bound: rounds", lambda s: S.destructive_bound(two, rounds=-1, _backend=s.be))
    add("destructive_bound: upper", lambda s: S.destructive_bound(two, upper=-1, _backend=s.be))
    for family in ("beam", "bound", "order", "tabu", "block", "relink", "decode", "machine", "carlier", "propagate"):
        add(f"{family}_library: a library without it", lambda s, family=family: getattr(S, family + "_library")(types.SimpleNamespace(lib=object())))
    # small runs
    for target in ("lower_bound", "one_machine", "one_machine_exact", "destructive", None, 480, [480, 230]):
        add(f"tabu_search(target={target})", lambda s, t=target: S.tabu_search(two, walkers=3, iters=12, target=t, _backend=s.be))
        add(f"brkga_search(target={target})", lambda s, t=target: S.brkga_search(two, population=8, generations=3, target=t, check_every=2, _backend=s.be))
        add(f"bottleneck_search(target={target})", lambda s, t=target: S.bottleneck_search(two, walkers=3, target=t, nodes=16 if t == "one_machine_exact" else 0,
                                                                                         _backend=s.be))
    add("tabu_search(block, one instance)", lambda s: S.tabu_search(two[0], walkers=4, iters=12, tenure=4, moves="block", reach=2, _backend=s.be))
    add("relink_search()", lambda s: S.relink_search(two, walkers=3, iters=8, rounds=2, _backend=s.be))
    add("relink_search(one instance, no target)", lambda s: S.relink_search(two[1], walkers=2, iters=5, rounds=1, target=None, _backend=s.be))
    add("relink_search(targets)", lambda s: S.relink_search(two, walkers=2, iters=5, rounds=1, target=[480, 230], _backend=s.be))
    add("brkga_search(polish)", lambda s: S.brkga_search(two, population=8, generations=2, polish=5, _backend=s.be))
    add("brkga_search(one instance)", lambda s: S.brkga_search(two[0], population=8, generations=2, seed_rules=None, _backend=s.be))
    add("bottleneck_search(polish)", lambda s: S.bottleneck_search(two, walkers=3, polish=5, _backend=s.be))
    add("bottleneck_search(one instance, nodes)", lambda s: S.bottleneck_search(two[0], walkers=2, nodes=8, _backend=s.be))
    add("beam_search()", lambda s: S.beam_search(two, width=3, _backend=s.be))
    add("improve()", lambda s: S.improve(two, _backend=s.be))
    add("improve(a done batch)", lambda s: S.improve(batch(s.be)))
    add("destructive_bound()", lambda s: S.destructive_bound(two, rounds=2, span=8, _backend=s.be))
    return c


# ---- records ---------------------------------------------------------------------------------------------------------------------
def describe(be, out):
    """the record of what a call returned: of every array its shape, dtype and SHA-256, in the order returned"""
    if dataclasses.is_dataclass(out):
        out = [getattr(out, f.name) for f in dataclasses.fields(out) if f.name != "env"]
    elif not isinstance(out, (tuple, list)):
        out = [out]
    rec = []
    for x in out:
        if x is None or isinstance(x, (bool, int, float, str)):
            rec.append(x)
            continue
        if isinstance(x, list):                                          # (BeamResult.actions: one list per group)
            rec.append([np.asarray(y).tolist() for y in x])
            continue
        a = np.ascontiguousarray(np.asarray(be.numpy(x) if not isinstance(x, np.ndarray) else x))
        rec.append({"shape": list(a.shape), "dtype": str(a.dtype), "sha256": hashlib.sha256(a.tobytes()).hexdigest()})
    return {"returns": rec}


def attempt(be, f, *args):
    try:
        out = f(*args)
    except Exception as e:                                               # noqa: BLE001  (whatever it raises is the record)
        return {"raises": type(e).__name__, "message": str(e)}
    return describe(be, out)


def run(be):
    """name -> record, over the whole list; a valid call is made once per form, and the forms must agree"""
    s = Setup(be)
    got = {}
    each = forms(be)
    for name, f in valid_calls():
        recs = {form: attempt(be, f, s, F) for form, F in each.items()}
        first = recs["list"]
        differ = [form for form, r in recs.items() if r != first]
        assert not differ, f"{name}: the forms {differ} give another result than lists do: {recs[differ[0]]} vs {first}"
        assert "returns" in first, f"{name}: {first}"
        got[name] = first
    for name, f in bad_calls() + refusal_calls() + driver_calls():
        assert name not in got, name
        got[name] = attempt(be, f, s)
    return got
