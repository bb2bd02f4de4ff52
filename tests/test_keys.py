"""Per-operation priority keys (include/jss_keys.h): jss_key_policy / jss_key_rollout / jss_key_lookahead and their Python
surface (keys=, nope_key=, KeyRule, rule_keys, keys_from_actions, keys_from_floats, evaluate_keys).  On the host against the
CPU twin and the unmodified kernel source under the SIMT emulator; on the MI355X against the HIP library."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import key_cases as Y  # noqa: E402
import lookahead_cases as L  # noqa: E402
import rule_cases as R  # noqa: E402
from jssenv_amd import _abi  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOKAHEAD_SHAPES = ("p16-J11", "p16-J16", "p32-ragged", "w1-J64", "w1-J40-map", "w2-J65", "by-shape")


@pytest.fixture(scope="module")
def twin():
    from jssenv_amd.env import CpuBackend
    return CpuBackend()


@pytest.fixture(scope="module")
def emu():
    from emu_backend import EmuBackend
    return EmuBackend()


@pytest.fixture(scope="module")
def hip():
    from jssenv_amd.env import HipBackend
    be = HipBackend("cuda:0")
    assert be.lib.jss_backend() == b"hip:gfx950"
    return be


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture(scope="module")
def libs():
    from emu_backend import build as build_emu
    from jssenv_amd.build import build_cpu_twin, build_extension
    out = {"twin": C.CDLL(build_cpu_twin()), "emu": C.CDLL(build_emu())}
    if not _has_gpu():              # no device: a row let through by mistake fails at its launch instead of reading host pointers
        out["hip"] = C.CDLL(build_extension())
    return {k: _abi.ensure_bound(_abi.ensure_bound(_abi.bind(v), "jss"), "jss_key") for k, v in out.items()}


# ---- 1. the boundary -----------------------------------------------------------------------------------------------------------------
def _declared(header):
    return set(re.findall(r"^int\s+(jss_\w+)\s*\(", open(os.path.join(ROOT, "include", header)).read(), re.M))


def test_keys_header_mirror():
    """jss_keys.h declares exactly _abi.KEYS_SYMBOLS, its version matches the mirror, it includes the two headers it builds on
    and shares no symbol with the three other headers; their versions have not moved"""
    text = open(os.path.join(ROOT, "include", "jss_keys.h")).read()
    declared = _declared("jss_keys.h")
    assert declared == set(_abi.KEYS_SYMBOLS) and len(declared) == 3
    assert int(re.search(r"#define JSS_KEYS_VERSION (\d+)", text).group(1)) == _abi.KEYS_VERSION == 1
    assert '#include "jss_hip.h"' in text and '#include "jss_search.h"' in text
    assert not set(_abi.KEYS_SYMBOLS) & (set(_abi.SYMBOLS) | set(_abi.SEARCH_SYMBOLS) | set(_abi.RULES_SYMBOLS))
    for header in ("jss_hip.h", "jss_search.h", "jss_rules.h"):
        assert not _declared(header) & declared, header
    assert _abi.ABI_VERSION == 14 and _abi.SEARCH_VERSION == 1 and _abi.RULES_VERSION == 1
    for header, macro, version in (("jss_hip.h", "JSS_ABI_VERSION", 14), ("jss_search.h", "JSS_SEARCH_VERSION", 1),
                                   ("jss_rules.h", "JSS_RULES_VERSION", 1)):
        other = open(os.path.join(ROOT, "include", header)).read()
        assert int(re.search(rf"#define {macro} (\d+)", other).group(1)) == version, header
    assert [f for f, _ in _abi.JssKeys._fields_] == ["keys", "stride", "nope_key"] and C.sizeof(_abi.JssKeys) == 16
    assert "keys" not in _abi.POLICY and 9 not in _abi.POLICY.values()


def test_libraries_export_key_symbols(libs):
    for name, lib in libs.items():
        for sym in _abi.KEYS_SYMBOLS:
            assert hasattr(lib, sym), (name, sym)


@pytest.mark.parametrize("name, call, expected, build", Y.argument_rows(), ids=[r[0] for r in Y.argument_rows()])
def test_argument_error(libs, name, call, expected, build):
    codes = {}
    for lib_name, lib in libs.items():
        rc, changed = R.run_argument_row(lib, call, build)
        assert not changed, f"{lib_name}: {call} wrote into buffers {changed}"
        codes[lib_name] = rc
    assert set(codes.values()) == {expected}, codes


def test_kind_9_is_still_unknown(libs):
    for lib_name, lib in libs.items():
        assert hasattr(lib, "jss_key_policy")
        for build in Y.kind9_rows():
            w = L._World()
            call, args = build(w)
            before = [b.copy() for b in w.bufs]
            assert getattr(lib, call)(*args) == _abi.E_KIND, (lib_name, call)
            assert all(np.array_equal(a, b) for a, b in zip(before, w.bufs)), (lib_name, call)


# ---- 7. the Python surface -------------------------------------------------------------------------------------------------------------
def test_python_surface(twin):
    from jssenv_amd import BatchedJssEnv, BucketedJssEnv
    from jssenv_amd.dispatching import rule_keys
    env = BatchedJssEnv("ta01", batch=3, _backend=twin)
    env.reset()
    t = rule_keys("ta01", "SPT")
    assert t.dtype == np.int32 and t.shape == (15, 15)
    for bad in (t.astype(np.int64), t.astype(np.float32), t[:14], t[:, :14], np.tile(t, (2, 1, 1)), t.tolist(), None):
        with pytest.raises(ValueError):
            env.policy("keys", keys=bad)
    for call in (lambda: env.rollout("SPT", keys=t), lambda: env.policy("weighted", keys=t), lambda: env.lookahead("SPT", keys=t),
                 lambda: env.rollout("SPT", nope_key=1), lambda: env.rollout("keys", keys=t, nope_key=2**31)):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: env.rollout_steps("keys", steps=2), lambda: env.trajectory("keys", steps=2),
                 lambda: env.policy_step_steps("keys", steps=2)):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(NotImplementedError):
        bucketed = BucketedJssEnv(["ta01", "ta41"], batch=4, _backend=twin)
        bucketed.reset()
        bucketed.policy("keys")
    with pytest.raises(ValueError):
        rule_keys("ta01", "FIFO")
    with pytest.raises(ValueError):
        rule_keys("ta01", "CR")

    class _Open:
        closed = False
    env._session = _Open()
    with pytest.raises(NotImplementedError):
        env.rollout("keys", keys=t)
    env._session = None


def test_keys_from_floats_keeps_the_order():
    import torch
    from jssenv_amd.dispatching import keys_from_floats
    tiny = np.float32(1e-45)                                              # a denormal
    x = np.array([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, 1.5, 1.5, -1.5, 3e38, -3e38, 1e-38, 2.0 ** -126, -7.25, 0.1], np.float32)
    x = x[np.random.default_rng(3).permutation(len(x))]
    for keys in (keys_from_floats(x), keys_from_floats(torch.from_numpy(x)).numpy(), keys_from_floats(x.astype(np.float64))):
        assert keys.dtype == np.int32 and keys.shape == x.shape
        for i in range(len(x)):
            for j in range(len(x)):
                assert (x[i] < x[j]) == (keys[i] < keys[j]) and (x[i] == x[j]) == (keys[i] == keys[j]), (x[i], x[j])
    assert keys_from_floats(np.float32(-0.0).reshape(1))[0] == keys_from_floats(np.float32(0.0).reshape(1))[0] == 0
    assert keys_from_floats(x.reshape(3, 5)).shape == (3, 5)
    for bad in (np.array([1.0, np.nan], np.float32), torch.tensor([np.nan, 0.0])):
        with pytest.raises(ValueError):
            keys_from_floats(bad)


def _golden_makespans(inst):
    g = np.load(os.path.join(ROOT, "tests", "golden", "rules.npz"))
    rules, insts = [str(x) for x in g["rules"]], [str(x) for x in g["instances"]]
    return {r: int(g["makespan"][rules.index(r), insts.index(inst)]) for r in rules}


class _OracleGym:
    """the oracle's env object with the reset() a run_episode expects"""
    def __new__(cls, inst):
        from oracle import OracleEnv

        class Env(OracleEnv):
            def reset(self):
                super().reset()
                return self._obs(), {}
        return Env(inst, strict=True)


def test_key_rule_plays_the_oracle_and_the_facade():
    """the host mirror reads public attributes only: it plays the oracle's env object and the device="cpu" facade (there by
    jss_key_rollout) to the golden makespans of the rules its tables restate"""
    from jssenv_amd import instances as I
    from jssenv_amd import make
    from jssenv_amd.dispatching import KeyRule, device_kind, rule_keys
    gold = _golden_makespans("ta01")
    assert gold["SPT"] == 1462
    for name in ("SPT", "MWR"):
        rule = KeyRule(rule_keys("ta01", name), name=name + " as keys")
        assert device_kind(rule) == "keys" and rule.get_name() == name + " as keys"
        _, on_oracle = rule.run_episode(_OracleGym(I.builtin_instance("ta01")))
        facade = make("jss-v1", env_config={"instance_path": "ta01"}, device="cpu")
        _, on_facade = rule.run_episode(facade)
        assert on_oracle == on_facade == gold[name], name
        # ... and decision for decision through the facade's step()
        facade.reset()
        done = False
        while not done:
            _, _, done, _, _ = facade.step(rule(facade))
        assert facade.current_time_step == gold[name]
    with pytest.raises(ValueError):
        KeyRule(np.zeros((15, 15), np.float32))
    with pytest.raises(ValueError):
        KeyRule(np.zeros(15, np.int32))


def test_compare_rules_with_a_registered_key_rule():
    from jssenv_amd import dispatching as D
    from jssenv_amd import instances as I
    from jssenv_amd import make
    D.DISPATCHING_RULES["MWR-keys"] = D.KeyRule(D.rule_keys("ta01", "MWR"), name="MWR-keys")
    try:
        on_device = D.compare_rules(make("jss-v1", env_config={"instance_path": "ta01"}, device="cpu"), ["MWR-keys"], num_episodes=3, seed=1)
        on_host = D.compare_rules(_OracleGym(I.builtin_instance("ta01")), ["MWR-keys"], num_episodes=1)
    finally:
        del D.DISPATCHING_RULES["MWR-keys"]
    want = float(_golden_makespans("ta01")["MWR"])
    assert on_device["MWR-keys"]["avg_makespan"] == want == on_host["MWR-keys"]["avg_makespan"]


def test_evaluate_keys_twin(twin):
    """evaluate_keys equals P facade episodes, takes tensors, and returns solutions that end at the makespan"""
    import torch
    from jssenv_amd import instances as I
    from jssenv_amd import make
    from jssenv_amd.dispatching import KeyRule, evaluate_keys, rule_keys
    inst = I.builtin_instance("ta01")
    rng = np.random.default_rng(4)
    pop = np.concatenate([rng.integers(-50, 50, size=(4, 15, 15)).astype(np.int32),
                          np.stack([rule_keys(inst, r) for r in Y.STOCK])])
    ms, sol = evaluate_keys("ta01", pop, device="cpu", return_solution=True)
    assert ms.shape == (9,) and sol.shape == (9, 15, 15) and ms.dtype == np.int64
    gold = _golden_makespans("ta01")
    assert ms[4:].tolist() == [gold[r] for r in Y.STOCK]
    assert ((sol + inst.duration[None]).max(axis=(1, 2)) == ms).all() and (sol >= 0).all()
    facade = make("jss-v1", env_config={"instance_path": "ta01"}, device="cpu")
    for i in range(4):
        assert KeyRule(pop[i]).run_episode(facade)[1] == ms[i], i
    assert np.array_equal(evaluate_keys(inst, torch.from_numpy(pop), device="cpu"), ms)
    assert np.array_equal(evaluate_keys(inst, pop, nope_key=None, _backend=twin), ms)
    waits = evaluate_keys(inst, pop, nope_key=0, device="cpu")
    assert waits.shape == (9,) and (waits != ms).any()                   # (NOPE-happy: other schedules)
    assert evaluate_keys(inst, pop[:0], device="cpu").shape == (0,)
    for bad in (pop.astype(np.int64), pop[0], pop[:, :14]):
        with pytest.raises(ValueError):
            evaluate_keys(inst, bad, device="cpu")


# ---- host: the twin ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", Y.SHAPES + ("by-shape",))
def test_stock_tables_twin(twin, shape):
    Y.case_stock_tables(twin, shape)


def test_golden_twin(twin):
    Y.case_golden(twin)


@pytest.mark.parametrize("nope_key", (2, Y.I32_MIN))
@pytest.mark.parametrize("shape", Y.SHAPES + ("by-shape",))
def test_random_tables_twin(twin, shape, nope_key):
    Y.case_random_tables(twin, shape, nope_key)


@pytest.mark.parametrize("shape", ("p32-J32", "p32-ragged"))
def test_random_tables_reach_ties_and_nopes(twin, shape):
    """on the yardstick's own trace: a choice decided by the tie rule; with nope_key = 2 a NOPE taken while a job was legal, with
    INT32_MIN none"""
    trace = Y.case_random_tables(twin, shape, 2)
    assert trace["nopes"] >= 1 and trace["ties"] >= 1, trace
    trace = Y.case_random_tables(twin, shape, Y.I32_MIN)
    assert trace["nopes"] == 0 and trace["ties"] >= 1, trace


@pytest.mark.parametrize("shape", Y.SHAPES + ("by-shape",))
def test_extremes_twin(twin, shape):
    Y.case_extremes(twin, shape)


@pytest.mark.parametrize("shape", ("p16-J11", "p32-ragged", "w1-J40-map", "w2-J65", "by-shape"))
def test_replay_twin(twin, shape):
    Y.case_replay(twin, shape)


def test_replay_oracle_spt():
    """keys_from_actions over the oracle alone: SPT on 11 x 5, the 55 actions one for one, both makespans 764"""
    from jssenv_amd.dispatching import KeyRule, keys_from_actions, rule_keys
    from oracle import OracleEnv
    inst = R._inst(11, 5)

    def play(rule):
        orc = OracleEnv(inst, strict=True)
        orc.reset()
        acts = []
        while True:
            a = rule(orc)
            if a < 0:
                return acts, orc.current_time_step
            acts.append(a)
            orc.step(a)
    first, ms = play(KeyRule(rule_keys(inst, "SPT")))
    again, ms2 = play(KeyRule(keys_from_actions(inst, first)))
    assert sum(1 for a in first if a < inst.jobs) == 55 and first == again and ms == ms2 == 764


@pytest.mark.parametrize("shape", LOOKAHEAD_SHAPES)
def test_lookahead_twin(twin, shape):
    Y.case_lookahead(twin, shape, per_parent=6)


def test_mirror_twin(twin):
    Y.case_mirror(twin)


# ---- host: the kernel source under the emulator ---------------------------------------------------------------------------------------
# (the emulator plays some hundred env steps a second: slices and whole episodes on p16-J11, the first steps elsewhere)
def test_stock_tables_emu(emu):
    Y.case_stock_tables(emu, "p16-J11", rules=("SPT", "MWR"), explores=(0.5,))


@pytest.mark.parametrize("shape", ("p32-ragged", "w1-J40-map", "w2-J65"))
def test_stock_tables_slices_emu(emu, shape):
    """one shape per selector form, in slices"""
    Y.case_stock_tables(emu, shape, rules=("SPT", "MWR"), explores=(0.5,), whole=False)


@pytest.mark.parametrize("nope_key", (2, Y.I32_MIN))
def test_random_tables_emu(emu, nope_key):
    Y.case_random_tables(emu, "p16-J11", nope_key)


@pytest.mark.parametrize("shape", ("p16-J16", "p32-ragged", "w1-J64", "w2-J65"))
def test_random_tables_first_steps_emu(emu, shape):
    Y.case_random_tables(emu, shape, 2, max_steps=12)


def test_extremes_emu(emu):
    Y.case_extremes(emu, "p16-J11")


@pytest.mark.parametrize("shape", ("p32-ragged", "w2-J65"))
def test_extremes_first_steps_emu(emu, shape):
    Y.case_extremes(emu, shape, max_steps=8)


def test_lookahead_emu(emu):
    Y.case_lookahead(emu, "p16-J11", per_parent=2, n_iter=6, explores=(0.4,))


# ---- 8. resources ------------------------------------------------------------------------------------------------------------------------
def _table(path):
    rows = {}
    for line in open(path):
        m = re.match(r"(.*?)\s+vgpr\s+(\d+) sgpr\s+(\d+) vspill\s+(\d+) sspill\s+(\d+) scratch (\d+)", line)
        if m:
            rows[m.group(1).strip()] = tuple(int(x) for x in m.groups()[1:])
    return rows


def test_key_kernels_resources():
    """Against the parent's table (profiles/r14_rules): the same kernel names -- no kernel was added --; every kernel outside
    kPolicy / kRollout / kLookahead keeps its VGPR count -- the key selector is not in it --; each of the 49 kernels that carry
    the caller's selectors has no scratch, no spilled VGPRs and at least the parent's wavefronts per SIMD (512 / VGPRs rounded up
    to 8, at most 8)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import LLVM, kernel_resources
    if not os.path.isfile(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf on this host")
    from jssenv_amd.build import build_extension
    parent = _table(os.path.join(ROOT, "profiles", "r14_rules", "kernel_resources.txt"))
    assert len(parent) == 190
    lib = build_extension()
    assert hasattr(C.CDLL(lib), "jss_key_rollout")
    now = {n: (v, s, vs, ss, scratch) for n, v, s, vs, ss, scratch in kernel_resources(lib)}
    assert set(now) == set(parent)
    occ = lambda v: min(8, 512 // ((v + 7) // 8 * 8))        # noqa: E731
    touched = re.compile(r"jss::jss_(packed_)?kernel<\d+, (3|4|10), \d>|jss_multi_kernel<3>")
    bad = []
    for n, (v, _, vs, _, scratch) in sorted(now.items()):
        pv = parent[n][0]
        if touched.match(n):
            if scratch or vs or occ(v) < occ(pv):
                bad.append((n, pv, v, vs, scratch))
        elif v != pv:
            bad.append((n, pv, v, vs, scratch))
    assert not bad, f"(kernel, parent's VGPRs, VGPRs, spilled, scratch): {bad}"
    assert sum(1 for n in now if touched.match(n)) == 49


# ---- 9. GPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", Y.SHAPES + ("by-shape",))
def test_stock_tables_gpu(hip, shape):
    Y.case_stock_tables(hip, shape)


@pytest.mark.gpu
def test_golden_gpu(hip):
    Y.case_golden(hip)


@pytest.mark.gpu
@pytest.mark.parametrize("nope_key", (2, Y.I32_MIN))
@pytest.mark.parametrize("shape", Y.SHAPES + ("by-shape",))
def test_random_tables_gpu(hip, shape, nope_key):
    trace = Y.case_random_tables(hip, shape, nope_key)
    if shape in ("p32-J32", "p32-ragged"):
        assert trace["ties"] >= 1 and (trace["nopes"] >= 1) == (nope_key == 2), trace


@pytest.mark.gpu
@pytest.mark.parametrize("shape", Y.SHAPES + ("by-shape",))
def test_extremes_gpu(hip, shape):
    Y.case_extremes(hip, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ("p16-J11", "p32-ragged", "w1-J40-map", "w2-J65", "by-shape"))
def test_replay_gpu(hip, shape):
    Y.case_replay(hip, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", LOOKAHEAD_SHAPES)
def test_lookahead_gpu(hip, shape):
    Y.case_lookahead(hip, shape, per_parent=6)


@pytest.mark.gpu
def test_mirror_gpu(hip):
    Y.case_mirror(hip)


@pytest.mark.gpu
def test_evaluate_keys_gpu(hip, twin):
    """one population call: 96 random tables on ta01, device equal to twin -- as arrays and as device tensors"""
    import torch
    from jssenv_amd.dispatching import evaluate_keys
    pop = np.random.default_rng(6).integers(-1000, 1000, size=(96, 15, 15)).astype(np.int32)
    want, want_sol = evaluate_keys("ta01", pop, nope_key=900, _backend=twin, return_solution=True)
    got, got_sol = evaluate_keys("ta01", pop, nope_key=900, _backend=hip, return_solution=True)
    assert np.array_equal(got, want) and np.array_equal(got_sol, want_sol) and len(set(got.tolist())) > 10
    assert np.array_equal(evaluate_keys("ta01", torch.from_numpy(pop).to("cuda:0"), nope_key=900, device="cuda:0"), want)
