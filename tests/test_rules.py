"""Caller-weighted dispatching rules (include/jss_rules.h): jss_rule_policy / jss_rule_rollout / jss_rule_lookahead and their
Python surface (weights=, WeightedRule, RULE_WEIGHTS, evaluate_weights).  On the host against the CPU twin and the unmodified
kernel source under the SIMT emulator; on the MI355X against the HIP library."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import lookahead_cases as L  # noqa: E402
import rule_cases as R  # noqa: E402
from jssenv_amd import _abi  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    return {k: _abi.ensure_bound(_abi.ensure_bound(_abi.bind(v), "jss"), "jss_rule") for k, v in out.items()}


# ---- 5. the boundary -----------------------------------------------------------------------------------------------------------------
def test_rules_header_mirror():
    """jss_rules.h declares exactly _abi.RULES_SYMBOLS, its version matches the mirror, it includes the two headers it builds
    on and shares no symbol with them; their versions have not moved"""
    text = open(os.path.join(ROOT, "include", "jss_rules.h")).read()
    declared = set(re.findall(r"^int\s+(jss_\w+)\s*\(", text, re.M))
    assert declared == set(_abi.RULES_SYMBOLS) and len(declared) == 3
    assert int(re.search(r"#define JSS_RULES_VERSION (\d+)", text).group(1)) == _abi.RULES_VERSION == 1
    assert '#include "jss_hip.h"' in text and '#include "jss_search.h"' in text
    assert not set(_abi.RULES_SYMBOLS) & (set(_abi.SYMBOLS) | set(_abi.SEARCH_SYMBOLS))
    for header in ("jss_hip.h", "jss_search.h"):
        other = set(re.findall(r"^int\s+(jss_\w+)\s*\(", open(os.path.join(ROOT, "include", header)).read(), re.M))
        assert not other & declared, header
    assert _abi.ABI_VERSION == 14 and _abi.SEARCH_VERSION == 1
    assert [f for f, _ in _abi.JssRule._fields_] == ["weights", "stride"] and C.sizeof(_abi.JssRule) == 16
    for name, value in (("DUR", 0), ("NEXT", 1), ("REM", 2), ("TOTAL", 3), ("OPS", 4), ("WAIT", 5), ("IDLE", 6), ("NOPE", 7), ("N", 8)):
        assert int(re.search(rf"#define JSS_RW_{name} (\d+)", text).group(1)) == value == getattr(_abi, "RW_" + name)
    assert "weighted" not in _abi.POLICY and 8 not in _abi.POLICY.values()


def test_libraries_export_rule_symbols(libs):
    for name, lib in libs.items():
        for sym in _abi.RULES_SYMBOLS:
            assert hasattr(lib, sym), (name, sym)


@pytest.mark.parametrize("name, call, expected, build", R.argument_rows(), ids=[r[0] for r in R.argument_rows()])
def test_argument_error(libs, name, call, expected, build):
    codes = {}
    for lib_name, lib in libs.items():
        rc, changed = R.run_argument_row(lib, call, build)
        assert not changed, f"{lib_name}: {call} wrote into buffers {changed}"
        codes[lib_name] = rc
    assert set(codes.values()) == {expected}, codes


def test_kind_8_is_still_unknown(libs):
    for lib_name, lib in libs.items():
        for build in R.kind8_rows():
            w = L._World()
            call, args = build(w)
            before = [b.copy() for b in w.bufs]
            assert getattr(lib, call)(*args) == _abi.E_KIND, (lib_name, call)
            assert all(np.array_equal(a, b) for a, b in zip(before, w.bufs)), (lib_name, call)


def test_python_surface(twin):
    from jssenv_amd import BatchedJssEnv, BucketedJssEnv
    from jssenv_amd.dispatching import RULE_WEIGHTS
    env = BatchedJssEnv("ta01", batch=3, _backend=twin)
    env.reset()
    row = RULE_WEIGHTS["SPT"]
    for bad in (row.astype(np.int64), row.astype(np.float32), row[:7], np.tile(row, (2, 1)), list(row), None):
        with pytest.raises(ValueError):
            env.policy("weighted", weights=bad)
    with pytest.raises(ValueError):
        env.rollout("SPT", weights=row)
    for call in (lambda: env.rollout_steps("weighted", steps=2), lambda: env.trajectory("weighted", steps=2),
                 lambda: env.policy_step_steps("weighted", steps=2)):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(NotImplementedError):
        bucketed = BucketedJssEnv(["ta01", "ta41"], batch=4, _backend=twin)
        bucketed.reset()
        bucketed.policy("weighted")

    class _Open:
        closed = False
    env._session = _Open()
    with pytest.raises(NotImplementedError):
        env.rollout("weighted", weights=row)
    env._session = None


# ---- host: the twin ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES + ("by-shape",))
def test_stock_rows_twin(twin, shape):
    R.case_stock_rows(twin, shape)


def test_golden_twin(twin):
    R.case_golden(twin)


@pytest.mark.parametrize("shape", R.SHAPES + ("by-shape",))
def test_mixed_rows_twin(twin, shape):
    R.case_mixed_rows(twin, shape)


@pytest.mark.parametrize("shape", ("p32-J32", "p32-ragged"))
def test_mixed_rows_reach_bias_and_ties(twin, shape):
    """on the yardstick's own trace: a NOPE chosen by its bias while a job was legal, and a choice decided by the tie rule"""
    trace = R.case_mixed_rows(twin, shape)
    assert trace["nopes"] >= 1 and trace["ties"] >= 1, trace


def test_wrap_twin(twin):
    R.case_wrap(twin)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_wrap_state_twin(twin, shape):
    R.case_wrap_state(twin, shape)


@pytest.mark.parametrize("shape", ("p16-J11", "p32-ragged", "w1-J40-map", "w2-J65", "by-shape"))
def test_lookahead_twin(twin, shape):
    R.case_lookahead(twin, shape, per_parent=6)


# ---- host: the kernel source under the emulator ---------------------------------------------------------------------------------------
# (the emulator plays some hundred env steps a second: slices and the first steps of an episode on every shape, whole episodes
#  on the smallest one; the twin above and the device below play everything whole)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_stock_rows_emu(emu, shape):
    R.case_stock_rows(emu, shape, rules=("SPT", "MWR"), explores=(0.5,), whole=shape == "p16-J11")


@pytest.mark.parametrize("shape", ("p16-J11", "p32-ragged", "w1-J40-map", "w2-J65"))
def test_all_stock_rows_emu(emu, shape):
    """every stock row, without exploration, in slices: one shape per selector form"""
    R.case_stock_rows(emu, shape, explores=(0.0,), whole=False)


def test_by_shape_emu(emu):
    """a batch dealt out by shape class (slow under the emulator: 100-job rows): the first steps of the mixed rows -- every
    feature, policy launches -- and of one rollout per form of the row; the twin and the device play it whole"""
    R.case_mixed_rows(emu, "by-shape", max_steps=5)
    env, _ = R.make_shape(emu, "by-shape")
    ref, _ = R.make_shape(emu, "by-shape")
    for w in (R.RULE_WEIGHTS["LWR"], np.tile(R.RULE_WEIGHTS["LWR"], (env.batch, 1))):
        for e in (env, ref):
            e.reset()
        env.rollout("weighted", n_iter=4, autoreset=False, explore=0.5, seed=3, weights=w)
        ref.rollout("LWR", n_iter=4, autoreset=False, explore=0.5, seed=3)
        R.same(R.snapshot(ref), R.snapshot(env), "by-shape")


@pytest.mark.parametrize("shape", R.SHAPES)
def test_mixed_rows_emu(emu, shape):
    R.case_mixed_rows(emu, shape, max_steps=None if shape == "p16-J11" else 24)


def test_wrap_emu(emu):
    R.case_wrap(emu)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_wrap_state_emu(emu, twin, shape):
    assert np.array_equal(R.case_wrap_state(emu, shape), R.case_wrap_state(twin, shape))


@pytest.mark.parametrize("shape", ("p16-J11", "p32-ragged", "w1-J40-map", "w2-J65"))
def test_lookahead_emu(emu, shape):
    R.case_lookahead(emu, shape, per_parent=2, n_iter=6, explores=(0.4,))


# ---- 6. host mirror, population call ----------------------------------------------------------------------------------------------------
def _golden_makespans(inst):
    g = np.load(os.path.join(ROOT, "tests", "golden", "rules.npz"))
    rules, insts = [str(x) for x in g["rules"]], [str(x) for x in g["instances"]]
    return {r: int(g["makespan"][rules.index(r), insts.index(inst)]) for r in rules}


def test_weighted_rule_run_episode_golden():
    from jssenv_amd import make
    from jssenv_amd.dispatching import RULE_WEIGHTS, WeightedRule, device_kind
    rule = WeightedRule(RULE_WEIGHTS["SPT"], name="SPT as weights")
    assert device_kind(rule) == "weighted" and rule.get_name() == "SPT as weights"
    env = make("jss-v1", env_config={"instance_path": "ta01"}, device="cpu")
    _, makespan = rule.run_episode(env)
    assert makespan == _golden_makespans("ta01")["SPT"] == 1462


def test_weighted_rule_on_an_env_with_the_reference_attributes():
    """the host mirror reads public attributes only: it plays the oracle's env object, to the golden makespan"""
    from jssenv_amd import instances as I
    from jssenv_amd.dispatching import RULE_WEIGHTS, WeightedRule
    from oracle import OracleEnv

    class Env(OracleEnv):
        def reset(self):
            super().reset()
            return self._obs(), {}
    env = Env(I.builtin_instance("ta01"), strict=True)
    _, makespan = WeightedRule(RULE_WEIGHTS["FIFO"]).run_episode(env)
    assert makespan == 1486


def test_evaluate_weights_golden(twin):
    from jssenv_amd.dispatching import RULE_WEIGHTS, evaluate_weights
    names = list(RULE_WEIGHTS)
    w = np.stack([RULE_WEIGHTS[n] for n in names])
    gold = _golden_makespans("ta01")
    assert evaluate_weights("ta01", w, device="cpu").ravel().tolist() == [gold[n] for n in names]
    both = evaluate_weights(["ta01", "ta41"], w, device="cpu")
    assert both.shape == (6, 2) and both[:, 0].tolist() == [gold[n] for n in names]
    assert both[:, 1].tolist() == [_golden_makespans("ta41")[n] for n in names]


def test_evaluate_weights_takes_tensors(twin):
    import torch
    from jssenv_amd.dispatching import evaluate_weights
    w = np.random.default_rng(2).integers(-8, 9, size=(5, 8)).astype(np.int32)
    a = evaluate_weights(["ta01", "ta02"], w, device="cpu")
    assert np.array_equal(evaluate_weights(["ta01", "ta02"], torch.from_numpy(w), device="cpu"), a) and a.shape == (5, 2)
    with pytest.raises(ValueError):
        evaluate_weights("ta01", w.astype(np.int64), device="cpu")


def test_compare_rules_with_a_registered_weighted_rule():
    """a WeightedRule put into DISPATCHING_RULES is compared like the stock ones: on a jssenv_amd env by jss_rule_rollout with
    its row, on any other env by the host loop; both give the golden makespan of the rule it restates"""
    from jssenv_amd import dispatching as D
    from jssenv_amd import instances as I
    from jssenv_amd import make
    from oracle import OracleEnv

    class Env(OracleEnv):
        def reset(self):
            super().reset()
            return self._obs(), {}
    D.DISPATCHING_RULES["MWR-row"] = D.WeightedRule(D.RULE_WEIGHTS["MWR"], name="MWR-row")
    try:
        on_device = D.compare_rules(make("jss-v1", env_config={"instance_path": "ta01"}, device="cpu"), ["MWR-row"], num_episodes=3, seed=1)
        on_host = D.compare_rules(Env(I.builtin_instance("ta01"), strict=True), ["MWR-row"], num_episodes=1)
    finally:
        del D.DISPATCHING_RULES["MWR-row"]
    want = float(_golden_makespans("ta01")["MWR"])
    assert on_device["MWR-row"]["avg_makespan"] == want == on_host["MWR-row"]["avg_makespan"]


def test_mirror_twin(twin):
    R.case_mirror(twin)


# ---- 7. resources ------------------------------------------------------------------------------------------------------------------------
def _table(path):
    rows = {}
    for line in open(path):
        m = re.match(r"(.*?)\s+vgpr\s+(\d+) sgpr\s+(\d+) vspill\s+(\d+) sspill\s+(\d+) scratch (\d+)", line)
        if m:
            rows[m.group(1).strip()] = tuple(int(x) for x in m.groups()[1:])
    return rows


def test_rule_kernels_resources():
    """The kernel set is the parent's (190 names, from the committed table of the parent: no kernel was added); every kernel
    outside kPolicy / kRollout / kLookahead keeps its VGPR count and wavefronts per SIMD -- the weighted selector is not in it --
    and every kPolicy / kRollout / kLookahead kernel has no scratch, no spilled VGPRs and at least its wavefronts per SIMD
    (512 / VGPRs rounded up to 8, at most 8)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import LLVM, kernel_resources
    if not os.path.isfile(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf on this host")
    from jssenv_amd.build import build_extension
    parent = _table(os.path.join(ROOT, "profiles", "r12_launcher", "kernel_resources.txt"))
    assert len(parent) == 190
    now = {n: (v, s, vs, ss, scratch) for n, v, s, vs, ss, scratch in kernel_resources(build_extension())}
    assert set(now) == set(parent)
    occ = lambda v: min(8, 512 // ((v + 7) // 8 * 8))        # noqa: E731
    touched = re.compile(r"jss::jss_(packed_)?kernel<\d+, (3|4|10), \d>|jss_multi_kernel<3>")
    bad = []
    for n, (v, _, vs, _, scratch) in sorted(now.items()):
        pv = parent[n][0]
        if touched.match(n):
            if scratch or vs or occ(v) < occ(pv):
                bad.append((n, pv, v, vs, scratch))
        elif v != pv or occ(v) != occ(pv):
            bad.append((n, pv, v, vs, scratch))
    print("\n".join(f"{n}: {pv} -> {v} VGPRs" for n, (v, *_) in sorted(now.items()) for pv in [parent[n][0]] if v != pv))
    assert not bad, f"(kernel, parent's VGPRs, VGPRs, spilled, scratch): {bad}"
    assert sum(1 for n in now if touched.match(n)) == 49


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", R.SHAPES + ("by-shape",))
def test_stock_rows_gpu(hip, shape):
    R.case_stock_rows(hip, shape)


@pytest.mark.gpu
def test_golden_gpu(hip):
    R.case_golden(hip)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", R.SHAPES + ("by-shape",))
def test_mixed_rows_gpu(hip, shape):
    R.case_mixed_rows(hip, shape)


@pytest.mark.gpu
def test_wrap_gpu(hip):
    R.case_wrap(hip)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", R.SHAPES)
def test_wrap_state_gpu(hip, twin, shape):
    assert np.array_equal(R.case_wrap_state(hip, shape), R.case_wrap_state(twin, shape))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ("p16-J11", "p16-J16", "p32-ragged", "w1-J64", "w1-J40-map", "w2-J65", "by-shape"))
def test_lookahead_gpu(hip, shape):
    R.case_lookahead(hip, shape, per_parent=6)


@pytest.mark.gpu
def test_mirror_and_population_gpu(hip, twin):
    """the host mirror against the device, and one population call: 96 random rows on ta01, device == twin"""
    from jssenv_amd.dispatching import evaluate_weights
    R.case_mirror(hip)
    w = np.random.default_rng(3).integers(-8, 9, size=(96, 8)).astype(np.int32)
    a = evaluate_weights("ta01", w, _backend=hip)
    b = evaluate_weights("ta01", w, _backend=twin)
    assert np.array_equal(a, b) and (a > 0).all()
    import torch
    assert np.array_equal(evaluate_weights(["ta01", "ta41"], torch.from_numpy(w).to("cuda:0"), _backend=hip),
                          evaluate_weights(["ta01", "ta41"], w, _backend=twin))
