"""jss_lookahead / BatchedJssEnv.lookahead / pilot_step: candidate moves scored by rule rollouts in one launch, without
clones (include/jss_search.h).  On the host against the CPU twin and the kernel source under the SIMT emulator; on the MI355X
against the HIP library, at test sizes and at full size against the twin."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import clone_cases as K  # noqa: E402
import lookahead_cases as L  # noqa: E402
from jssenv_amd import _abi  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def twin():
    from jssenv_amd.env import CpuBackend
    return CpuBackend()


@pytest.fixture(scope="module", params=["auto", "wave"])
def emu(request):
    from emu_backend import EmuBackend
    return EmuBackend(default_kernel=request.param)


@pytest.fixture(scope="module")
def hip():
    from jssenv_amd.env import HipBackend
    be = HipBackend("cuda:0")
    assert be.lib.jss_backend() == b"hip:gfx950"
    return be


# ---- the interface: the companion header and its mirror ----------------------------------------------------------------
def test_search_header_mirror():
    """jss_search.h declares exactly _abi.SEARCH_SYMBOLS, its version matches the mirror, and jss_hip.h is untouched by it"""
    text = open(os.path.join(ROOT, "include", "jss_search.h")).read()
    declared = set(re.findall(r"^int\s+(jss_\w+)\s*\(", text, re.M))
    assert declared == set(_abi.SEARCH_SYMBOLS)
    assert int(re.search(r"#define JSS_SEARCH_VERSION (\d+)", text).group(1)) == _abi.SEARCH_VERSION == 1
    assert '#include "jss_hip.h"' in text and not set(_abi.SEARCH_SYMBOLS) & set(_abi.SYMBOLS)
    assert [f for f, _ in _abi.JssLookahead._fields_] == ["n", "parent", "action", "id_base", "makespan", "steps", "reward_num"]
    assert C.sizeof(_abi.JssLookahead) == 56


def _libs():
    from emu_backend import build as build_emu
    from jssenv_amd.build import build_cpu_twin, build_extension
    out = {"twin": C.CDLL(build_cpu_twin()), "emu": C.CDLL(build_emu())}
    if not _has_gpu():              # no device: a row let through by mistake fails at its launch instead of reading host pointers
        out["hip"] = C.CDLL(build_extension())
    return {k: _abi.ensure_bound(_abi.bind(v), "jss") for k, v in out.items()}


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture(scope="module")
def libs():
    return _libs()


def test_libraries_export_search_symbols(libs):
    for name, lib in libs.items():
        for sym in _abi.SEARCH_SYMBOLS:
            assert hasattr(lib, sym), (name, sym)


@pytest.mark.parametrize("name, expected, build", L.argument_rows(), ids=[r[0] for r in L.argument_rows()])
def test_argument_error(libs, name, expected, build):
    codes = {}
    for lib_name, lib in libs.items():
        rc, changed = L.run_argument_row(lib, build)
        assert not changed, f"{lib_name}: jss_lookahead wrote into buffers {changed}"
        codes[lib_name] = rc
    assert set(codes.values()) == {expected}, codes


# ---- host: the twin ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", K.LAYOUTS)
def test_equivalence_twin(twin, layout):
    L.case_equivalence(twin, layout)


def test_every_action_twin(twin):
    L.case_every_action(twin)


def test_nothing_to_evaluate_twin(twin):
    L.case_nothing_to_evaluate(twin)


def test_oracle_twin(twin):
    L.case_oracle(twin)


def test_pilot_small_twin(twin):
    L.case_pilot_small(twin)


def test_pilot_ta01_twin(twin):
    L.case_pilot_ta01(twin)


def test_refused_while_session_open(twin):
    env = K.make_layout(twin, "compact", 2)
    env.reset()

    class _Open:
        closed = False
    env._session = _Open()
    with pytest.raises(RuntimeError):
        env.lookahead("SPT")
    with pytest.raises(RuntimeError):
        env.pilot_step("SPT")
    env._session = None
    with pytest.raises(ValueError):
        env.lookahead("SPT", actions=[0])


# ---- host: the kernel source under the emulator ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", K.LAYOUTS)
def test_equivalence_emu(emu, layout):
    kinds = L.KINDS if layout == "compact" else (("SPT", 0.0), ("random", 0.0), ("SPT", 0.3))
    L.case_equivalence(emu, layout, kinds=kinds, B=4, n_steps=20, per_parent=4)


def test_every_action_and_errors_emu(emu):
    L.case_every_action(emu)
    L.case_nothing_to_evaluate(emu)


def test_oracle_emu(emu):
    L.case_oracle(emu)


def test_pilot_small_emu(emu):
    L.case_pilot_small(emu)


def test_emu_equals_twin(emu, twin):
    a = L.case_equivalence(emu, "medium", kinds=(("random", 0.0), ("CR", 0.0)), B=4, n_steps=20, per_parent=4)
    b = L.case_equivalence(twin, "medium", kinds=(("random", 0.0), ("CR", 0.0)), B=4, n_steps=20, per_parent=4)
    for k in a:
        for x, y in zip(a[k], b[k]):
            assert np.array_equal(x, y), k


# ---- kernels -------------------------------------------------------------------------------------------------------------
def test_lookahead_kernel_resources():
    """16 kLookahead kernels (packed 16 / 32, one wavefront per env with one or two jobs per lane, four table layouts): no
    scratch, no spilled VGPRs, and at most the VGPRs of their kRollout twins (at least their wavefronts per SIMD)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import LLVM, kernel_resources
    if not os.path.isfile(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf on this host")
    from jssenv_amd.build import build_extension
    rows = {r[0]: r for r in kernel_resources(build_extension())}
    mine = [n for n in rows if re.fullmatch(r"jss::jss_(packed_)?kernel<\d+, 10, \d>", n)]
    assert len(mine) == 16, mine
    for n in mine:
        _, vgpr, _, vspill, _, scratch = rows[n]
        twin = rows[n.replace(", 10, ", ", 4, ")]
        assert scratch == 0 and vspill == 0, n
        assert vgpr <= twin[1], (n, vgpr, twin[1])


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("layout", K.LAYOUTS)
def test_equivalence_gpu(hip, layout):
    L.case_equivalence(hip, layout, B=12, by_shape=K.BY_SHAPE_FULL if layout == "by_shape" else K.BY_SHAPE_SMALL)


@pytest.mark.gpu
def test_every_action_errors_oracle_gpu(hip):
    L.case_every_action(hip)
    L.case_every_action(hip, layout="by_shape", B=10)
    L.case_nothing_to_evaluate(hip)
    L.case_nothing_to_evaluate(hip, layout="compact")
    L.case_oracle(hip)


@pytest.mark.gpu
def test_pilot_gpu(hip):
    L.case_pilot_small(hip)
    L.case_pilot_ta01(hip)


@pytest.mark.gpu
def test_device_candidates_gpu(hip, twin):
    """parents / actions as device tensors (int64, as torch makes them): the same scores as host sequences on the twin"""
    import torch
    out = []
    for be in (hip, twin):
        env = K.make_layout(be, "full", 6, seed=4)
        env.reset()
        K.drive(env, np.random.default_rng(8), 15)
        par, act = np.repeat(np.arange(6), 4), np.tile([-1, 0, 3, 21], 6)
        if be is hip:
            par, act = torch.tensor(par, device="cuda:0"), torch.tensor(act, device="cuda:0")
        out.append([L.host(x) for x in env.lookahead("random", actions=act, parents=par, seed=3, id_base=5)])
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def _full_size(be, case):
    """the three measured shapes of tools/gpu_lookahead_probe.py: (parents, candidates per parent, batch)"""
    rng = np.random.default_rng(11)
    if case == "ta01":
        env = K.make_layout(be, "compact", 4096, seed=1)
        env.reset()
        env.rollout("random", n_iter=60, autoreset=False, seed=2)
        par, act = np.repeat(np.arange(4096), 16), np.tile(np.arange(-1, 15), 4096)
    elif case == "per_env_50x20":
        from jssenv_amd import BatchedJssEnv
        from jssenv_amd import instances as I
        env = BatchedJssEnv(I.synthetic_packed(512, 50, 20), batch=512, _backend=be, seed=1, records="medium")
        env.reset()
        env.rollout("random", n_iter=300, autoreset=False, seed=2)
        par, act = np.repeat(np.arange(512), 21), np.tile(np.arange(-1, 20), 512)
    else:
        env = K.make_layout(be, "by_shape", 2048, seed=1, by_shape=K.BY_SHAPE_FULL)
        env.reset()
        env.rollout("random", n_iter=int(rng.integers(50, 200)), autoreset=False, seed=2)
        return env, None, None
    return env, par.astype(np.int32), act.astype(np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["ta01", "per_env_50x20", "by_shape_all_actions"])
def test_full_size_gpu_equals_twin(hip, twin, case):
    """4 096 ta01 parents x 16, per-env 50 x 20 medium 512 x 21, config 5 by shape 2 048 x all actions: bit-identical to the twin"""
    res = []
    for be in (hip, twin):
        env, par, act = _full_size(be, case)
        for kind, explore in (("SPT", 0.0), ("random", 0.0)):
            if par is None:
                out = env.lookahead(kind, seed=9, explore=explore)
            else:
                out = env.lookahead(kind, actions=act, parents=par, seed=9, explore=explore)
            res.append([L.host(x) for x in out])
    half = len(res) // 2
    for a, b in zip(res[:half], res[half:]):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    assert (res[0][0] > 0).any()


@pytest.mark.gpu
def test_pilot_step_full_size_gpu_equals_twin(hip, twin):
    """one pilot_step over 4 096 mid-episode ta01 envs: actions, scores and the stepped state bit-identical to the twin"""
    res = []
    for be in (hip, twin):
        env = K.make_layout(be, "compact", 4096, seed=1)
        env.reset()
        env.rollout("random", n_iter=40, autoreset=False, seed=2)
        _, _, _, _, info = env.pilot_step("SPT")
        res.append((L.host(info["action"]), L.host(info["scores"]), K.rows_of(env)))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    for k in res[0][2]:
        assert np.array_equal(res[0][2][k], res[1][2][k]), k
