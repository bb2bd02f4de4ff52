"""jss_beam_select (include/jss_beam.h) and jssenv_amd.search.beam_search: beam search on the device.  On the host against the
CPU twin and the kernel source under the SIMT emulator; on the MI355X against libjss_beam_hip.so."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import beam_cases as K  # noqa: E402
from clone_cases import rows_of  # noqa: E402

THREE = ["ta01", "ta02", "ta11"]
_RESULTS = {}


@pytest.fixture(scope="module")
def twin():
    from jssenv_amd.env import CpuBackend
    return CpuBackend()


@pytest.fixture(scope="module")
def emu():
    return K.emu_backend()


@pytest.fixture(scope="module")
def hip():
    from jssenv_amd.env import HipBackend
    be = HipBackend("cuda:0")
    assert be.lib.jss_backend() == b"hip:gfx950"
    return be


def twin_search(twin, instances, width, dedupe=True):
    """beam_search on the twin, SPT continuation; computed once per module and not changed by its readers"""
    key = (tuple(instances) if isinstance(instances, list) else instances, width, dedupe)
    if key not in _RESULTS:
        from jssenv_amd.search import beam_search
        _RESULTS[key] = beam_search(instances, "SPT", width=width, dedupe=dedupe, _backend=twin)
    return _RESULTS[key]


def test_abi_mirror():
    from jssenv_amd import _abi
    assert _abi.ABI_VERSION == 14 and _abi.BEAM_VERSION == 1 and _abi.BEAM_SYMBOLS == ("jss_beam_select",)
    assert "jss_beam_select" not in _abi.SYMBOLS
    assert [f for f, _ in _abi.JssBeam._fields_] == ["n_groups", "width", "n_actions", "flags", "cand_parent", "makespan", "steps",
                                                    "reward_num", "done", "env_makespan", "src", "action", "score", "next_parent",
                                                    "counts"]
    header = open(os.path.join(K.ROOT, "include", "jss_beam.h")).read()
    assert "#define JSS_BEAM_VERSION 1" in header and "#define JSS_BEAM_DEDUPE 1u" in header


# ---- 1. the selection against the NumPy mirror --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", K.SHAPES, ids=str)
def test_select_twin(twin, shape):
    K.case_select_shape(twin, shape)


def test_select_threshold_twin(twin):
    K.case_threshold(twin)


@pytest.mark.parametrize("shape", K.SHAPES, ids=str)
def test_select_emu(emu, shape):
    K.case_select_shape(emu, shape)


def test_select_threshold_emu(emu):
    K.case_threshold(emu)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", K.SHAPES, ids=str)
def test_select_gpu(hip, shape):
    K.case_select_shape(hip, shape)


@pytest.mark.gpu
def test_select_threshold_gpu(hip):
    K.case_threshold(hip)


# ---- 2. ABI errors --------------------------------------------------------------------------------------------------------------
def test_abi_errors_twin(twin):
    K.case_abi_errors(twin)


def test_abi_errors_emu(emu):
    K.case_abi_errors(emu)


@pytest.mark.gpu
def test_abi_errors_gpu(hip):
    K.case_abi_errors(hip)


def test_driver_refuses(twin):
    from jssenv_amd import BatchedJssEnv, instances as I
    from jssenv_amd.search import beam_search
    with pytest.raises(NotImplementedError):
        beam_search(I.synthetic_packed(4, 6, 5), _backend=twin)
    with pytest.raises(NotImplementedError):
        beam_search(BatchedJssEnv("ta01", batch=2, _backend=twin), _backend=twin)
    with pytest.raises(ValueError):
        beam_search("ta01", "weighted", width=2, weights=np.zeros((2, 8), np.int32), _backend=twin)
    with pytest.raises(ValueError):
        beam_search("ta01", width=0, _backend=twin)


# ---- 3. the driver is its definition -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("instances, width", [("ta01", 4), (THREE, 8)], ids=["ta01-4", "three-8"])
def test_driver_is_its_definition_twin(twin, instances, width):
    K.check_driver(twin, instances, width)


def test_driver_is_its_definition_emu(emu, twin):
    """(one emulated run, windows of 8 and 4 levels, against the definition loop on the twin)"""
    K.check_driver(emu, "ta01", 2, max_levels=12, check_every=(8,), definition_on=twin)


@pytest.mark.gpu
@pytest.mark.parametrize("instances, width", [("ta01", 4), (THREE, 8)], ids=["ta01-4", "three-8"])
def test_driver_is_its_definition_gpu(hip, instances, width):
    K.check_driver(hip, instances, width)


@pytest.mark.gpu
def test_width_64_gpu_equals_twin(hip, twin):
    """ta01 at W = 64: the GPU's final batch and per-level choices, byte for byte the twin's"""
    from jssenv_amd.search import beam_search
    want = twin_search(twin, "ta01", 64)
    got = beam_search("ta01", "SPT", width=64, _backend=hip)
    assert got.levels == want.levels and got.makespan.tolist() == want.makespan.tolist()
    assert np.array_equal(got.src, want.src) and np.array_equal(got.action, want.action)
    a, b = rows_of(got.env), rows_of(want.env)
    for k in b:
        assert np.array_equal(a[k], b[k]), k


# ---- 4. width 1 without dedupe is the pilot method ------------------------------------------------------------------------------
def test_width_one_is_the_pilot_method(twin):
    actions, makespan = K.pilot_loop(twin)
    res = twin_search(twin, "ta01", 1, dedupe=False)
    assert makespan == 1391 and len(actions) == 228
    assert res.actions[0] == actions and int(res.makespan[0]) == 1391 and res.levels == 228


# ---- 5. anchors, SPT continuation -----------------------------------------------------------------------------------------------
# (instances, width, dedupe, the makespans include/jss_beam.h's semantics determine, the makespans listed when the feature was
# specified).  The listed ones were measured with a host-loop prototype whose triple held the float return cut to a whole
# number, trunc(reward_num / max_time_op): a coarser identity than the header's exact (makespan, steps, reward_num), which
# merges more.  Three rows are the same under both; ta01 at width 64 and the batch of three are not.  test_anchors holds the
# library to the header's semantics, test_listed_anchors shows where the listed numbers come from.
ANCHORS = [("ta01", 4, True, [1378], [1378]), ("ta01", 16, True, [1335], [1335]), ("ta01", 64, True, [1330], [1321]),
           ("ta01", 16, False, [1391], [1391]), (THREE, 8, True, [1361, 1326, 1482], [1361, 1312, 1472])]
ANCHOR_IDS = ["ta01-4", "ta01-16", "ta01-64", "ta01-16-plain", "three-8"]


@pytest.mark.parametrize("instances, width, dedupe, makespans, _listed", ANCHORS, ids=ANCHOR_IDS)
def test_anchors(twin, instances, width, dedupe, makespans, _listed):
    """beam_search's makespans with the SPT continuation: exact integers that include/jss_beam.h determines (the same figures
    come from the definition loop of beam_cases, which shares only the NumPy selection with the library)."""
    res = twin_search(twin, instances, width, dedupe)
    assert res.makespan.tolist() == makespans
    best = res.score[:, ::width]                       # (levels, G): slot g * W holds the group's best
    if instances == "ta01":
        assert int(best[0, 0]) == 1417
    for g in range(best.shape[1]):
        mine = best[:, g][best[:, g] >= 0]             # (-1: the group had finished)
        assert mine.size and (np.diff(mine) <= 0).all(), g
        assert int(mine[-1]) == makespans[g]


@pytest.mark.parametrize("instances, width, dedupe, makespans, listed", ANCHORS, ids=ANCHOR_IDS)
def test_listed_anchors(twin, instances, width, dedupe, makespans, listed):
    """Which side departs from the header.  The loop of the public calls with the NumPy selection gives `makespans` on the
    exact triple, and every listed makespan -- with the 7 262 duplicates dropped on ta01 at width 64 -- once the triple's third
    member is the truncated float return."""
    env, _, _, _, _ = K.definition_loop(twin, instances, width, dedupe=dedupe)
    assert twin.numpy(env.makespan)[::width].tolist() == makespans
    env, _, _, _, counts = K.definition_loop(twin, instances, width, dedupe=dedupe, truncated_return=True)
    assert twin.numpy(env.makespan)[::width].tolist() == listed
    if (instances, width, dedupe) == ("ta01", 64, True):
        assert int(counts[:, :, 2].sum()) == 7262


# ---- 6. replay ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("instances, width", [("ta01", 4), (THREE, 8)], ids=["ta01-4", "three-8"])
def test_replay(twin, instances, width):
    res = twin_search(twin, instances, width)
    for g, name in enumerate([instances] if isinstance(instances, str) else instances):
        makespan, solution, done = K.replay(twin, name, res.actions[g])
        J, M = solution.shape
        assert done and makespan == int(res.makespan[g])
        assert np.array_equal(solution, res.solution[g][:J, :M])


# ---- 7. resources -----------------------------------------------------------------------------------------------------------------
def test_beam_kernel_resources():
    """libjss_beam_hip.so holds the selection kernel and nothing else: no scratch, no spills, at most 64 KB of LDS"""
    rows = K.beam_kernel_rows()
    assert [r[0] for r in rows] == ["jss_beam_select_kernel(JssBeam)"]
    _, _, _, vspill, sspill, scratch, lds = rows[0]
    assert scratch == 0 and vspill == 0 and sspill == 0 and 0 < lds <= 64 * 1024


def test_beam_library_is_ignored_by_git():
    import subprocess
    out = subprocess.run(["git", "check-ignore", "jssenv_amd/libjss_beam_hip.so", "tests/emu/libjss_beam_emu.so"], cwd=K.ROOT,
                         capture_output=True, text=True)
    if out.returncode == 128:                          # (not a git checkout: nothing to ask)
        return
    assert out.stdout.split() == ["jssenv_amd/libjss_beam_hip.so", "tests/emu/libjss_beam_emu.so"]
