"""jss_order_eval / jss_order_apply (include/jss_order.h), BatchedJssEnv.evaluate_order and search.improve: the exact schedule of
a machine order, its tails, critical operations and swap neighbourhood, and steepest descent over that neighbourhood.  On the
host against the CPU twin and the kernel source under the SIMT emulator; on the MI355X against libjss_order_hip.so."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import order_cases as K  # noqa: E402

NAMES = list(K.CASES)
RULES = ["SPT", "FIFO", "random"]


@pytest.fixture(scope="module")
def twin():
    return K.twin_backend()


@pytest.fixture(scope="module")
def emu():
    return K.emu_backend()


@pytest.fixture(scope="module")
def hip():
    from jssenv_amd.env import HipBackend
    be = HipBackend("cuda:0")
    assert be.lib.jss_backend() == b"hip:gfx950"
    return be


# ---- 1. the hand cases ----------------------------------------------------------------------------------------------------------
def test_hand_case_mirror():
    """the 2 x 2 (a schedule, and the cyclic rank) and the 3 x 2 with ties, on the mirror alone, from arrays written out"""
    const, ops, rank = K.hand_arrays()
    K.check_hand(*K.search.order_eval_reference(const, ops, rank, pair_cap=3, fill=K.FILL), K.FILL)


def test_hand_case_twin(twin):
    K.case_hand(twin)


def test_hand_case_emu(emu):
    K.case_hand(emu)


@pytest.mark.gpu
def test_hand_case_gpu(hip):
    K.case_hand(hip)


# ---- 2. the backends against the mirror ----------------------------------------------------------------------------------------
def test_cases_cover():
    seen = K.what_the_cases_cover()
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("name", NAMES)
def test_against_mirror_twin(twin, name):
    K.case_against_mirror(twin, name)


@pytest.mark.parametrize("name", NAMES)
def test_against_mirror_emu(emu, name):
    K.case_against_mirror(emu, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_against_mirror_gpu(hip, name):
    K.case_against_mirror(hip, name)


def test_apply_twin(twin):
    K.case_apply(twin)


def test_apply_emu(emu):
    K.case_apply(emu)


@pytest.mark.gpu
def test_apply_gpu(hip):
    K.case_apply(hip)


# ---- 3. properties of re-timed rollouts ------------------------------------------------------------------------------------------
def _instance(name):
    return K.syn50x20() if name == "syn50x20" else name


@pytest.mark.parametrize("kind", RULES)
@pytest.mark.parametrize("name", ["ta01", "ta41", "syn50x20"])
def test_properties_twin(twin, name, kind):
    K.case_properties(twin, _instance(name), kind)


@pytest.mark.parametrize("kind", RULES)
@pytest.mark.parametrize("name", ["ta01", "ta41", "syn50x20"])
def test_properties_emu(emu, name, kind):
    K.case_properties(emu, _instance(name), kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", RULES)
@pytest.mark.parametrize("name", ["ta01", "ta41", "syn50x20"])
def test_properties_gpu(hip, name, kind):
    K.case_properties(hip, _instance(name), kind)


def test_unfinished_env_is_refused(twin):
    """the solution of an env in mid-episode holds -1: evaluate_order() refuses it, and only it"""
    from jssenv_amd import BatchedJssEnv
    env = BatchedJssEnv("ta01", batch=2, _backend=twin, seed=4)
    env.reset()
    env.rollout("SPT", n_iter=40, autoreset=False)
    assert not np.asarray(twin.numpy(env.done)).any()
    mk, start = env.evaluate_order(start=True)
    assert mk.tolist() == [-1, -1] and (start == -1).all()
    env.rollout("SPT", n_iter=3 * 225, autoreset=False)
    assert env.evaluate_order().tolist() == [1462, 1462]


# ---- 4. the driver -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", list(K.ANCHORS))
def test_improve_anchors_twin(twin, name, kind):
    """improve is its definition loop for every check_every; the listed makespans, iterations and evaluations; truncated == 0"""
    K.case_driver(twin, name, kind, anchor=K.ANCHORS[(name, kind)])


def test_improve_batch_twin(twin):
    """three instances in one batch (they stop improving at different iterations); a small pair_cap that truncates"""
    K.case_driver(twin, ["ta01", "ta02", "ta11"], "SPT")
    res = K.case_driver(twin, ["ta01", "ta02"], "FIFO", cap=5, check_every=(2,))
    assert res.truncated > 0


def test_improve_emu(emu):
    """the three launches of an iteration under the emulator: ta01 from FIFO (2 improving iterations), 64 candidates per row"""
    res = K.case_driver(emu, "ta01", "FIFO", cap=64, check_every=(1, 8))
    assert (int(res.makespan_before[0]), int(res.makespan[0]), res.iterations, res.evaluations, res.truncated) == (1486, 1455, 2, 35, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", list(K.ANCHORS))
def test_improve_anchors_gpu(hip, name, kind):
    K.case_driver(hip, name, kind, anchor=K.ANCHORS[(name, kind)])


@pytest.mark.gpu
def test_improve_batch_gpu(hip):
    K.case_driver(hip, ["ta01", "ta02", "ta11"], "SPT", check_every=(1, 8))


def test_facade_and_refusals(twin):
    from jssenv_amd import BatchedJssEnv, search
    from jssenv_amd.bucketed import BucketedJssEnv
    from jssenv_amd.facade import JssEnv
    from jssenv_amd.vector import JssVectorEnv
    env = JssEnv({"instance_path": "ta01"}, _backend=twin)
    env.reset()
    assert env.evaluate_order() == -1                                 # nothing scheduled yet
    b = BatchedJssEnv("ta01", batch=1, _backend=twin)
    b.reset()
    b.rollout("SPT", n_iter=3 * 225, autoreset=False)
    sol = np.asarray(twin.numpy(b.solution))[0]
    assert env.evaluate_order(sol) == 1462 and isinstance(env.evaluate_order(sol), int)
    mk, start, pa, pb, found = env.evaluate_order(sol, start=True, pairs=64)
    assert mk == 1462 and start.shape == (15, 15) and found == 19 and (pa[:found] >= 0).all() and (pb[found:] == -1).all()
    assert env.evaluate_order(sol, swap=(int(pa[0]), int(pb[0]))) > 0
    fresh = BatchedJssEnv("ta01", batch=2, _backend=twin)
    with pytest.raises(RuntimeError):
        fresh.evaluate_order()                                       # never reset
    for bad in (dict(rank=np.zeros((1, 15, 14), np.int32)), dict(parents=[[0]]), dict(parents=[0, 0], swaps=([1], [2])),
                dict(swaps=np.zeros((1, 3), np.int32)), dict(pairs=0)):
        with pytest.raises(ValueError):
            b.evaluate_order(**bad)
    for cls in (BucketedJssEnv, JssVectorEnv):
        with pytest.raises(NotImplementedError):
            cls.evaluate_order(None)
    with pytest.raises(NotImplementedError):
        search.improve(object.__new__(BucketedJssEnv))
    half = BatchedJssEnv("ta01", batch=1, _backend=twin)
    half.reset()
    half.rollout("SPT", n_iter=10, autoreset=False)
    with pytest.raises(ValueError):
        search.improve(half)


class _OpenSession:
    closed = False


def test_open_session_is_refused(twin):
    from jssenv_amd import BatchedJssEnv
    env = BatchedJssEnv("ta01", batch=1, _backend=twin)
    env.reset()
    env._session = _OpenSession()
    try:
        with pytest.raises(NotImplementedError):
            env.evaluate_order()
    finally:
        env._session = None


# ---- 5. argument checks and bindings ----------------------------------------------------------------------------------------------
def test_abi_errors_twin(twin):
    K.case_abi_errors(twin)


def test_abi_errors_emu(emu):
    K.case_abi_errors(emu)


@pytest.mark.gpu
def test_abi_errors_gpu(hip):
    K.case_abi_errors(hip)


def test_abi_mirror():
    from jssenv_amd import _abi
    assert _abi.ABI_VERSION == 14 and _abi.ORDER_VERSION == 1 and _abi.ORDER_SYMBOLS == ("jss_order_eval", "jss_order_apply")
    for name in _abi.ORDER_SYMBOLS:
        assert name not in _abi.SYMBOLS + _abi.SEARCH_SYMBOLS + _abi.BEAM_SYMBOLS + _abi.BOUND_SYMBOLS
    header = open(os.path.join(K.ROOT, "include", "jss_order.h")).read()
    assert "#define JSS_ORDER_VERSION 1" in header
    for struct, ints in ((_abi.JssOrder, ("n", "pair_cap")), (_abi.JssOrderApply, ("batch", "jmax", "mmax", "pair_cap"))):
        body = header[header.index("typedef struct " + struct.__name__ + " {"):header.index("} " + struct.__name__ + ";")]
        names = [f for f, _ in struct._fields_]
        where = [min(body.index(t) for t in (f" {f};", f" {f},", f"*{f};") if t in body) for f in names]
        assert where == sorted(where) and len(set(where)) == len(where), struct.__name__
        import ctypes as C
        assert all((t is C.c_int32) == (f in ints) for f, t in struct._fields_)
        assert body.count(";") == len(names) - (3 if struct is _abi.JssOrderApply else 0)   # (batch, jmax, mmax, pair_cap share a line)
    assert "#define JSS_ABI_VERSION 14" in open(os.path.join(K.ROOT, "include", "jss_hip.h")).read()


def test_exports():
    """the two symbols come from libjss_order_hip.so and the twin, and from none of the other three HIP libraries"""
    from jssenv_amd import _abi, build
    build.build_extension()                            # (all four HIP libraries; nothing to do after build())
    for name in _abi.ORDER_SYMBOLS:
        assert name in K.exported(build.ORDER_OUT) and name in K.exported(build.build_cpu_twin())
        for other in (build.OUT, build.BEAM_OUT, build.BOUND_OUT):
            assert name not in K.exported(other)
    for name in ("jss_bound", "jss_beam_select", "jss_step"):
        assert name not in K.exported(build.ORDER_OUT)


# ---- 6. resources -----------------------------------------------------------------------------------------------------------------
def test_order_kernel_resources():
    """libjss_order_hip.so holds exactly its two kernels: no scratch, no spills; the eval kernel's LDS is the dynamic allocation
    the host sizes, at most 64 KB (order_lds_bytes: what a larger shape gets is JSS_E_LDS, see case_abi_errors)"""
    rows = K.order_kernel_rows()
    assert sorted(r[0].split("(")[0] for r in rows) == ["jss_order_apply_kernel", "jss_order_eval_kernel"]
    for _, _, _, vspill, sspill, scratch, lds in rows:
        assert scratch == 0 and vspill == 0 and sspill == 0 and lds <= 64 * 1024
    # the dynamic part, from the header's formula: 100 x 20 and 128 x 40 fit one wavefront's 64 KB
    for jmax, mmax, fits in ((15, 15, True), (100, 20, True), (128, 40, True), (128, 42, False), (128, 64, False)):
        entries8 = (jmax * mmax + 7) // 8 * 8
        assert (12 * entries8 + 1280 <= 64 * 1024) == fits


def test_order_library_is_ignored_by_git():
    out = subprocess.run(["git", "check-ignore", "jssenv_amd/libjss_order_hip.so", "tests/emu/libjss_order_emu.so"], cwd=K.ROOT,
                         capture_output=True, text=True)
    if out.returncode == 128:                          # (not a git checkout: nothing to ask)
        return
    assert out.stdout.split() == ["jssenv_amd/libjss_order_hip.so", "tests/emu/libjss_order_emu.so"]
