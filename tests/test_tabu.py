"""jss_tabu_search (include/jss_tabu.h), BatchedJssEnv.tabu and search.tabu_search: tabu search over the swap neighbourhood of
machine orders, a whole walk per env in one launch.  On the host against the CPU twin and the kernel source under the SIMT
emulator; on the MI355X against libjss_tabu_hip.so."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import order_cases as K  # noqa: E402
import tabu_cases as T  # noqa: E402

NAMES = list(T.RUNS)


@pytest.fixture(scope="module")
def twin():
    return T.twin_backend()


@pytest.fixture(scope="module")
def emu():
    return T.emu_backend()


@pytest.fixture(scope="module")
def hip():
    from jssenv_amd.env import HipBackend
    be = HipBackend("cuda:0")
    assert be.lib.jss_backend() == b"hip:gfx950"
    return be


# ---- 1. the backends against the mirror ----------------------------------------------------------------------------------------
def test_cases_cover():
    """the references hold an aspirated tabu move, a forced move, every stop, a refused and a cyclic row, a refused tenure"""
    seen = T.what_the_cases_cover()
    assert all(v > 0 for v in seen.values()), seen


def test_cases_are_order_cases():
    assert set(NAMES) == set(K.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_against_mirror_twin(twin, name):
    T.case_against_mirror(twin, name)


@pytest.mark.parametrize("name", NAMES)
def test_against_mirror_emu(emu, name):
    T.case_against_mirror(emu, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_against_mirror_gpu(hip, name):
    T.case_against_mirror(hip, name)


def test_cyclic_and_unfinished_rows_twin(twin):
    T.case_hand_rows(twin)


def test_cyclic_and_unfinished_rows_emu(emu):
    T.case_hand_rows(emu)


@pytest.mark.gpu
def test_cyclic_and_unfinished_rows_gpu(hip):
    T.case_hand_rows(hip)


# ---- 2. the anchors --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(T.ANCHORS), ids=lambda k: "-".join(str(x) for x in k))
def test_anchors_twin(twin, key):
    """the listed start, best, move and evaluations; the mirror gives them too (checked on the walk of 64 moves: a mirror of 300
    moves takes many seconds, and test_against_mirror_* hold the twin to the mirror)"""
    T.case_anchor(twin, key, mirror=key[3] <= 64)


def test_target_anchors_twin(twin):
    T.case_target_anchors(twin, mirror=True)


def test_mixed_batch_twin(twin):
    T.case_mixed(twin)


def test_anchor_emu(emu):
    T.case_anchor(emu, ("ta01", "SPT", 3, 64))


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(T.ANCHORS), ids=lambda k: "-".join(str(x) for x in k))
def test_anchors_gpu(hip, key):
    T.case_anchor(hip, key)


@pytest.mark.gpu
def test_target_anchors_gpu(hip):
    T.case_target_anchors(hip)


@pytest.mark.gpu
def test_mixed_batch_gpu(hip):
    T.case_mixed(hip)


# ---- 3. properties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,iters,tenure", [("ta01", "SPT", 60, 8), ("ta01", "random", 60, 0), ("ta41", "FIFO", 30, 5),
                                                    ("syn50x20", "SPT", 12, 64)])
def test_properties_twin(twin, name, kind, iters, tenure):
    T.case_properties(twin, K.syn50x20() if name == "syn50x20" else name, kind, iters, tenure)


def test_properties_emu(emu):
    T.case_properties(emu, "ta01", "FIFO", 10, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind,iters,tenure", [("ta01", "SPT", 60, 8), ("ta01", "random", 60, 0), ("ta41", "FIFO", 30, 5),
                                                    ("syn50x20", "SPT", 12, 64)])
def test_properties_gpu(hip, name, kind, iters, tenure):
    T.case_properties(hip, K.syn50x20() if name == "syn50x20" else name, kind, iters, tenure)


@pytest.mark.parametrize("name,kind", list(K.ANCHORS))
def test_descent_is_the_first_moves_twin(twin, name, kind):
    T.case_descent(twin, name, kind)


def test_descent_is_the_first_moves_emu(emu):
    T.case_descent(emu, "ta01", "FIFO", tenures=(3,))


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", list(K.ANCHORS))
def test_descent_is_the_first_moves_gpu(hip, name, kind):
    T.case_descent(hip, name, kind)


# ---- 4. the driver -----------------------------------------------------------------------------------------------------------------
def test_driver_twin(twin):
    """tabu_search is its definition loop; the groups' bests; one instance and a list; targets of every kind"""
    res = T.case_driver(twin, ["ta01", "ta02"], walkers=4, iters=30)
    assert not res.optimal.any() and (res.makespan < np.array([1462, 1446])).all()
    T.case_driver(twin, "ta01", kind="FIFO", walkers=3, iters=20, tenure=(4, 4), explore=0.0, seed=5, target=None)
    res = T.case_driver(twin, ["ta01", "ta11"], walkers=2, iters=20, target=[5000, 1])
    assert res.optimal.tolist() == [True, False] and res.info[0, 0] == 2


def test_driver_proves_the_one_job_optimal(twin):
    one = K.inst("one", [[1, 0]], [[4, 9]])
    res = T.case_driver(twin, one, walkers=2, iters=5)
    assert res.optimal.tolist() == [True] and res.makespan.tolist() == [13]
    res = T.case_driver(twin, one, walkers=2, iters=5, target=None)                      # no target: the walk itself finds no arc
    assert res.optimal.tolist() == [True] and (res.info[:, 0] == 1).all()


def test_driver_emu(emu):
    """(the emulator backend carries no jss_bound: a walk without a target)"""
    T.case_driver(emu, ["ta01", "ta02"], walkers=2, iters=6, target=None)


@pytest.mark.gpu
def test_driver_gpu(hip):
    res = T.case_driver(hip, ["ta01", "ta02"], walkers=4, iters=30)
    assert (res.makespan < np.array([1462, 1446])).all()


def test_driver_refusals():
    from jssenv_amd import search
    from jssenv_amd.bucketed import BucketedJssEnv
    with pytest.raises(NotImplementedError):
        search.tabu_search(object.__new__(BucketedJssEnv))
    for bad in (dict(walkers=0), dict(tenure=(5, 65)), dict(tenure=(6, 5)), dict(target="upper_bound")):
        with pytest.raises(ValueError):
            search.tabu_search("ta01", _backend=T.twin_backend(), **bad)
    with pytest.raises(ValueError):
        search.tabu_search([], _backend=T.twin_backend())


# ---- 5. the env classes ------------------------------------------------------------------------------------------------------------
def test_facade_and_refusals(twin):
    from jssenv_amd import BatchedJssEnv
    from jssenv_amd.bucketed import BucketedJssEnv
    from jssenv_amd.facade import JssEnv
    from jssenv_amd.vector import JssVectorEnv
    env = JssEnv({"instance_path": "ta01"}, _backend=twin)
    env.reset()
    assert env.tabu()[0] == -1                                        # nothing scheduled yet
    b = K.rolled_out(twin, "ta01", "SPT")
    sol = np.asarray(twin.numpy(b.solution))[0]
    mk, rank, info = env.tabu(sol, iters=64, tenure=3)
    assert mk == 1361 and isinstance(mk, int) and rank.shape == (15, 15) and info.tolist() == [0, 64, 50, 990]
    mk, rank, info, trace, last = env.tabu(sol, 64, 3, target=1400, trace=True, last=True)
    assert mk <= 1400 and info[0] == 2 and trace.shape == (64,) and trace[info[1] - 1] == mk and (trace[info[1]:] == -1).all()
    assert env.evaluate_order(last) == mk
    fresh = BatchedJssEnv("ta01", batch=2, _backend=twin)
    with pytest.raises(RuntimeError):
        fresh.tabu()                                                 # never reset
    for bad in (dict(rank=np.zeros((1, 15, 14), np.int32)), dict(iters=-1), dict(iters=65537), dict(tenure=65), dict(tenure=-1),
                dict(tenure=[1, 2]), dict(target=[1, 2])):
        with pytest.raises(ValueError):
            b.tabu(**bad)
    for cls in (BucketedJssEnv, JssVectorEnv):
        with pytest.raises(NotImplementedError):
            cls.tabu(None)


class _OpenSession:
    closed = False


def test_open_session_is_refused(twin):
    from jssenv_amd import BatchedJssEnv
    env = BatchedJssEnv("ta01", batch=1, _backend=twin)
    env.reset()
    env._session = _OpenSession()
    try:
        with pytest.raises(NotImplementedError):
            env.tabu()
    finally:
        env._session = None


# ---- 6. argument checks and bindings ----------------------------------------------------------------------------------------------
def test_abi_errors_twin(twin):
    T.case_abi_errors(twin)


def test_abi_errors_emu(emu):
    T.case_abi_errors(emu)


@pytest.mark.gpu
def test_abi_errors_gpu(hip):
    T.case_abi_errors(hip)


def test_abi_mirror():
    import ctypes as C
    from jssenv_amd import _abi
    assert _abi.ABI_VERSION == 14 and _abi.ORDER_VERSION == 1 and _abi.TABU_VERSION == 1 and _abi.TABU_SYMBOLS == ("jss_tabu_search",)
    assert _abi.TABU_SYMBOLS[0] not in _abi.SYMBOLS + _abi.SEARCH_SYMBOLS + _abi.BEAM_SYMBOLS + _abi.BOUND_SYMBOLS + _abi.ORDER_SYMBOLS
    header = open(os.path.join(K.ROOT, "include", "jss_tabu.h")).read()
    assert "#define JSS_TABU_VERSION 1" in header and f"#define JSS_TABU_NI {_abi.TABU_NI}" in header
    body = header[header.index("typedef struct JssTabu {"):header.index("} JssTabu;")]
    names = [f for f, _ in _abi.JssTabu._fields_]
    where = [min(body.index(t) for t in (f" {f};", f"*{f};") if t in body) for f in names]
    import re
    assert where == sorted(where) and len(set(where)) == len(where)
    assert re.sub(r"/\*.*?\*/", "", body).count(";") == len(names)              # one member per field, and no others
    assert all((t is C.c_int32) == (f in ("iters", "tenure")) for f, t in _abi.JssTabu._fields_)
    assert "#define JSS_ABI_VERSION 14" in open(os.path.join(K.ROOT, "include", "jss_hip.h")).read()
    assert "#define JSS_ORDER_VERSION 1" in open(os.path.join(K.ROOT, "include", "jss_order.h")).read()


def test_exports():
    """the symbol comes from libjss_tabu_hip.so and the twin, and from none of the other four HIP libraries, none of whose symbols
    is in the new one"""
    from jssenv_amd import _abi, build
    build.build_extension()                            # (all five HIP libraries; nothing to do after build())
    name = _abi.TABU_SYMBOLS[0]
    assert name in K.exported(build.TABU_OUT) and name in K.exported(build.build_cpu_twin())
    for other in (build.OUT, build.BEAM_OUT, build.BOUND_OUT, build.ORDER_OUT):
        assert name not in K.exported(other)
    for other in _abi.SYMBOLS + _abi.SEARCH_SYMBOLS + _abi.BEAM_SYMBOLS + _abi.BOUND_SYMBOLS + _abi.ORDER_SYMBOLS:
        assert other not in K.exported(build.TABU_OUT), other


# ---- 7. resources -----------------------------------------------------------------------------------------------------------------
def test_tabu_kernel_resources():
    """libjss_tabu_hip.so holds exactly its one kernel: no scratch, no spills; its LDS is the dynamic allocation the host sizes,
    at most 64 KB per wavefront (tabu_lds_bytes: what a larger shape gets is JSS_E_LDS, see case_abi_errors)"""
    rows = T.tabu_kernel_rows()
    assert [r[0].split("(")[0] for r in rows] == ["jss_tabu_kernel"]
    for _, _, _, vspill, sspill, scratch, lds in rows:
        assert scratch == 0 and vspill == 0 and sspill == 0 and lds <= 64 * 1024
    for jmax, mmax, fits in ((15, 15, True), (100, 20, True), (128, 40, True), (128, 42, False), (128, 64, False)):
        entries8 = (jmax * mmax + 7) // 8 * 8
        assert (12 * entries8 + 1280 <= 64 * 1024) == fits


def test_tabu_library_is_ignored_by_git():
    out = subprocess.run(["git", "check-ignore", "jssenv_amd/libjss_tabu_hip.so", "tests/emu/libjss_tabu_emu.so"], cwd=K.ROOT,
                         capture_output=True, text=True)
    if out.returncode == 128:                          # (not a git checkout: nothing to ask)
        return
    assert out.stdout.split() == ["jssenv_amd/libjss_tabu_hip.so", "tests/emu/libjss_tabu_emu.so"]
