"""jss_block_search (include/jss_block.h), BatchedJssEnv.tabu_blocks and search.tabu_search(moves="block"): tabu search over block
insertions scored by head and tail estimates, a whole walk per env in one launch.  On the host against the CPU twin and the
kernel source under the SIMT emulator; on the MI355X against libjss_block_hip.so."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import order_cases as K  # noqa: E402
import tabu_cases as T  # noqa: E402
import block_cases as Bk  # noqa: E402

NAMES = list(Bk.RUNS)


@pytest.fixture(scope="module")
def twin():
    return Bk.twin_backend()


@pytest.fixture(scope="module")
def emu():
    return Bk.emu_backend()


@pytest.fixture(scope="module")
def hip():
    from jssenv_amd.env import HipBackend
    be = HipBackend("cuda:0")
    assert be.lib.jss_backend() == b"hip:gfx950"
    return be


# ---- 1. the backends against the mirror ----------------------------------------------------------------------------------------
def test_cases_are_order_cases_and_the_hand_ones():
    assert set(NAMES) == set(K.CASES) | set(Bk.HAND)
    for name in Bk.HAND:
        env = Bk.case_state(name)["env"]
        assert env.jmax <= 4 and env.mmax <= 3


@pytest.mark.parametrize("name", NAMES)
def test_against_mirror_twin(twin, name):
    Bk.case_against_mirror(twin, name)


@pytest.mark.parametrize("name", NAMES)
def test_against_mirror_emu(emu, name):
    Bk.case_against_mirror(emu, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_against_mirror_gpu(hip, name):
    Bk.case_against_mirror(hip, name)


def test_cyclic_and_unfinished_rows_twin(twin):
    Bk.case_hand_rows(twin)


def test_cyclic_and_unfinished_rows_emu(emu):
    Bk.case_hand_rows(emu)


@pytest.mark.gpu
def test_cyclic_and_unfinished_rows_gpu(hip):
    Bk.case_hand_rows(hip)


# ---- 2. what the references hold ---------------------------------------------------------------------------------------------------
def test_cases_cover():
    """far moves of both kinds, the three screens (the job's own operation on "repeats"), an aspired and a forced move, every stop,
    a cut by reach, a refused and a cyclic row, a refused tenure"""
    seen = Bk.what_the_cases_cover()
    assert all(v > 0 for v in seen.values()), seen


# ---- 3. replay -----------------------------------------------------------------------------------------------------------------------
REPLAYS = [("ta01", "SPT", 60, 8, 0), ("ta01", "random", 40, 0, 1), ("ta41", "FIFO", 30, 5, 2), ("syn50x20", "SPT", 12, 64, 0)]


@pytest.mark.parametrize("name,kind,iters,tenure,reach", REPLAYS)
def test_replay_twin(twin, name, kind, iters, tenure, reach):
    Bk.case_replay(twin, K.syn50x20() if name == "syn50x20" else name, kind, iters, tenure, reach)


def test_replay_emu(emu):
    Bk.case_replay(emu, "ta01", "FIFO", 10, 3, 0)
    Bk.case_replay(emu, "ta01", "FIFO", 6, 3, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind,iters,tenure,reach", REPLAYS)
def test_replay_gpu(hip, name, kind, iters, tenure, reach):
    Bk.case_replay(hip, K.syn50x20() if name == "syn50x20" else name, kind, iters, tenure, reach)


# ---- 4. the anchors --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(Bk.ANCHORS), ids=lambda k: "-".join(str(x) for x in k))
def test_anchors_twin(twin, key):
    """the listed start, best, move and evaluations; the mirror gives them too (checked on the walk of 64 moves: a mirror of 300
    moves takes seconds, and test_against_mirror_* hold the twin to the mirror)"""
    Bk.case_anchor(twin, key, mirror=key[3] <= 64)


def test_anchor_emu(emu):
    Bk.case_anchor(emu, ("ta01", "SPT", 3, 64))


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(Bk.ANCHORS), ids=lambda k: "-".join(str(x) for x in k))
def test_anchors_gpu(hip, key):
    Bk.case_anchor(hip, key)


# ---- 5. the walk earns its keep ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(Bk.EARNS), ids=lambda k: "-".join(str(x) for x in k))
def test_earns_its_keep_twin(twin, key):
    """with as many moves as the swap walk's anchor spent re-timings, from the same start with the same tenure, the block walk's
    best is <= the swap walk's"""
    Bk.case_earns_its_keep(twin, key)


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(Bk.EARNS), ids=lambda k: "-".join(str(x) for x in k))
def test_earns_its_keep_gpu(hip, twin, key):
    Bk.case_earns_its_keep(twin, key)                   # (the twin's figures, which the kernel is to give bit for bit)
    Bk.case_earns_its_keep(hip, key)


# ---- 6. the driver -----------------------------------------------------------------------------------------------------------------
def test_driver_twin(twin):
    """tabu_search(moves="block") is its definition loop; the groups' bests; one instance and a list; targets of every kind"""
    res = Bk.case_driver(twin, ["ta01", "ta02"], walkers=4, iters=30)
    assert not res.optimal.any() and (res.makespan < np.array([1462, 1446])).all()
    Bk.case_driver(twin, "ta01", kind="FIFO", walkers=3, iters=20, tenure=(4, 4), explore=0.0, seed=5, target=None, reach=1)
    res = Bk.case_driver(twin, ["ta01", "ta11"], walkers=2, iters=20, target=[5000, 1], reach=2)
    assert res.optimal.tolist() == [True, False] and res.info[0, 0] == 2


def test_driver_proves_the_one_job_optimal(twin):
    one = K.inst("one", [[1, 0]], [[4, 9]])
    res = Bk.case_driver(twin, one, walkers=2, iters=5)
    assert res.optimal.tolist() == [True] and res.makespan.tolist() == [13]
    res = Bk.case_driver(twin, one, walkers=2, iters=5, target=None)                     # no target: the walk itself finds no arc
    assert res.optimal.tolist() == [True] and (res.info[:, 0] == 1).all()


def test_driver_swap_is_unchanged(twin):
    Bk.case_driver_swap_is_unchanged(twin)


def test_driver_emu(emu):
    """(the emulator backend carries no jss_bound: a walk without a target)"""
    Bk.case_driver(emu, ["ta01", "ta02"], walkers=2, iters=6, target=None)


@pytest.mark.gpu
def test_driver_gpu(hip):
    res = Bk.case_driver(hip, ["ta01", "ta02"], walkers=4, iters=30)
    assert (res.makespan < np.array([1462, 1446])).all()
    Bk.case_driver_swap_is_unchanged(hip)


def test_driver_refusals():
    from jssenv_amd import search
    for bad in (dict(moves="insert"), dict(moves=None), dict(moves="block", reach=-1), dict(moves="block", reach=65536),
                dict(moves="swap", reach=1), dict(reach=2)):
        with pytest.raises(ValueError):
            search.tabu_search("ta01", _backend=Bk.twin_backend(), **bad)


# ---- 7. the env classes ------------------------------------------------------------------------------------------------------------
def test_facade_and_refusals(twin):
    from jssenv_amd import BatchedJssEnv
    from jssenv_amd.bucketed import BucketedJssEnv
    from jssenv_amd.facade import JssEnv
    from jssenv_amd.vector import JssVectorEnv
    env = JssEnv({"instance_path": "ta01"}, _backend=twin)
    env.reset()
    assert env.tabu_blocks()[0] == -1                                 # nothing scheduled yet
    b = K.rolled_out(twin, "ta01", "SPT")
    sol = np.asarray(twin.numpy(b.solution))[0]
    mk, rank, info = env.tabu_blocks(sol, iters=64, tenure=3)
    assert mk == 1361 and isinstance(mk, int) and rank.shape == (15, 15) and info.tolist()[:4] == [0, 64, 50, 1149] and info.shape == (8,)
    mk, rank, info, trace, last, moved = env.tabu_blocks(sol, 64, 3, target=1400, reach=2, trace=True, last=True, log=True)
    assert mk <= 1400 and info[0] == 2 and trace.shape == (64,) and trace[info[1] - 1] == mk and (trace[info[1]:] == -1).all()
    assert moved.shape == (64, 2) and (moved[:info[1]] >= 0).all() and (moved[info[1]:] == -1).all()
    assert env.evaluate_order(last) == mk
    fresh = BatchedJssEnv("ta01", batch=2, _backend=twin)
    with pytest.raises(RuntimeError):
        fresh.tabu_blocks()                                          # never reset
    for bad in (dict(rank=np.zeros((1, 15, 14), np.int32)), dict(iters=-1), dict(iters=65537), dict(tenure=65), dict(tenure=-1),
                dict(tenure=[1, 2]), dict(target=[1, 2]), dict(reach=-1), dict(reach=65536)):
        with pytest.raises(ValueError):
            b.tabu_blocks(**bad)
    for cls in (BucketedJssEnv, JssVectorEnv):
        with pytest.raises(NotImplementedError):
            cls.tabu_blocks(None)


class _OpenSession:
    closed = False


def test_open_session_is_refused(twin):
    from jssenv_amd import BatchedJssEnv
    env = BatchedJssEnv("ta01", batch=1, _backend=twin)
    env.reset()
    env._session = _OpenSession()
    try:
        with pytest.raises(NotImplementedError):
            env.tabu_blocks()
    finally:
        env._session = None


# ---- 8. argument checks and bindings ----------------------------------------------------------------------------------------------
def test_abi_errors_twin(twin):
    Bk.case_abi_errors(twin)


def test_abi_errors_emu(emu):
    Bk.case_abi_errors(emu)


@pytest.mark.gpu
def test_abi_errors_gpu(hip):
    Bk.case_abi_errors(hip)


def test_abi_mirror():
    import ctypes as C
    import re
    from jssenv_amd import _abi
    assert _abi.ABI_VERSION == 14 and _abi.ORDER_VERSION == 1 and _abi.TABU_VERSION == 1 and _abi.BLOCK_VERSION == 1
    assert _abi.BLOCK_SYMBOLS == ("jss_block_search",) and _abi.TABU_SYMBOLS == ("jss_tabu_search",) and _abi.TABU_NI == 4
    assert _abi.BLOCK_SYMBOLS[0] not in (_abi.SYMBOLS + _abi.SEARCH_SYMBOLS + _abi.BEAM_SYMBOLS + _abi.BOUND_SYMBOLS + _abi.ORDER_SYMBOLS
                                         + _abi.TABU_SYMBOLS)
    header = open(os.path.join(K.ROOT, "include", "jss_block.h")).read()
    assert "#define JSS_BLOCK_VERSION 1" in header and f"#define JSS_BLOCK_NI {_abi.BLOCK_NI}" in header and _abi.BLOCK_NI == 8
    body = header[header.index("typedef struct JssBlock {"):header.index("} JssBlock;")]
    names = [f for f, _ in _abi.JssBlock._fields_]
    where = [min(body.index(t) for t in (f" {f};", f"*{f};") if t in body) for f in names]
    assert where == sorted(where) and len(set(where)) == len(where)
    assert re.sub(r"/\*.*?\*/", "", body).count(";") == len(names) == 12        # one member per field, and no others
    assert all((t is C.c_int32) == (f in ("iters", "tenure", "reach")) for f, t in _abi.JssBlock._fields_)
    assert "#define JSS_TABU_VERSION 1" in open(os.path.join(K.ROOT, "include", "jss_tabu.h")).read()


def test_exports():
    """the symbol comes from libjss_block_hip.so and the twin, and from none of the other five HIP libraries, none of whose
    symbols is in the new one"""
    from jssenv_amd import _abi, build
    build.build_extension()                            # (all six HIP libraries; nothing to do after build())
    name = _abi.BLOCK_SYMBOLS[0]
    assert name in K.exported(build.BLOCK_OUT) and name in K.exported(build.build_cpu_twin())
    for other in (build.OUT, build.BEAM_OUT, build.BOUND_OUT, build.ORDER_OUT, build.TABU_OUT):
        assert name not in K.exported(other)
    for other in _abi.SYMBOLS + _abi.SEARCH_SYMBOLS + _abi.BEAM_SYMBOLS + _abi.BOUND_SYMBOLS + _abi.ORDER_SYMBOLS + _abi.TABU_SYMBOLS:
        assert other not in K.exported(build.BLOCK_OUT), other


# ---- 9. resources -----------------------------------------------------------------------------------------------------------------
def test_block_kernel_resources():
    """libjss_block_hip.so holds exactly its one kernel: no scratch, no spills; its LDS is the dynamic allocation the host sizes,
    at most 64 KB per wavefront (block_lds_bytes: what a larger shape gets is JSS_E_LDS, see case_abi_errors)"""
    rows = Bk.block_kernel_rows()
    assert [r[0].split("(")[0] for r in rows] == ["jss_block_kernel"]
    for _, _, _, vspill, sspill, scratch, lds in rows:
        assert scratch == 0 and vspill == 0 and sspill == 0 and lds <= 64 * 1024
    for jmax, mmax, fits in ((15, 15, True), (100, 20, True), (128, 27, True), (128, 28, False), (128, 64, False)):
        entries8 = (jmax * mmax + 7) // 8 * 8
        assert (18 * entries8 + 1280 <= 64 * 1024) == fits


def test_block_library_is_ignored_by_git():
    out = subprocess.run(["git", "check-ignore", "jssenv_amd/libjss_block_hip.so", "tests/emu/libjss_block_emu.so"], cwd=K.ROOT,
                         capture_output=True, text=True)
    if out.returncode == 128:                          # (not a git checkout: nothing to ask)
        return
    assert out.stdout.split() == ["jssenv_amd/libjss_block_hip.so", "tests/emu/libjss_block_emu.so"]
