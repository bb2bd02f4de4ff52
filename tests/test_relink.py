"""jss_relink_walk (include/jss_relink.h), BatchedJssEnv.relink / order_distance and search.relink_search: the distance between
two machine orders and a walk from the one towards the other through orders that all have schedules, a whole walk per env in one
launch, and the population driver over it.  On the host against the CPU twin and the kernel source under the SIMT emulator; on the
MI355X against libjss_relink_hip.so."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import order_cases as K  # noqa: E402
import block_cases as Bk  # noqa: E402
import relink_cases as R  # noqa: E402

NAMES = list(R.RUNS)
TA01 = [k for k in R.ANCHORS if k[0] == "ta01"]
ARRIVALS = ([(name, kind) for name in R.SMALL for kind in ("asc", "desc")]
            + [("fallback", "other"), ("retry", "other"), ("chain", "other"), ("repeats", "other")])


@pytest.fixture(scope="module")
def twin():
    return R.twin_backend()


@pytest.fixture(scope="module")
def emu():
    return R.emu_backend()


@pytest.fixture(scope="module")
def hip():
    from jssenv_amd.env import HipBackend
    be = HipBackend("cuda:0")
    assert be.lib.jss_backend() == b"hip:gfx950"
    return be


# ---- 1. the backends against the mirror ----------------------------------------------------------------------------------------
def test_cases_are_block_cases_and_the_hand_one():
    assert set(NAMES) == set(Bk.CASES) | {"fallback", "retry"} and set(Bk.CASES) == set(K.CASES) | {"chain"}
    assert [(R.case_state(name)["env"].jmax, R.case_state(name)["env"].mmax) for name in ("fallback", "retry")] == [(3, 5), (3, 4)]


@pytest.mark.parametrize("name", NAMES)
def test_against_mirror_twin(twin, name):
    R.case_against_mirror(twin, name)


@pytest.mark.parametrize("name", NAMES)
def test_against_mirror_emu(emu, name):
    R.case_against_mirror(emu, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_against_mirror_gpu(hip, name):
    R.case_against_mirror(hip, name)


def test_refused_rows_twin(twin):
    R.case_refused_rows(twin)


def test_refused_rows_emu(emu):
    R.case_refused_rows(emu)


@pytest.mark.gpu
def test_refused_rows_gpu(hip):
    R.case_refused_rows(hip)


def test_cases_cover():
    """a move without a sure candidate, every stop at move 0 and in mid-walk, no eligible order, a refused and a cyclic row;
    `retries` is reported and not required here (test_retry_* hold the one known walk that swaps a candidate back)"""
    seen = R.what_the_cases_cover()
    print("retries over all cases:", seen.pop("retries"))
    assert all(v > 0 for v in seen.values()), seen


# ---- 2. arrival ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", ARRIVALS + [("ta01", "desc"), ("J65", "asc"), ("table-of-env", "desc")])
def test_arrival_twin(twin, name, kind):
    R.case_arrival(twin, name, kind)


@pytest.mark.parametrize("name,kind", ARRIVALS)
def test_arrival_emu(emu, name, kind):
    R.case_arrival(emu, name, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", ARRIVALS + [("ta01", "desc"), ("J65", "asc"), ("table-of-env", "desc")])
def test_arrival_gpu(hip, name, kind):
    R.case_arrival(hip, name, kind)


# ---- 3. replay -------------------------------------------------------------------------------------------------------------------
REPLAYS = [("ta01", "SPT", "FIFO", 0), ("ta01", "SPT", "FIFO", 30), ("hand", R.HAND_SOURCE, R.HAND_GUIDE, 0), ("hand", R.HAND_GUIDE, R.HAND_SOURCE, 2),
           ("hand", R.HAND_SOURCE, R.HAND_GUIDE, 4)]
REPLAY_IDS = ["ta01", "ta01-margin30", "hand-forward", "hand-back-margin2", "hand-no-eligible"]


def _replay(be, name, source, guide, margin):
    return R.case_replay(be, R.hand_instance() if name == "hand" else name, source, guide, margin)


@pytest.mark.parametrize("name,source,guide,margin", REPLAYS, ids=REPLAY_IDS)
def test_replay_twin(twin, name, source, guide, margin):
    info, _ = _replay(twin, name, source, guide, margin)
    assert (info[2] == -1) == (margin == 4)                           # 6 moves: no t has t >= 4 and 6 - t >= 4


def test_replay_emu(emu):
    _replay(emu, "hand", R.HAND_SOURCE, R.HAND_GUIDE, 0)
    _replay(emu, "hand", R.HAND_GUIDE, R.HAND_SOURCE, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("name,source,guide,margin", REPLAYS, ids=REPLAY_IDS)
def test_replay_gpu(hip, name, source, guide, margin):
    _replay(hip, name, source, guide, margin)


# ---- 4. the anchors --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(R.ANCHORS), ids=lambda k: "-".join(k))
def test_anchors_twin(twin, key):
    """the listed distance, makespans of both ends, lowest and highest on the path; the mirror gives one of ta01's too (its 134
    moves take a few seconds; test_against_mirror_* hold the twin to the mirror)"""
    R.case_anchor(twin, key, mirror=key == ("ta01", "MWR", "FIFO"))


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(R.ANCHORS), ids=lambda k: "-".join(k))
def test_anchors_gpu(hip, key):
    R.case_anchor(hip, key)


def test_hand_walks_twin(twin):
    R.case_hand_walks(twin, mirror=True)


def test_hand_walks_emu(emu):
    R.case_hand_walks(emu)


@pytest.mark.gpu
def test_hand_walks_gpu(hip):
    R.case_hand_walks(hip)


def test_retry_twin(twin):
    """the walk the seeded search found: one candidate swapped back, on the twin and on the mirror"""
    R.case_retry(twin, mirror=True)


def test_retry_emu(emu):
    R.case_retry(emu)


@pytest.mark.gpu
def test_retry_gpu(hip):
    R.case_retry(hip)


# ---- 5. a seeded search for a retry ----------------------------------------------------------------------------------------------
def test_seeded_search_twin():
    """3 000 random tiny walks, repeats and durations of 0 among them: every one arrives, the twin is the mirror on every 50th.
    The sums are reported; a walk with retries > 0 becomes a case (seed 2024 gives one: relink_cases.RETRY_*)"""
    from jssenv_amd.env import CpuBackend
    t0 = time.time()
    total, with_retry = R.case_seeded_search(CpuBackend(threads=1), 3000)   # (B = 1 calls: no thread team to wake per call)
    print("seeded search: info sums (stop, moves, best_move, dist0, dist, candidates, fallbacks, retries)", total.tolist(),
          "walks with a retry:", len(with_retry), f"{time.time() - t0:.1f} s")
    assert total[6] > 0 and total[1] == total[3] and total[4] == 0    # the fallback is reached; every walk arrived
    for inst, src, gd in with_retry:
        print("retry:", inst.machine.tolist(), inst.duration.tolist(), src.tolist(), gd.tolist())


# ---- 6. the driver ---------------------------------------------------------------------------------------------------------------
def test_driver_twin(twin):
    """relink_search is its definition loop; history never rises; one instance and a list"""
    R.case_driver(twin, "ta01", walkers=4, iters=30)
    res = R.case_driver(twin, ["ta01", "ta11"], walkers=4, iters=30)
    assert res.distance.shape == (8, 2) and (res.distance.reshape(2, 4, 2).min(axis=1) == 0).all()     # the elites
    R.case_driver(twin, "ta01", kind="FIFO", walkers=3, iters=12, rounds=3, share=(1, 3), tenure=(4, 4), explore=0.3, seed=5, target=None, reach=1)
    res = R.case_driver(twin, ["ta01", "ta11"], walkers=2, iters=10, rounds=1, target=[5000, 1])
    assert res.optimal.tolist() == [True, False] and (res.distance[:2] >= 0).all()


def test_driver_rounds_0_twin(twin):
    R.case_driver_rounds_0(twin, "ta01", walkers=4, iters=30)
    R.case_driver_rounds_0(twin, ["ta01", "ta11"], walkers=4, iters=30, target=None)


def test_driver_emu(emu):
    """(the emulator backend carries no jss_bound: walks without a target)"""
    R.case_driver(emu, ["ta01", "ta02"], walkers=2, iters=4, rounds=1, target=None)


@pytest.mark.gpu
def test_driver_gpu(hip):
    R.case_driver(hip, ["ta01", "ta11"], walkers=4, iters=30)
    R.case_driver_rounds_0(hip, "ta01", walkers=4, iters=30)


def test_driver_refusals(twin):
    from jssenv_amd import BatchedJssEnv, search
    for bad in (dict(rounds=-1), dict(share=(2, 1)), dict(share=(1, 0)), dict(share=(-1, 2)), dict(walkers=0), dict(reach=-1),
                dict(tenure=(3, 65)), dict(target="upper")):
        with pytest.raises(ValueError):
            search.relink_search("ta01", _backend=twin, **bad)
    with pytest.raises(NotImplementedError):
        search.relink_search(BatchedJssEnv("ta01", batch=2, _backend=twin))


# ---- 7. the env classes ------------------------------------------------------------------------------------------------------------
def test_facade_and_refusals(twin):
    from jssenv_amd import BatchedJssEnv
    from jssenv_amd.bucketed import BucketedJssEnv
    from jssenv_amd.facade import JssEnv
    from jssenv_amd.vector import JssVectorEnv
    n = lambda x: np.asarray(twin.numpy(x))   # noqa: E731
    spt, fifo = (n(K.rolled_out(twin, "ta01", kind).solution)[0] for kind in ("SPT", "FIFO"))
    env = JssEnv({"instance_path": "ta01"}, _backend=twin)
    env.reset()
    assert env.relink(None, fifo)[0] == -1 and env.order_distance(None, fifo) == -1     # nothing scheduled yet
    assert env.order_distance(spt, fifo) == 204 == env.order_distance(fifo, spt) and env.order_distance(spt, spt) == 0
    best, best_rank, last, last_rank, info = env.relink(spt, fifo)
    assert (best, last) == (1440, 1486) and isinstance(best, int) and isinstance(last, int) and best_rank.shape == (15, 15)
    assert info.tolist() == [1, 204, 92, 204, 0] + info.tolist()[5:] and info.shape == (8,) and env.evaluate_order(best_rank) == 1440
    best, best_rank, last, last_rank, info, trace, moved = env.relink(spt, fifo, steps=150, until=102, margin=5, trace=True, log=True)
    assert info[:5].tolist() == [2, 102, 92, 204, 102] and trace.shape == (150,) and (trace[102:] == -1).all() and trace[101] == last
    assert moved.shape == (150, 2) and (moved[:102] >= 0).all() and (moved[102:] == -1).all() and env.evaluate_order(last_rank) == last
    out = env.relink(spt, fifo, steps=3, last=False)
    assert out[2] is None and out[3] is None and out[4][:2].tolist() == [0, 3]
    b = K.rolled_out(twin, "ta01", "SPT")
    assert n(b.relink(None, fifo[None])[0]).tolist() == [1440] and n(b.order_distance(None, fifo[None])).tolist() == [204]
    assert n(b.relink(None, fifo[None], until=np.array([150], np.int32))[4])[0, :5].tolist() == [2, 54, n(b.relink(None, fifo[None], until=150)[4])[0, 2], 204, 150]
    fresh = BatchedJssEnv("ta01", batch=2, _backend=twin)
    with pytest.raises(RuntimeError):
        fresh.relink(None, fifo[None])                               # never reset
    for bad in (dict(rank=np.zeros((1, 15, 14), np.int32)), dict(guide=np.zeros((1, 14, 15), np.int32)), dict(guide=None), dict(steps=-1),
                dict(steps=65537), dict(until=-1), dict(until=[1, 2]), dict(margin=-1)):
        with pytest.raises(ValueError):
            b.relink(**dict(dict(rank=None, guide=fifo[None]), **bad))
    for cls in (BucketedJssEnv, JssVectorEnv):
        for call in (cls.relink, cls.order_distance):
            with pytest.raises(NotImplementedError):
                call(None)


class _OpenSession:
    closed = False


def test_open_session_is_refused(twin):
    from jssenv_amd import BatchedJssEnv
    env = BatchedJssEnv("ta01", batch=1, _backend=twin)
    env.reset()
    env._session = _OpenSession()
    try:
        for call in (env.relink, env.order_distance):
            with pytest.raises(NotImplementedError):
                call(None, np.zeros((1, 15, 15), np.int32))
    finally:
        env._session = None


# ---- 8. argument checks and bindings ----------------------------------------------------------------------------------------------
def test_abi_errors_twin(twin):
    R.case_abi_errors(twin)


def test_abi_errors_emu(emu):
    R.case_abi_errors(emu)


@pytest.mark.gpu
def test_abi_errors_gpu(hip):
    R.case_abi_errors(hip)


def test_abi_mirror():
    import ctypes as C
    import re
    from jssenv_amd import _abi
    assert _abi.ABI_VERSION == 14 and _abi.ORDER_VERSION == 1 and _abi.TABU_VERSION == 1 and _abi.BLOCK_VERSION == 1 and _abi.RELINK_VERSION == 1
    assert _abi.RELINK_SYMBOLS == ("jss_relink_walk",) and _abi.RELINK_NI == 8 and _abi.RELINK_MAX_STEPS == 65536
    assert _abi.RELINK_SYMBOLS[0] not in (_abi.SYMBOLS + _abi.SEARCH_SYMBOLS + _abi.BEAM_SYMBOLS + _abi.BOUND_SYMBOLS + _abi.ORDER_SYMBOLS
                                          + _abi.TABU_SYMBOLS + _abi.BLOCK_SYMBOLS)
    header = open(os.path.join(K.ROOT, "include", "jss_relink.h")).read()
    assert "#define JSS_RELINK_VERSION 1" in header and f"#define JSS_RELINK_NI {_abi.RELINK_NI}" in header
    body = header[header.index("typedef struct JssRelink {"):header.index("} JssRelink;")]
    names = [f for f, _ in _abi.JssRelink._fields_]
    where = [min(body.index(t) for t in (f" {f};", f"*{f};") if t in body) for f in names]
    assert where == sorted(where) and len(set(where)) == len(where)
    assert re.sub(r"/\*.*?\*/", "", body).count(";") == len(names) == 13        # one member per field, and no others
    assert all((t is C.c_int32) == (f in ("steps", "until", "margin")) for f, t in _abi.JssRelink._fields_)
    assert "#define JSS_BLOCK_VERSION 1" in open(os.path.join(K.ROOT, "include", "jss_block.h")).read()


def test_exports():
    """the symbol comes from libjss_relink_hip.so and the twin, and from none of the other six HIP libraries, none of whose
    symbols is in the new one"""
    from jssenv_amd import _abi, build
    build.build_extension()                            # (all seven HIP libraries; nothing to do after build())
    name = _abi.RELINK_SYMBOLS[0]
    assert name in K.exported(build.RELINK_OUT) and name in K.exported(build.build_cpu_twin())
    for other in (build.OUT, build.BEAM_OUT, build.BOUND_OUT, build.ORDER_OUT, build.TABU_OUT, build.BLOCK_OUT):
        assert name not in K.exported(other)
    for other in (_abi.SYMBOLS + _abi.SEARCH_SYMBOLS + _abi.BEAM_SYMBOLS + _abi.BOUND_SYMBOLS + _abi.ORDER_SYMBOLS + _abi.TABU_SYMBOLS
                  + _abi.BLOCK_SYMBOLS):
        assert other not in K.exported(build.RELINK_OUT), other


# ---- 9. resources -----------------------------------------------------------------------------------------------------------------
def test_relink_kernel_resources():
    """libjss_relink_hip.so holds exactly its one kernel: no scratch, no spills; its LDS is the dynamic allocation the host sizes,
    at most 64 KB per wavefront (relink_lds_bytes: what a larger shape gets is JSS_E_LDS, see case_abi_errors)"""
    rows = R.relink_kernel_rows()
    assert [r[0].split("(")[0] for r in rows] == ["jss_relink_kernel"]
    for _, _, _, vspill, sspill, scratch, lds in rows:
        assert scratch == 0 and vspill == 0 and sspill == 0 and lds <= 64 * 1024
    for jmax, mmax, fits in ((15, 15, True), (100, 20, True), (128, 28, True), (128, 29, False), (128, 64, False)):
        entries8 = (jmax * mmax + 7) // 8 * 8
        assert (18 * entries8 + 1024 <= 64 * 1024) == fits


def test_relink_library_is_ignored_by_git():
    out = subprocess.run(["git", "check-ignore", "jssenv_amd/libjss_relink_hip.so", "tests/emu/libjss_relink_emu.so"], cwd=K.ROOT,
                         capture_output=True, text=True)
    if out.returncode == 128:                          # (not a git checkout: nothing to ask)
        return
    assert out.stdout.split() == ["jssenv_amd/libjss_relink_hip.so", "tests/emu/libjss_relink_emu.so"]
