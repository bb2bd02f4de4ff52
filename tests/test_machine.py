"""jss_machine_relax and jss_bottleneck_build (include/jss_machine.h), BatchedJssEnv.relax_machines / bottleneck and
search.bottleneck_search: the one-machine relaxations of partial selections -- heads, tails, Jackson's preemptive bound, Schrage's
schedule -- and whole shifting bottleneck constructions, one candidate per wavefront in one launch.  On the host against the CPU
twin and the kernel source under the SIMT emulator; on the MI355X against libjss_machine_hip.so."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import order_cases as K  # noqa: E402
import machine_cases as S  # noqa: E402

NAMES = list(S.CASES)


@pytest.fixture(scope="module")
def twin():
    return S.twin_backend()


@pytest.fixture(scope="module")
def emu():
    return S.emu_backend()


@pytest.fixture(scope="module")
def hip():
    from jssenv_amd.env import HipBackend
    be = HipBackend("cuda:0")
    assert be.lib.jss_backend() == b"hip:gfx950"
    return be


# ---- 1. the backends against the mirror ----------------------------------------------------------------------------------------
def test_cases():
    assert set(NAMES) == set(S.REUSED) | {"hand", "zeros", "J1", "M1", "J64", "J128", "one-machine", "m64"}
    S.what_the_cases_cover()


@pytest.mark.parametrize("name", NAMES)
def test_against_mirror_twin(twin, name):
    S.case_against_mirror(twin, name)


@pytest.mark.parametrize("name", NAMES)
def test_against_mirror_emu(emu, name):
    S.case_against_mirror(emu, name, light=1 if name in S.SMALL else 2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_against_mirror_gpu(hip, name):
    S.case_against_mirror(hip, name)


def test_hand_twin(twin):
    S.case_hand(twin, mirror=True)


def test_hand_emu(emu):
    S.case_hand(emu)


@pytest.mark.gpu
def test_hand_gpu(hip):
    S.case_hand(hip)


def test_cyclic_build_twin(twin):
    S.case_cyclic_build(twin)


def test_cyclic_build_emu(emu):
    S.case_cyclic_build(emu)


@pytest.mark.gpu
def test_cyclic_build_gpu(hip):
    S.case_cyclic_build(hip)


# ---- 2. the anchors --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.ANCHOR_BOUND))
def test_anchors_twin(twin, name):
    """the bounds and makespans (and ta01's info rows) a prototype of the header's definition gave; where the mirror is quick
    enough (up to 20 x 20) it gives them too"""
    S.case_anchor(twin, name, reopts=(0, 1, 3), mirror=True)


def test_anchor_emu(emu):
    S.case_anchor(emu, "ta01", reopts=(0,))


@pytest.mark.gpu
@pytest.mark.parametrize("name", S.GPU_ANCHORS)
def test_anchors_gpu(hip, name):
    S.case_anchor(hip, name, reopts=(0, 1, 3))


# ---- 3. properties -----------------------------------------------------------------------------------------------------------------
def test_properties_seeded_twin():
    """150 seeded tiny instances: jps is the subset maximum, Schrage lies within p_max of it, the bound never exceeds the best
    completion, all fixed is evaluate_order, rank_out fed back stays acyclic, a build re-times to its makespan and is never
    cyclic"""
    from jssenv_amd.env import CpuBackend
    solved, bounded = S.case_seeded_properties(CpuBackend(threads=1), 150)
    print("seeded properties: one-machine problems solved by brute force", solved, "selections bounded by their best completion", bounded)
    assert solved > 300 and bounded > 100


@pytest.mark.parametrize("name", ("hand", "3x2", "repeats", "ta01", "J65", "one-machine", "m64"))
def test_properties_twin(twin, name):
    S.case_properties(twin, name)


@pytest.mark.parametrize("name", ("hand", "repeats"))
def test_properties_emu(emu, name):
    S.case_properties(emu, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("hand", "repeats", "ta01", "J65", "one-machine", "m64"))
def test_properties_gpu(hip, name):
    S.case_properties(hip, name)


def test_brute_force_checks_can_fail(twin):
    """the subset maximum tells a value that is one too low, and the best completion a bound that is one too high"""
    from jssenv_amd import BatchedJssEnv
    r, p, q = [0, 2, 4], [3, 2, 1], [5, 1, 0]
    assert S.subset_bound(r, p, q) == 8 and S.subset_bound(r, p, [6, 1, 0]) == 9 and S.subset_bound([9], [1], [1]) == 11
    from decode_cases import hand_instance
    inst = hand_instance()
    mach = np.asarray(S.D.HAND_MACHINE)
    best = S.best_completion(twin, inst, np.zeros((3, 3), np.int32), 0, mach)
    env = BatchedJssEnv(inst, batch=1, _backend=twin)
    env.reset()
    assert int(twin.numpy(env.relax_machines()[0])[0]) == 11 == best              # (the hand case's bound is its optimum)
    assert S.best_completion(twin, inst, np.asarray(S.HAND_BUILD["rank"], np.int32), 7, mach) == 11
    # machine 1 fixed the wrong way round, (1,2) before (2,1) before (0,0): no completion is that short any more, and the
    # bound of that selection, which the check must let pass, would not pass as a bound of the free instance
    wrong = np.zeros((3, 3), np.int32)
    wrong[2, 1], wrong[0, 0] = 1, 2
    worse = S.best_completion(twin, inst, wrong, 2, mach)
    lower = int(twin.numpy(env.relax_machines(wrong, 2)[0])[0])
    assert best < lower <= worse


# ---- 4. refusals and errors ----------------------------------------------------------------------------------------------------------
def test_refused_rows_twin(twin):
    S.case_refused_rows(twin)


def test_refused_rows_emu(emu):
    S.case_refused_rows(emu)


@pytest.mark.gpu
def test_refused_rows_gpu(hip):
    S.case_refused_rows(hip)


def test_abi_errors_twin(twin):
    S.case_abi_errors(twin)


def test_abi_errors_emu(emu):
    S.case_abi_errors(emu)


@pytest.mark.gpu
def test_abi_errors_gpu(hip):
    S.case_abi_errors(hip)


# ---- 5. the drivers ----------------------------------------------------------------------------------------------------------------
def test_driver_twin(twin):
    """bottleneck_search is its definition loop; one instance and a list; reproducible by seed, another seed other builds"""
    from jssenv_amd import search
    res = S.case_driver(twin, "ta01")
    assert res.lower_bound.tolist() == [1168] and res.makespan[0] <= 1475 and res.best_makespan[0] == 1475 and not res.optimal[0]
    both = S.case_driver(twin, ["ta01", "ta11"], walkers=6, reopt=0, spread=100, seed=4)
    assert both.rank.shape == (2, 20, 15) and both.lower_bound.tolist() == [1168, 1254] and both.best_makespan[[0, 6]].tolist() == [1633, 1928]
    again = search.bottleneck_search(["ta01", "ta11"], 6, 0, 100, seed=4, _backend=twin)
    assert np.array_equal(again.best_makespan, both.best_makespan) and np.array_equal(again.rank, both.rank)
    other = search.bottleneck_search(["ta01", "ta11"], 6, 0, 100, seed=5, _backend=twin)
    assert not np.array_equal(other.best_makespan, both.best_makespan)
    assert S.case_driver(twin, "ta01", walkers=4, target=5000).optimal.tolist() == [True]
    assert S.case_driver(twin, "ta01", walkers=4, target=None).target is None
    assert S.case_driver(twin, "ta01", walkers=4, target="lower_bound").target.tolist() == [1005]
    assert twin.numpy(res.env.evaluate_order(res.rank))[0] == res.makespan[0]


def test_driver_polish_twin(twin):
    plain = S.case_driver(twin, ["ta01", "ta11"], walkers=4)
    polished = S.case_driver(twin, ["ta01", "ta11"], walkers=4, polish=30)
    assert (polished.best_makespan <= plain.best_makespan).all() and (polished.makespan <= plain.makespan).all()
    assert np.array_equal(polished.info, plain.info)


def test_driver_emu(emu):
    S.case_driver(emu, S.D.hand_instance(), walkers=3, reopt=1, spread=3)


@pytest.mark.gpu
def test_driver_gpu(hip):
    S.case_driver(hip, ["ta01", "ta11"], walkers=16, polish=20)


def test_driver_refusals(twin):
    from jssenv_amd import BatchedJssEnv, search
    for bad in (dict(walkers=0), dict(reopt=-1), dict(reopt=9), dict(spread=-1), dict(polish=-1), dict(tenure=65), dict(target="upper")):
        with pytest.raises(ValueError):
            search.bottleneck_search("ta01", _backend=twin, **dict(dict(walkers=2), **bad))
    with pytest.raises(ValueError):
        search.bottleneck_search([], _backend=twin)
    with pytest.raises(NotImplementedError):
        search.bottleneck_search(BatchedJssEnv("ta01", batch=2, _backend=twin))


def test_one_machine_target_of_the_other_drivers(twin):
    """tabu_search, relink_search and brkga_search take target="one_machine", relax_machines() of the empty selection; "upper"
    is still refused and the default is still "lower_bound" """
    import inspect
    from jssenv_amd import search
    res = search.tabu_search("ta01", walkers=2, iters=5, target="one_machine", _backend=twin)
    assert res.target.tolist() == [1168, 1168]
    res = search.relink_search("ta01", walkers=2, iters=5, rounds=1, target="one_machine", _backend=twin)
    assert res.target.tolist() == [1168, 1168]
    res = search.brkga_search("ta01", population=4, generations=1, target="one_machine", _backend=twin)
    assert not res.optimal[0]
    for driver, kw in ((search.tabu_search, dict(walkers=2, iters=1)), (search.relink_search, dict(walkers=2, iters=1, rounds=1)),
                       (search.brkga_search, dict(population=4, generations=1))):
        assert inspect.signature(driver).parameters["target"].default == "lower_bound"
        with pytest.raises(ValueError):
            driver("ta01", target="upper", _backend=twin, **kw)


# ---- 6. the env classes ------------------------------------------------------------------------------------------------------------------
def test_facade_and_refusals(twin):
    from jssenv_amd import BatchedJssEnv
    from jssenv_amd.bucketed import BucketedJssEnv
    from jssenv_amd.facade import JssEnv
    from jssenv_amd.vector import JssVectorEnv
    n = lambda x: np.asarray(twin.numpy(x))   # noqa: E731
    env = JssEnv({"instance_path": "ta01"}, _backend=twin)
    env.reset()
    lower, length, neck = env.relax_machines()
    assert (lower, length, neck) == (1168, 963, 1) and all(isinstance(x, int) for x in (lower, length, neck))
    out = env.relax_machines(jps=True, rank_out=True)
    assert out[3].shape == (15,) and out[3].max() == 1168 and out[4].shape == (15, 15)
    assert env.relax_machines(out[4], 1 << 1)[1] >= length
    mk, rank, info = env.bottleneck()
    assert mk == 1475 and rank.shape == (15, 15) and info.tolist() == [15, 105, 28, 1168] and env.evaluate_order(rank) == 1475
    mk, rank, info, order = env.bottleneck(reopt=0, order=True)
    assert mk == 1633 and sorted(order.tolist()) == list(range(15)) and order[0] == 1
    part = env.relax_machines(rank_out=True)[3]
    assert env.bottleneck(reopt=0, rank=part, fixed=1 << 1)[0] == 1633            # the first machine fixed by hand: the same build
    b = BatchedJssEnv("ta01", batch=2, _backend=twin)
    with pytest.raises(RuntimeError):
        b.relax_machines()
    with pytest.raises(RuntimeError):
        b.bottleneck()
    b.reset()
    assert n(b.relax_machines()[0]).tolist() == [1168, 1168]
    full = n(b.bottleneck(reopt=0)[1])
    # fixed as an int, as (n,) integers, as a boolean (n, M) array
    masks = np.array([0, 2 ** 15 - 1, 5], np.uint64)
    as_bool = (masks[:, None] >> np.arange(15, dtype=np.uint64) & np.uint64(1)).astype(bool)
    a = n(b.relax_machines(full[0], masks, [0, 1, 0])[1])
    assert np.array_equal(a, n(b.relax_machines(full[0], as_bool, [0, 1, 0])[1])) and a[1] == 1633 and a[0] == 963
    assert n(b.relax_machines(full, 2 ** 15 - 1)[1]).tolist() == [1633, 1633]
    assert n(b.relax_machines(full[0], 0, [1, 1, 0, 5])[1]).tolist() == [963, 963, 963, -1]
    assert n(b.relax_machines(full, 1 << 15)[1]).tolist() == [-1, -1]
    for bad in (dict(rank=np.zeros((15, 14), np.int32)), dict(rank=np.zeros((3, 15, 15), np.int32)), dict(fixed=1), dict(rank=full, fixed=-1),
                dict(rank=full, fixed=np.zeros(3, np.int64)), dict(rank=full, fixed=np.zeros((2, 65), bool)), dict(rank=full, fixed=np.zeros(2)),
                dict(parents=[[0, 1]]), dict(parents=[0, 1, 0], rank=full)):
        with pytest.raises(ValueError):
            b.relax_machines(**bad)
    for bad in (dict(reopt=9), dict(reopt=-1), dict(rank=full), dict(fixed=3), dict(bias=np.zeros((2, 14), np.int32)), dict(parents=[0, 1, 0], bias=np.zeros((2, 15), np.int32)),
                dict(rank=full[0], fixed=0)):
        with pytest.raises(ValueError):
            b.bottleneck(**bad)
    for cls in (BucketedJssEnv, JssVectorEnv):
        for call in (cls.relax_machines, cls.bottleneck):
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
        with pytest.raises(NotImplementedError):
            env.relax_machines()
        with pytest.raises(NotImplementedError):
            env.bottleneck()
    finally:
        env._session = None


# ---- 7. ABI mirror, exports and resources -----------------------------------------------------------------------------------------------
def test_abi_mirror():
    import ctypes as C
    import re
    from jssenv_amd import _abi
    assert (_abi.ABI_VERSION, _abi.ORDER_VERSION, _abi.DECODE_VERSION, _abi.MACHINE_VERSION) == (14, 1, 1, 1)
    assert _abi.MACHINE_SYMBOLS == ("jss_machine_relax", "jss_bottleneck_build") and _abi.BOTTLENECK_NI == 4 and _abi.BOTTLENECK_MAX_REOPT == 8
    others = (_abi.SYMBOLS + _abi.SEARCH_SYMBOLS + _abi.BEAM_SYMBOLS + _abi.BOUND_SYMBOLS + _abi.ORDER_SYMBOLS + _abi.TABU_SYMBOLS
              + _abi.BLOCK_SYMBOLS + _abi.RELINK_SYMBOLS + _abi.DECODE_SYMBOLS)
    assert not set(_abi.MACHINE_SYMBOLS) & set(others)
    header = open(os.path.join(K.ROOT, "include", "jss_machine.h")).read()
    assert "#define JSS_MACHINE_VERSION 1" in header and f"#define JSS_BOTTLENECK_NI {_abi.BOTTLENECK_NI}" in header
    assert f"#define JSS_BOTTLENECK_MAX_REOPT {_abi.BOTTLENECK_MAX_REOPT}" in header
    for struct, cls, ints, count in (("JssMachineRelax", _abi.JssMachineRelax, ("n", "stride"), 13), ("JssBottleneck", _abi.JssBottleneck, ("n", "reopt"), 10)):
        body = header[header.index(f"typedef struct {struct} {{"):header.index(f"}} {struct};")]
        names = [f for f, _ in cls._fields_]
        where = [min(body.index(t) for t in (f" {f};", f"*{f};") if t in body) for f in names]
        assert where == sorted(where) and len(set(where)) == len(where)
        assert re.sub(r"/\*.*?\*/", "", body, flags=re.S).count(";") == len(names) == count        # one member per field, and no others
        assert all((t is C.c_int32) == (f in ints) for f, t in cls._fields_)
        assert C.sizeof(cls) == 8 + 8 * (count - 2)
    for name, version in (("jss_decode.h", "JSS_DECODE_VERSION 1"), ("jss_relink.h", "JSS_RELINK_VERSION 1"), ("jss_order.h", "JSS_ORDER_VERSION 1"),
                          ("jss_hip.h", "JSS_ABI_VERSION 14")):
        assert f"#define {version}" in open(os.path.join(K.ROOT, "include", name)).read()


def test_exports():
    """the two symbols come from libjss_machine_hip.so and the twin, and from none of the other eight HIP libraries, none of whose
    symbols is in the new one"""
    from jssenv_amd import _abi, build
    build.build_extension()                            # (all nine HIP libraries; nothing to do after build())
    twin_symbols, own = K.exported(build.build_cpu_twin()), K.exported(build.MACHINE_OUT)
    for name in _abi.MACHINE_SYMBOLS:
        assert name in own and name in twin_symbols
        for other in (build.OUT, build.BEAM_OUT, build.BOUND_OUT, build.ORDER_OUT, build.TABU_OUT, build.BLOCK_OUT, build.RELINK_OUT, build.DECODE_OUT):
            assert name not in K.exported(other)
    for other in (_abi.SYMBOLS + _abi.SEARCH_SYMBOLS + _abi.BEAM_SYMBOLS + _abi.BOUND_SYMBOLS + _abi.ORDER_SYMBOLS + _abi.TABU_SYMBOLS
                  + _abi.BLOCK_SYMBOLS + _abi.RELINK_SYMBOLS + _abi.DECODE_SYMBOLS):
        assert other not in own, other


def test_machine_kernel_resources():
    """libjss_machine_hip.so holds exactly its two kernels: no scratch, no spills, LDS only as the dynamic allocation the host
    sizes, at most 64 KB per wavefront (machine_lds_bytes: what a larger shape gets is JSS_E_LDS, see case_abi_errors)"""
    rows = S.machine_kernel_rows()
    assert [r[0].split("(")[0] for r in rows] == ["jss_bottleneck_kernel", "jss_machine_relax_kernel"]
    for _, _, _, vspill, sspill, scratch, lds in rows:
        assert scratch == 0 and vspill == 0 and sspill == 0 and lds == 0
    for jmax, mmax, fits in ((15, 15, True), (100, 20, True), (128, 21, True), (128, 22, False), (42, 64, True), (43, 64, False)):
        entries8 = (jmax * mmax + 7) // 8 * 8
        assert (24 * entries8 + 1024 <= 64 * 1024) == fits
    header = open(os.path.join(K.ROOT, "include", "jss_machine.h")).read()
    assert "24 bytes per entry" in header and "plus 1024" in header


def test_machine_library_is_ignored_by_git():
    out = subprocess.run(["git", "check-ignore", "jssenv_amd/libjss_machine_hip.so", "tests/emu/libjss_machine_emu.so"], cwd=K.ROOT,
                         capture_output=True, text=True)
    if out.returncode == 128:                          # (not a git checkout: nothing to ask)
        return
    assert out.stdout.split() == ["jssenv_amd/libjss_machine_hip.so", "tests/emu/libjss_machine_emu.so"]


# ---- 8. the twin's entry points under the sanitizers, in a program of their own ------------------------------------------------------
def test_twin_stand_alone_under_asan_and_ubsan(tmp_path):
    """tests/machine_twin_main.cpp and the twin's source in one program with AddressSanitizer and UndefinedBehaviorSanitizer: the
    "hand" and "repeats" cases relaxed and built; its printed lines are the mirrors' results"""
    from jssenv_amd import search
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "machine_twin_san")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(K.ROOT, "include"),
                           os.path.join(K.ROOT, "jssenv_amd", "csrc", "jss_cpu.cpp"), os.path.join(K.ROOT, "tests", "machine_twin_main.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", OMP_NUM_THREADS="2")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "MACHINE-TWIN-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    lines = out.stdout.splitlines()
    want = []
    flat = lambda x: " ".join(str(v) for v in np.asarray(x).reshape(-1))   # noqa: E731
    for name in ("hand", "repeats"):
        host = S.case_state(name)["host"]
        jmax, mmax = S.case_state(name)["env"].jmax, S.case_state(name)["env"].mmax
        ops = host["ops"].reshape(-1, jmax, mmax)
        base = S.base_rank(jmax, mmax)
        for mask in (0, 1, 2 ** mmax - 1):
            r = search.machine_reference(host["env_const"], ops, base, mask, [0])
            want.append(f"{name} relax {mask} length {r[0][0]} bound {r[1][0]} neck {r[2][0]} jps {flat(r[3])} schrage {flat(r[4])} head {flat(r[5])} "
                        f"tail {flat(r[6])} rank {flat(r[7])}")
        for reopt in (0, 2):
            b = search.bottleneck_reference(host["env_const"], ops, [0], None, reopt)
            want.append(f"{name} build {reopt} makespan {b[0][0]} info {flat(b[2])} order {flat(b[3])} rank {flat(b[1])}")
        mk = search.bottleneck_reference(host["env_const"], ops, [0, 7, 0, -1], None, 1)[0]
        want.append(f"{name} candidates {flat(mk)}")
    assert lines[:len(want)] == want, (lines, want)
