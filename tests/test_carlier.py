"""jss_machine_solve and jss_bottleneck_exact (include/jss_carlier.h), BatchedJssEnv.solve_machines / bottleneck_exact and
search.bottleneck_search(nodes=...): Carlier's branch and bound for the one-machine problems of partial selections, and shifting
bottleneck constructions sequenced by it, one candidate per wavefront in one launch.  On the host against the CPU twin and the
kernel source under the SIMT emulator; on the MI355X against libjss_carlier_hip.so."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import order_cases as K  # noqa: E402
import machine_cases as S  # noqa: E402
import carlier_cases as X  # noqa: E402

NAMES = list(S.CASES)


@pytest.fixture(scope="module")
def twin():
    return X.twin_backend()


@pytest.fixture(scope="module")
def emu():
    return X.emu_backend()


@pytest.fixture(scope="module")
def hip():
    from jssenv_amd.env import HipBackend
    be = HipBackend("cuda:0")
    assert be.lib.jss_backend() == b"hip:gfx950"
    return be


# ---- 1. the backends against the mirror ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_against_mirror_twin(twin, name):
    X.case_against_mirror(twin, name)


@pytest.mark.parametrize("name", NAMES)
def test_against_mirror_emu(emu, name):
    X.case_against_mirror(emu, name, light=1 if name in S.SMALL else 2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_against_mirror_gpu(hip, name):
    X.case_against_mirror(hip, name)


def test_the_budgets_differ():
    """the budgets of the cases are told apart: somewhere a second node finds a better schedule, somewhere a budget leaves a
    problem open that a larger one closes, and a build changes with it"""
    one, two, many = (X.solve_ref("ta01", nodes) for nodes in (1, 2, 256))
    live = one[0] >= 0
    assert (two[3][live] < one[3][live]).any() and (many[6][live] != two[6][live]).any() and (many[5][live] > 3).any()
    assert not np.array_equal(X.exact_ref("ta01", 1, 0)[0], X.exact_ref("ta01", 256, 0)[0])


# ---- 2. a budget of one node is the existing library -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_budget_one_twin(twin, name):
    X.case_budget_one(twin, name)


@pytest.mark.parametrize("name", NAMES)
def test_budget_one_emu(emu, name):
    X.case_budget_one(emu, name, light=1 if name in S.SMALL else 2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_budget_one_gpu(hip, name):
    X.case_budget_one(hip, name)


def test_cyclic_build_twin(twin):
    X.case_cyclic_build(twin)


def test_cyclic_build_emu(emu):
    X.case_cyclic_build(emu)


@pytest.mark.gpu
def test_cyclic_build_gpu(hip):
    X.case_cyclic_build(hip)


# ---- 3. the hand case ------------------------------------------------------------------------------------------------------------------
def test_hand_twin(twin):
    X.case_hand(twin, mirror=True)


def test_hand_emu(emu):
    X.case_hand(emu)


@pytest.mark.gpu
def test_hand_gpu(hip):
    X.case_hand(hip)


# ---- 4. brute force --------------------------------------------------------------------------------------------------------------------
def test_brute_force_twin():
    """150 seeded tiny instances, every selection on the way of their exact build: every proved optimum is the minimum over all
    permutations and no bound exceeds the best completion.  A prototype of the definition improved on Schrage's schedule in 764
    of 3 000 such instances (25 %); asked for here is less than half of that share, 10 % of the instances, so that a search that
    never or hardly ever finds a better schedule fails while another generator of tiny instances does not"""
    from jssenv_amd.env import CpuBackend
    checked, improved, bounded = X.case_brute_force(CpuBackend(threads=1), 150)
    print("brute force: one-machine problems", checked, "instances better than Schrage", improved, "selections bounded by their best completion", bounded)
    assert checked >= 450 and improved >= 15 and bounded >= 25


def test_brute_force_check_can_fail():
    """the permutation minimum tells a value that is off by one, either way"""
    assert X.brute_optimum(X.HAND_R, X.HAND_P, X.HAND_Q) == 52
    X.check_optimum(52, X.HAND_R, X.HAND_P, X.HAND_Q)
    for off in (51, 53):
        with pytest.raises(AssertionError):
            X.check_optimum(off, X.HAND_R, X.HAND_P, X.HAND_Q)
    assert X.brute_optimum([0, 2, 4], [3, 2, 1], [5, 1, 0]) == 8 and X.brute_optimum([9], [1], [1]) == 11


# ---- 5. properties -----------------------------------------------------------------------------------------------------------------------
def test_properties_seeded_twin():
    from jssenv_amd.env import CpuBackend
    X.case_seeded_properties(CpuBackend(threads=1), 40)


@pytest.mark.parametrize("name", ("hand", "zeros", "3x2", "repeats", "ta01", "J65", "one-machine", "m64"))
def test_properties_twin(twin, name):
    X.case_properties(twin, name)


@pytest.mark.parametrize("name", ("hand", "repeats"))
def test_properties_emu(emu, name):
    X.case_properties(emu, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("hand", "zeros", "repeats", "ta01", "J65", "one-machine", "m64"))
def test_properties_gpu(hip, name):
    X.case_properties(hip, name)


# ---- 6. the anchors --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted({name for name, _ in X.ANCHOR_EXACT}))
def test_anchors_twin(twin, name):
    """the makespans, node counts and problem counts a prototype of the header's definition gave; where the mirror is quick
    enough (up to 20 x 20, reopt 0 and 1) it gives them too"""
    X.case_anchor(twin, name, mirror=True)


def test_anchor_ta01_twin(twin):
    X.case_anchor_ta01(twin, mirror=True)


def test_anchor_emu(emu):
    X.case_anchor(emu, "ta01", reopts=(0,))


@pytest.mark.gpu
@pytest.mark.parametrize("name", X.GPU_ANCHORS)
def test_anchors_gpu(hip, name):
    X.case_anchor(hip, name)


@pytest.mark.gpu
def test_anchor_ta01_gpu(hip):
    X.case_anchor_ta01(hip)


# ---- 7. refusals and errors ----------------------------------------------------------------------------------------------------------
def test_refused_rows_twin(twin):
    X.case_refused_rows(twin)


def test_refused_rows_emu(emu):
    X.case_refused_rows(emu)


@pytest.mark.gpu
def test_refused_rows_gpu(hip):
    X.case_refused_rows(hip)


def test_abi_errors_twin(twin):
    X.case_abi_errors(twin)


def test_abi_errors_emu(emu):
    X.case_abi_errors(emu)


@pytest.mark.gpu
def test_abi_errors_gpu(hip):
    X.case_abi_errors(hip)


# ---- 8. ABI mirror, exports and resources -----------------------------------------------------------------------------------------------
def test_abi_mirror():
    import ctypes as C
    import re
    from jssenv_amd import _abi
    assert (_abi.ABI_VERSION, _abi.MACHINE_VERSION, _abi.CARLIER_VERSION) == (14, 1, 1)
    assert _abi.CARLIER_SYMBOLS == ("jss_machine_solve", "jss_bottleneck_exact")
    assert (_abi.CARLIER_MAX_NODES, _abi.CARLIER_MAX_DEPTH, _abi.EXACT_NI) == (4096, 64, 8)
    others = (_abi.SYMBOLS + _abi.SEARCH_SYMBOLS + _abi.BEAM_SYMBOLS + _abi.BOUND_SYMBOLS + _abi.ORDER_SYMBOLS + _abi.TABU_SYMBOLS
              + _abi.BLOCK_SYMBOLS + _abi.RELINK_SYMBOLS + _abi.DECODE_SYMBOLS + _abi.MACHINE_SYMBOLS)
    assert not set(_abi.CARLIER_SYMBOLS) & set(others)
    header = open(os.path.join(K.ROOT, "include", "jss_carlier.h")).read()
    assert "#define JSS_CARLIER_VERSION 1" in header and f"#define JSS_EXACT_NI {_abi.EXACT_NI} " in header
    assert f"#define JSS_CARLIER_MAX_NODES {_abi.CARLIER_MAX_NODES} " in header and f"#define JSS_CARLIER_MAX_DEPTH {_abi.CARLIER_MAX_DEPTH} " in header
    for struct, cls, count in (("JssMachineSolve", _abi.JssMachineSolve, 17), ("JssBottleneckExact", _abi.JssBottleneckExact, 12)):
        body = header[header.index(f"typedef struct {struct} {{"):header.index(f"}} {struct};")]
        names = [f for f, _ in cls._fields_]
        where = [min(body.index(t) for t in (f" {f};", f"*{f};") if t in body) for f in names]
        assert where == sorted(where) and len(set(where)) == len(where)
        assert re.sub(r"/\*.*?\*/", "", body, flags=re.S).count(";") == len(names) == count        # one member per field, and no others
        assert all((t is C.c_int32) == (i < 4) for i, (_, t) in enumerate(cls._fields_))
        assert C.sizeof(cls) == 16 + 8 * (count - 4)
    for name, version in (("jss_machine.h", "JSS_MACHINE_VERSION 1"), ("jss_decode.h", "JSS_DECODE_VERSION 1"), ("jss_order.h", "JSS_ORDER_VERSION 1"),
                          ("jss_hip.h", "JSS_ABI_VERSION 14")):
        assert f"#define {version}" in open(os.path.join(K.ROOT, "include", name)).read()


def test_exports():
    """the two symbols come from libjss_carlier_hip.so and the twin, and from none of the other nine HIP libraries, none of whose
    symbols is in the new one"""
    from jssenv_amd import _abi, build
    build.build_extension()                            # (all ten HIP libraries; nothing to do after build())
    twin_symbols, own = K.exported(build.build_cpu_twin()), K.exported(build.CARLIER_OUT)
    for name in _abi.CARLIER_SYMBOLS:
        assert name in own and name in twin_symbols
        for other in (build.OUT, build.BEAM_OUT, build.BOUND_OUT, build.ORDER_OUT, build.TABU_OUT, build.BLOCK_OUT, build.RELINK_OUT, build.DECODE_OUT,
                      build.MACHINE_OUT):
            assert name not in K.exported(other)
    for other in (_abi.SYMBOLS + _abi.SEARCH_SYMBOLS + _abi.BEAM_SYMBOLS + _abi.BOUND_SYMBOLS + _abi.ORDER_SYMBOLS + _abi.TABU_SYMBOLS
                  + _abi.BLOCK_SYMBOLS + _abi.RELINK_SYMBOLS + _abi.DECODE_SYMBOLS + _abi.MACHINE_SYMBOLS):
        assert other not in own, other


def test_carlier_kernel_resources():
    """libjss_carlier_hip.so holds exactly its two kernels: no scratch, no spills, LDS only as the dynamic allocation the host
    sizes, at most 64 KB per wavefront (carlier_lds_bytes: what a larger shape gets is JSS_E_LDS, see case_abi_errors)"""
    rows = X.carlier_kernel_rows()
    assert [r[0].split("(")[0] for r in rows] == ["jss_bottleneck_exact_kernel", "jss_machine_solve_kernel"]
    for _, _, _, vspill, sspill, scratch, lds in rows:
        assert scratch == 0 and vspill == 0 and sspill == 0 and lds == 0
    for jmax, mmax, fits in ((15, 15, True), (100, 20, True), (128, 17, True), (128, 18, False), (35, 64, True), (36, 64, False)):
        entries8 = (jmax * mmax + 7) // 8 * 8
        assert (28 * entries8 + 1024 + 768 <= 64 * 1024) == fits
    header = open(os.path.join(K.ROOT, "include", "jss_carlier.h")).read()
    assert "28 bytes per entry" in header and "plus 1024 plus 768" in header
    checks = open(os.path.join(K.ROOT, "jssenv_amd", "csrc", "jss_abi_checks.hpp")).read()
    assert "28 * order_entries8(jmax, mmax) + 4 * 64 * 4 + 3 * JSS_CARLIER_MAX_DEPTH * 4" in checks


def test_carlier_library_is_ignored_by_git():
    out = subprocess.run(["git", "check-ignore", "jssenv_amd/libjss_carlier_hip.so", "tests/emu/libjss_carlier_emu.so"], cwd=K.ROOT,
                         capture_output=True, text=True)
    if out.returncode == 128:                          # (not a git checkout: nothing to ask)
        return
    assert out.stdout.split() == ["jssenv_amd/libjss_carlier_hip.so", "tests/emu/libjss_carlier_emu.so"]


# ---- 9. the drivers and the env classes ----------------------------------------------------------------------------------------------
def test_driver_nodes_zero_is_todays_path(twin):
    """bottleneck_search(nodes=0) is machine_cases' definition loop, which does not know the new calls"""
    from jssenv_amd import search
    want = S.definition_loop(twin, ["ta01", "ta11"], 6, 1, 100, 0, 8, 4, "one_machine")
    for res in (search.bottleneck_search(["ta01", "ta11"], 6, 1, 100, seed=4, _backend=twin),
                search.bottleneck_search(["ta01", "ta11"], 6, 1, 100, seed=4, _backend=twin, nodes=0)):
        for label, w in zip(S.FIELDS, want):
            assert np.array_equal(getattr(res, label), w), label
        assert res.info.shape == (12, 4)
    with pytest.raises(ValueError):
        search.bottleneck_search("ta01", 2, target="one_machine_exact", _backend=twin)


def check_driver(be, walkers):
    from jssenv_amd import search
    n = lambda x: np.asarray(be.numpy(x))   # noqa: E731
    res = search.bottleneck_search("ta01", walkers, nodes=256, seed=3, _backend=be)
    assert res.makespan[0] <= 1345 and res.best_makespan[0] == 1345 and res.lower_bound.tolist() == [1168] and res.target.tolist() == [1168]
    assert res.info.shape == (walkers, 8) and (res.info[:, 6] == 0).all() and n(res.env.evaluate_order(res.rank))[0] == res.makespan[0]
    again = search.bottleneck_search("ta01", walkers, nodes=256, seed=3, _backend=be)
    assert np.array_equal(again.best_makespan, res.best_makespan) and np.array_equal(again.rank, res.rank) and np.array_equal(again.info, res.info)
    # the definition: the builds are bottleneck_exact's on the driver's biases
    bias = np.random.default_rng(3).integers(0, 51, (walkers, 15)).astype(np.int32)
    bias[0] = 0
    mk = n(res.env.bottleneck_exact(np.zeros(walkers, np.int32), bias, 1, 256)[0])
    assert np.array_equal(mk, res.best_makespan)
    return res


def test_driver_exact_twin(twin):
    from jssenv_amd import search
    res = check_driver(twin, 8)
    other = search.bottleneck_search("ta01", 8, nodes=256, seed=4, _backend=twin)
    assert not np.array_equal(other.best_makespan, res.best_makespan)
    polished = search.bottleneck_search("ta01", 4, nodes=256, polish=20, seed=3, target="one_machine_exact", _backend=twin)
    assert (polished.best_makespan <= res.best_makespan[:4]).all() and polished.target.tolist() == [1168]
    for bad in (dict(nodes=-1), dict(nodes=4097)):
        with pytest.raises(ValueError):
            search.bottleneck_search("ta01", 2, _backend=twin, **bad)


@pytest.mark.gpu
def test_driver_exact_gpu(hip):
    check_driver(hip, 16)


def test_exact_target_of_the_other_drivers(twin):
    """tabu_search, relink_search and brkga_search take target="one_machine_exact", solve_machines() of the empty selection; the
    defaults are unchanged"""
    import inspect
    from jssenv_amd import search
    res = search.tabu_search("ta01", walkers=2, iters=5, target="one_machine_exact", _backend=twin)
    assert res.target.tolist() == [1168, 1168]
    res = search.relink_search("ta01", walkers=2, iters=5, rounds=1, target="one_machine_exact", _backend=twin)
    assert res.target.tolist() == [1168, 1168]
    res = search.brkga_search("ta01", population=4, generations=1, target="one_machine_exact", _backend=twin)
    assert not res.optimal[0]
    for driver, kw in ((search.tabu_search, dict(walkers=2, iters=1)), (search.relink_search, dict(walkers=2, iters=1, rounds=1)),
                       (search.brkga_search, dict(population=4, generations=1))):
        assert inspect.signature(driver).parameters["target"].default == "lower_bound"
        with pytest.raises(ValueError):
            driver("ta01", target="upper", _backend=twin, **kw)
    assert inspect.signature(search.bottleneck_search).parameters["nodes"].default == 0


def test_facade_and_refusals(twin):
    from jssenv_amd import BatchedJssEnv
    from jssenv_amd.bucketed import BucketedJssEnv
    from jssenv_amd.facade import JssEnv
    from jssenv_amd.vector import JssVectorEnv
    n = lambda x: np.asarray(twin.numpy(x))   # noqa: E731
    env = JssEnv({"instance_path": "ta01"}, _backend=twin)
    env.reset()
    lower, length, neck = env.solve_machines()
    assert (lower, length, neck) == (1168, 963, 1) and all(isinstance(x, int) for x in (lower, length, neck))
    out = env.solve_machines(opt=True, nodes_used=True, proved=True, rank_out=True)
    assert out[3].tolist() == X.TA01_OPT and out[4].tolist() == X.TA01_NODES and out[5] == 2 ** 15 - 1 and out[6].shape == (15, 15)
    assert env.solve_machines(nodes=2, proved=True)[3] != 2 ** 15 - 1
    assert env.relax_machines(out[6], 1 << 0)[1] >= length
    mk, rank, info = env.bottleneck_exact()
    assert mk == 1345 and rank.shape == (15, 15) and info.tolist() == [15, 105, 33, 1168, 264, 18, 0, 0] and env.evaluate_order(rank) == 1345
    mk, rank, info, order = env.bottleneck_exact(reopt=0, nodes=4096, order=True)
    assert mk == 1512 and sorted(order.tolist()) == list(range(15)) and order[0] == 1
    part = env.solve_machines(rank_out=True)[3]
    assert env.bottleneck_exact(reopt=0, rank=part, fixed=1 << 1)[0] == 1512      # the first machine fixed by hand: the same build
    b = BatchedJssEnv("ta01", batch=2, _backend=twin)
    with pytest.raises(RuntimeError):
        b.solve_machines()
    with pytest.raises(RuntimeError):
        b.bottleneck_exact()
    b.reset()
    assert n(b.solve_machines()[0]).tolist() == [1168, 1168]
    full = n(b.bottleneck_exact(reopt=0)[1])
    assert n(b.solve_machines(full, 2 ** 15 - 1)[1]).tolist() == [1512, 1512]
    assert n(b.solve_machines(full[0], 0, [1, 1, 0, 5])[1]).tolist() == [963, 963, 963, -1]
    for bad in (dict(nodes=0), dict(nodes=4097), dict(rank=np.zeros((15, 14), np.int32)), dict(fixed=1), dict(rank=full, fixed=-1),
                dict(parents=[[0, 1]]), dict(parents=[0, 1, 0], rank=full)):
        with pytest.raises(ValueError):
            b.solve_machines(**bad)
    for bad in (dict(nodes=0), dict(nodes=4097), dict(reopt=9), dict(rank=full), dict(fixed=3), dict(bias=np.zeros((2, 14), np.int32))):
        with pytest.raises(ValueError):
            b.bottleneck_exact(**bad)
    for cls in (BucketedJssEnv, JssVectorEnv):
        for call in (cls.solve_machines, cls.bottleneck_exact):
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
            env.solve_machines()
        with pytest.raises(NotImplementedError):
            env.bottleneck_exact()
    finally:
        env._session = None


# ---- 10. the twin's entry points under the sanitizers, in a program of their own -----------------------------------------------------
def test_twin_stand_alone_under_asan_and_ubsan(tmp_path):
    """tests/carlier_twin_main.cpp and the twin's source in one program with AddressSanitizer and UndefinedBehaviorSanitizer: the
    textbook case, "hand" and "repeats" solved and built at several budgets; its printed lines are the mirrors' results"""
    from jssenv_amd import search
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "carlier_twin_san")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(K.ROOT, "include"),
                           os.path.join(K.ROOT, "jssenv_amd", "csrc", "jss_cpu.cpp"), os.path.join(K.ROOT, "tests", "carlier_twin_main.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", OMP_NUM_THREADS="2")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "CARLIER-TWIN-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    lines = out.stdout.splitlines()
    want = []
    flat = lambda x: " ".join(str(v) for v in np.asarray(x).reshape(-1))   # noqa: E731
    textbook = BatchedJssEnvTables(X.hand_instance())
    for name in ("textbook", "hand", "repeats"):
        if name == "textbook":
            const, ops, jmax, mmax = textbook
        else:
            host = S.case_state(name)["host"]
            jmax, mmax = S.case_state(name)["env"].jmax, S.case_state(name)["env"].mmax
            const, ops = host["env_const"], host["ops"].reshape(-1, jmax, mmax)
        base = S.base_rank(jmax, mmax)
        for nodes in (1, 2, 100):
            for mask in (0, 1):
                r = search.solve_reference(const, ops, base, mask, [0], nodes)
                want.append(f"{name} solve {nodes} {mask} length {r[0][0]} bound {r[1][0]} neck {r[2][0]} opt {flat(r[3])} low {flat(r[4])} "
                            f"nodes {flat(r[5])} proved {int(r[6][0])} head {flat(r[7])} tail {flat(r[8])} rank {flat(r[9])}")
            for reopt in (0, 2):
                b = search.bottleneck_exact_reference(const, ops, [0], None, reopt, nodes)
                want.append(f"{name} build {nodes} {reopt} makespan {b[0][0]} info {flat(b[2])} order {flat(b[3])} rank {flat(b[1])}")
        mk = search.bottleneck_exact_reference(const, ops, [0, 7, 0, -1], None, 1, 3)[0]
        want.append(f"{name} candidates {flat(mk)}")
    assert lines[:len(want)] == want, (lines, want)


def BatchedJssEnvTables(inst):
    """(env_const, ops, jmax, mmax) of a batch of two envs of `inst` on the twin, the second never reset (as the program's)"""
    from jssenv_amd import BatchedJssEnv
    env = BatchedJssEnv(inst, batch=2, _backend=X.twin_backend())
    env.reset(which=np.array([1, 0], np.uint8))
    host = K.host_tables(env)
    return host["env_const"], host["ops"].reshape(-1, env.jmax, env.mmax), env.jmax, env.mmax
