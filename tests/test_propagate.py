"""jss_propagate (include/jss_propagate.h), BatchedJssEnv.propagate, search.destructive_bound and target="destructive": constraint
propagation on the operation windows of partial selections under a trial makespan, one candidate per wavefront in one launch,
and the destructive lower bounds built on it.  On the host against the CPU twin and the kernel source under the SIMT emulator; on
the MI355X against libjss_propagate_hip.so."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import order_cases as K  # noqa: E402
import machine_cases as S  # noqa: E402
import propagate_cases as P  # noqa: E402

NAMES = list(S.CASES)


@pytest.fixture(scope="module")
def twin():
    return P.twin_backend()


@pytest.fixture(scope="module")
def emu():
    return P.emu_backend()


@pytest.fixture(scope="module")
def hip():
    from jssenv_amd.env import HipBackend
    be = HipBackend("cuda:0")
    assert be.lib.jss_backend() == b"hip:gfx950"
    return be


# ---- 1. the backends against the mirror ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_against_mirror_twin(twin, name):
    """(where the mirror is too slow the reference is the twin's own: test_twin_against_mirror_reduced holds it to the mirror)"""
    P.case_against_mirror(twin, name)


@pytest.mark.parametrize("name", [name for name in NAMES if name not in P.MIRRORED])
def test_twin_against_mirror_reduced(name):
    P.case_twin_against_mirror_reduced(name)


@pytest.mark.parametrize("name", NAMES)
def test_against_mirror_emu(emu, name):
    P.case_against_mirror(emu, name, light=0 if name in S.SMALL else 2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_against_mirror_gpu(hip, name):
    P.case_against_mirror(hip, name)


def test_what_the_cases_cover():
    """every status occurs among the candidates; hypotheses refute candidates that are open without them; the per-candidate tables
    differ from the shared one in their results"""
    seen = set()
    for name in P.MIRRORED:
        plain, hyp, own = (P.ref_of(name, v) for v in ((False, "none", 256), (True, "none", 256), (False, "own", 256)))
        seen |= set(plain[0].tolist()) | set(P.ref_of(name, (False, "none", 2))[0].tolist())
        if ((plain[0] == 0) & (hyp[0] == 1)).any():
            seen.add("hypothesis")
        if not np.array_equal(P.ref_of(name, (False, "shared", 256))[2], own[2]):
            seen.add("tables")
    assert seen >= {0, 1, 2, -1, "hypothesis", "tables"}, seen
    assert any((P.ref_of(name, (False, "none", 256))[0] == -2).any() for name in NAMES), "a cyclic selection"


# ---- 2. the cases tell the rules apart ---------------------------------------------------------------------------------------------
def test_the_rules_differ():
    """on the mirror, single rules switched off: somewhere a candidate is refuted only by the overload test, somewhere a window
    moves only by the "after" rule, by the "before" rule, by the pairwise rule, and somewhere two passes end with status 2 where
    256 end with 0 or 1"""
    found = P.rule_differences()
    assert found >= {"overload", "after", "before", "pairs", "budget"}, found


# ---- 3. the hand cases --------------------------------------------------------------------------------------------------------------
def test_ft06_twin(twin):
    """the pass counts are the mirror's (the statuses do not depend on how a pass is ordered, the counts on nothing but the
    definition): 11 passes refute 53, the fixpoint of 54 takes 6"""
    status, used = P.case_ft06(twin, mirror=True)
    assert used.tolist()[6:8] == [11, 6]


def test_ft06_emu(emu):
    P.case_ft06(emu)


@pytest.mark.gpu
def test_ft06_gpu(hip):
    P.case_ft06(hip)


def test_ta01_twin(twin):
    """the mirror refutes 1189 in pass 37 and ends 1190 at a fixpoint in pass 20"""
    from jssenv_amd import search
    status, used = P.case_ta01(twin)
    _, const, ops = P.tables_of("ta01")
    ref = search.propagate_reference(const, ops, np.asarray(sorted(P.TA01_STATUS)), parents=np.zeros(2, np.int64))
    assert np.array_equal(ref[0], status) and np.array_equal(ref[1], used) and used.tolist() == [37, 20]


@pytest.mark.gpu
def test_ta01_gpu(hip):
    status, used = P.case_ta01(hip)
    assert used.tolist() == [37, 20]


# ---- 4. soundness by brute force ---------------------------------------------------------------------------------------------------
def test_brute_force_twin():
    """150 seeded tiny instances (at most 4 x 3, durations 1 to 9), every order of every machine enumerated: no makespan at or
    above the optimum is refuted, by propagation or by a shaving hypothesis that holds an optimal start; an optimal schedule lies
    inside the windows at the optimum; destructive_bound never exceeds the optimum.  The shares were measured with the TWIN, not
    with the mirror, which would take a quarter of an hour for them (test 1 holds the twin to the mirror bit for bit, and the
    mirror's own loop gives the same counts on these 150: 31 and 3).  On 3 000 such instances the scan's bound
    exceeded the one-machine bound on 522 (17.4 %) and shaving raised it further on 26 (0.87 %): instances this small leave
    shaving little to do.  Asked for here is half of each share, 8.7 % and 0.43 % of 150 instances: 13 and 1, so that a
    propagation that deduces nothing, or a shaving loop that never cuts, fails"""
    from jssenv_amd.env import CpuBackend
    count, scan_better, shave_better = P.case_brute_force(CpuBackend(threads=1), 150)
    print("brute force: instances", count, "scan above the one-machine bound", scan_better, "shaving above the scan", shave_better)
    assert count == 150 and scan_better >= 13 and shave_better >= 1


def test_brute_force_check_can_fail():
    """a mirror whose overload threshold is off by one refutes an optimal makespan, and the check says so"""
    from jssenv_amd.env import CpuBackend
    with pytest.raises(AssertionError):
        P.case_brute_force(CpuBackend(threads=1), 150, prop=P.broken_propagation)
    opt, start = P.brute_optimum(np.asarray(P.FT06_MACHINE)[:3, :3] % 3, np.asarray(P.FT06_DURATION)[:3, :3])
    assert opt >= int(np.asarray(P.FT06_DURATION)[:3, :3].sum(axis=1).max()) and start.shape == (3, 3)


# ---- 5. properties ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("hand", "zeros", "3x2", "repeats", "J1", "M1", "ta01", "J65", "m64"))
def test_properties_twin(twin, name):
    P.case_properties(twin, name)


@pytest.mark.parametrize("name", ("hand", "repeats"))
def test_properties_emu(emu, name):
    P.case_properties(emu, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("hand", "zeros", "repeats", "ta01", "J65", "m64"))
def test_properties_gpu(hip, name):
    P.case_properties(hip, name)


# ---- 6. refusals and errors, the ABI mirror, exports and resources ---------------------------------------------------------------------
def test_refused_rows_twin(twin):
    P.case_refused_rows(twin)


def test_refused_rows_emu(emu):
    P.case_refused_rows(emu)


@pytest.mark.gpu
def test_refused_rows_gpu(hip):
    P.case_refused_rows(hip)


def test_abi_errors_twin(twin):
    P.case_abi_errors(twin)


def test_abi_errors_emu(emu):
    P.case_abi_errors(emu)


@pytest.mark.gpu
def test_abi_errors_gpu(hip):
    P.case_abi_errors(hip)


def test_abi_mirror():
    import ctypes as C
    import re
    from jssenv_amd import _abi
    assert (_abi.ABI_VERSION, _abi.MACHINE_VERSION, _abi.CARLIER_VERSION, _abi.PROPAGATE_VERSION) == (14, 1, 1, 1)
    assert _abi.PROPAGATE_SYMBOLS == ("jss_propagate",)
    assert (_abi.PROPAGATE_MAX_PASSES, _abi.PROPAGATE_MAX_TIME) == (4096, 2 ** 30 - 1)
    assert (_abi.PROPAGATE_FIXPOINT, _abi.PROPAGATE_REFUTED, _abi.PROPAGATE_BUDGET) == (0, 1, 2)
    others = (_abi.SYMBOLS + _abi.SEARCH_SYMBOLS + _abi.BEAM_SYMBOLS + _abi.BOUND_SYMBOLS + _abi.ORDER_SYMBOLS + _abi.TABU_SYMBOLS
              + _abi.BLOCK_SYMBOLS + _abi.RELINK_SYMBOLS + _abi.DECODE_SYMBOLS + _abi.MACHINE_SYMBOLS + _abi.CARLIER_SYMBOLS)
    assert not set(_abi.PROPAGATE_SYMBOLS) & set(others)
    header = open(os.path.join(K.ROOT, "include", "jss_propagate.h")).read()
    assert "#define JSS_PROPAGATE_VERSION 1" in header and f"#define JSS_PROPAGATE_MAX_PASSES {_abi.PROPAGATE_MAX_PASSES} " in header
    assert "#define JSS_PROPAGATE_MAX_TIME 0x3fffffff " in header
    for label, value in (("FIXPOINT", 0), ("REFUTED", 1), ("BUDGET", 2)):
        assert f"#define JSS_PROPAGATE_{label} {value} " in header
    body = header[header.index("typedef struct JssPropagate {"):header.index("} JssPropagate;")]
    names = [f for f, _ in _abi.JssPropagate._fields_]
    where = [min(body.index(t) for t in (f" {f};", f"*{f};") if t in body) for f in names]
    assert where == sorted(where) and len(set(where)) == len(where)
    assert re.sub(r"/\*.*?\*/", "", body, flags=re.S).count(";") == len(names) == 17           # one member per field, and no others
    assert all((t is C.c_int32) == (i < 4) for i, (_, t) in enumerate(_abi.JssPropagate._fields_))
    assert C.sizeof(_abi.JssPropagate) == 16 + 8 * 13
    for name, version in (("jss_carlier.h", "JSS_CARLIER_VERSION 1"), ("jss_machine.h", "JSS_MACHINE_VERSION 1"), ("jss_decode.h", "JSS_DECODE_VERSION 1"),
                          ("jss_relink.h", "JSS_RELINK_VERSION 1"), ("jss_order.h", "JSS_ORDER_VERSION 1"), ("jss_hip.h", "JSS_ABI_VERSION 14")):
        assert f"#define {version}" in open(os.path.join(K.ROOT, "include", name)).read()


def test_exports():
    """the symbol comes from libjss_propagate_hip.so and the twin, and from none of the other ten HIP libraries, none of whose
    symbols is in the new one"""
    from jssenv_amd import _abi, build
    build.build_extension()                            # (all eleven HIP libraries; nothing to do after build())
    twin_symbols, own = K.exported(build.build_cpu_twin()), K.exported(build.PROPAGATE_OUT)
    for name in _abi.PROPAGATE_SYMBOLS:
        assert name in own and name in twin_symbols
        for other in (build.OUT, build.BEAM_OUT, build.BOUND_OUT, build.ORDER_OUT, build.TABU_OUT, build.BLOCK_OUT, build.RELINK_OUT, build.DECODE_OUT,
                      build.MACHINE_OUT, build.CARLIER_OUT):
            assert name not in K.exported(other)
    for other in (_abi.SYMBOLS + _abi.SEARCH_SYMBOLS + _abi.BEAM_SYMBOLS + _abi.BOUND_SYMBOLS + _abi.ORDER_SYMBOLS + _abi.TABU_SYMBOLS
                  + _abi.BLOCK_SYMBOLS + _abi.RELINK_SYMBOLS + _abi.DECODE_SYMBOLS + _abi.MACHINE_SYMBOLS + _abi.CARLIER_SYMBOLS):
        assert other not in own, other


def test_propagate_kernel_resources():
    """libjss_propagate_hip.so holds exactly its one kernel: no scratch, no spills, LDS only as the dynamic allocation the host
    sizes, at most 64 KB per wavefront (propagate_lds_bytes: what a larger shape gets is JSS_E_LDS, see case_abi_errors)"""
    rows = P.propagate_kernel_rows()
    assert [r[0].split("(")[0] for r in rows] == ["jss_propagate_kernel"]
    for _, _, _, vspill, sspill, scratch, lds in rows:
        assert scratch == 0 and vspill == 0 and sspill == 0 and lds == 0
    for jmax, mmax, fits in ((15, 15, True), (100, 20, True), (128, 16, True), (128, 17, False), (33, 64, True), (34, 64, False)):
        entries8 = (jmax * mmax + 7) // 8 * 8
        assert (30 * entries8 + 1024 <= 64 * 1024) == fits
    header = open(os.path.join(K.ROOT, "include", "jss_propagate.h")).read()
    assert "30 bytes per entry" in header and "plus 1024" in header
    checks = open(os.path.join(K.ROOT, "jssenv_amd", "csrc", "jss_abi_checks.hpp")).read()
    assert "30 * order_entries8(jmax, mmax) + 4 * 64 * 4" in checks


def test_propagate_library_is_ignored_by_git():
    out = subprocess.run(["git", "check-ignore", "jssenv_amd/libjss_propagate_hip.so", "tests/emu/libjss_propagate_emu.so"], cwd=K.ROOT,
                         capture_output=True, text=True)
    if out.returncode == 128:                          # (not a git checkout: nothing to ask)
        return
    assert out.stdout.split() == ["jssenv_amd/libjss_propagate_hip.so", "tests/emu/libjss_propagate_emu.so"]
    lines = open(os.path.join(K.ROOT, ".gitignore")).read().split()                  # (*.so covers them too: the lines of their own)
    assert "jssenv_amd/libjss_propagate_hip.so" in lines and "tests/emu/libjss_propagate_emu.so" in lines


# ---- 7. the drivers and the env classes ----------------------------------------------------------------------------------------------
def test_driver_twin(twin):
    res = P.case_driver(twin)
    assert res.lower_bound.tolist()[0] == 55 and res.first_bound.tolist()[0] == 54


def test_driver_emu(emu):
    P.case_driver(emu, names=("3x2", "hand"))


@pytest.mark.gpu
def test_driver_gpu(hip):
    """ft06 and the small instances in full, ta01's scan only"""
    from jssenv_amd import search
    P.case_driver(hip)
    res = search.destructive_bound("ta01", shave=False, _backend=hip)
    assert (res.first_bound.tolist(), res.one_machine.tolist(), res.launches.tolist(), res.propagations.tolist()) == ([1190], [1168], [1], [64])


def test_destructive_target_of_the_drivers(twin):
    """tabu_search, relink_search, brkga_search and bottleneck_search take target="destructive", the scan's bound: 1190 on ta01;
    the defaults are unchanged"""
    import inspect
    from jssenv_amd import search
    res = search.tabu_search("ta01", walkers=2, iters=5, target="destructive", _backend=twin)
    assert res.target.tolist() == [1190, 1190]
    res = search.relink_search("ta01", walkers=2, iters=5, rounds=1, target="destructive", _backend=twin)
    assert res.target.tolist() == [1190, 1190]
    res = search.brkga_search("ta01", population=4, generations=1, target="destructive", _backend=twin)
    assert res.target.tolist() == [1190] and not res.optimal[0]
    res = search.bottleneck_search(["ta01", P.ft06()], 2, target="destructive", _backend=twin)
    assert res.target.tolist() == [1190, 54] and res.lower_bound.tolist() == [1168, 52]
    for driver in (search.tabu_search, search.relink_search, search.brkga_search):
        assert inspect.signature(driver).parameters["target"].default == "lower_bound"
    assert inspect.signature(search.bottleneck_search).parameters["target"].default == "one_machine"
    sig = inspect.signature(search.destructive_bound).parameters
    assert [(k, sig[k].default) for k in ("upper", "shave", "rounds", "span", "passes")] == [("upper", None), ("shave", True), ("rounds", 8), ("span", 64),
                                                                                               ("passes", 256)]
    for bad in (dict(span=0), dict(rounds=-1), dict(passes=0), dict(passes=4097), dict(upper=-1)):
        with pytest.raises(ValueError):
            search.destructive_bound("ta01", _backend=twin, **bad)
    with pytest.raises(NotImplementedError):
        search.destructive_bound(res.env)


def test_facade_and_refusals(twin):
    from jssenv_amd import BatchedJssEnv
    from jssenv_amd.bucketed import BucketedJssEnv
    from jssenv_amd.facade import JssEnv
    from jssenv_amd.vector import JssVectorEnv
    n = lambda x: np.asarray(twin.numpy(x))   # noqa: E731
    env = JssEnv({"instance_path": "ta01"}, _backend=twin)
    env.reset()
    assert env.propagate(1189) == (1, 37) and env.propagate(1190, passes=2) == (2, 2)
    status, used, est, lct = env.propagate(1190, windows=True)
    assert (status, used) == (0, 20) and all(isinstance(x, int) for x in (status, used)) and est.shape == (15, 15) and (est + 1 <= lct).all()
    assert env.propagate(1190, est=est, lct=lct) == (0, 1)
    op = int(np.argmax(lct - est))
    assert env.propagate(1190, hyp=(op, int(est.reshape(-1)[op]) + 5, int(lct.reshape(-1)[op]) - 5), windows=True)[0] in (0, 1)
    rank = env.solve_machines(rank_out=True)[3]
    assert env.propagate(1190, rank, 1 << 1)[0] in (0, 1) and env.propagate(5000, rank, 1 << 1)[0] == 0
    b = BatchedJssEnv("ta01", batch=2, _backend=twin)
    with pytest.raises(RuntimeError):
        b.propagate(1190)
    b.reset()
    assert n(b.propagate(1190)[0]).tolist() == [0, 0] and n(b.propagate([1189, 1190])[0]).tolist() == [1, 0]
    assert n(b.propagate(1190, parents=[1, 1, 0, 5])[0]).tolist() == [0, 0, 0, -1]
    assert n(b.propagate(1190, est=est, lct=lct)[1]).tolist() == [1, 1] and n(b.propagate(1190, est=np.stack([est, est]), lct=np.stack([lct, lct]))[1]).tolist() == [1, 1]
    for bad in (dict(passes=0), dict(passes=4097), dict(rank=np.zeros((15, 14), np.int32)), dict(fixed=1), dict(est=est), dict(lct=lct),
                dict(est=est, lct=lct[:14]), dict(hyp=(np.zeros(2, np.int32),)), dict(hyp=(np.zeros(3, np.int32),) * 3), dict(parents=[[0, 1]]),
                dict(parents=[0, 1, 0], est=np.stack([est, est]), lct=np.stack([lct, lct]))):
        with pytest.raises(ValueError):
            b.propagate(1190, **bad)
    with pytest.raises(ValueError):
        b.propagate([1190, 1190, 1190])
    with pytest.raises(ValueError):
        b.propagate(2 ** 40)
    for cls in (BucketedJssEnv, JssVectorEnv):
        with pytest.raises(NotImplementedError):
            cls.propagate(None)


class _OpenSession:
    closed = False


def test_open_session_is_refused(twin):
    from jssenv_amd import BatchedJssEnv
    env = BatchedJssEnv("ta01", batch=1, _backend=twin)
    env.reset()
    env._session = _OpenSession()
    try:
        with pytest.raises(NotImplementedError):
            env.propagate(1190)
    finally:
        env._session = None


# ---- 8. the twin's entry point under the sanitizers, in a program of its own -----------------------------------------------------------
def test_twin_stand_alone_under_asan_and_ubsan(tmp_path):
    """tests/propagate_twin_main.cpp and the twin's source in one program with AddressSanitizer and UndefinedBehaviorSanitizer:
    ft06, "hand" and "repeats" propagated under two masks, several makespans and budgets, with and without a hypothesis and once
    more from the returned windows; its printed lines are the mirror's results"""
    from jssenv_amd import BatchedJssEnv, search
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "propagate_twin_san")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(K.ROOT, "include"),
                           os.path.join(K.ROOT, "jssenv_amd", "csrc", "jss_cpu.cpp"), os.path.join(K.ROOT, "tests", "propagate_twin_main.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", OMP_NUM_THREADS="2")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "PROPAGATE-TWIN-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    lines = out.stdout.splitlines()
    want = []
    flat = lambda x: " ".join(str(v) for v in np.asarray(x).reshape(-1))   # noqa: E731
    ft = BatchedJssEnv(P.ft06(), batch=2, _backend=P.twin_backend())
    ft.reset(which=np.array([1, 0], np.uint8))
    host = K.host_tables(ft)
    for name, ubs in (("ft06", (50, 53, 54, 55, 70)), ("hand", (10, 11, 12, 20)), ("repeats", (20, 26, 30, 34, 60))):
        if name == "ft06":
            const, ops, jmax, mmax = host["env_const"], host["ops"].reshape(-1, 6, 6), 6, 6
        else:
            st = S.case_state(name)
            jmax, mmax = st["env"].jmax, st["env"].mmax
            const, ops = st["host"]["env_const"], st["host"]["ops"].reshape(-1, jmax, mmax)
        base = S.base_rank(jmax, mmax)
        for passes in (1, 2, 256):
            for mask in (0, 1):
                for ub in ubs:
                    for with_hyp in (0, 1):
                        hyp = ([1], [2], [ub - 1]) if with_hyp else None
                        r = search.propagate_reference(const, ops, [ub], base, mask, [0], hyp=hyp, passes=passes)
                        line = f"{name} prop {passes} {mask} {ub} {with_hyp} status {r[0][0]} used {r[1][0]}"
                        if r[0][0] != 1:
                            a = search.propagate_reference(const, ops, [ub], base, mask, [0], est=r[2][0], lct=r[3][0], passes=passes)
                            line += f" est {flat(r[2])} lct {flat(r[3])} again {a[0][0]} {a[1][0]} est {flat(a[2])} lct {flat(a[3])}"
                        want.append(line)
        status = search.propagate_reference(const, ops, [ubs[0], ubs[0], ubs[-1], ubs[0]], parents=[0, 7, 0, -1], passes=3)[0]
        want.append(f"{name} candidates {flat(status)}")
    assert lines[:len(want)] == want, [(a, b) for a, b in zip(lines, want) if a != b][:3]
