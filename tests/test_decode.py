"""jss_decode_keys and jss_keys_evolve (include/jss_decode.h), BatchedJssEnv.decode_keys / evolve_keys and search.brkga_search:
key tables decoded into active schedules by Giffler and Thompson's procedure, one decode per candidate in one launch, one BRKGA
generation, and the driver over both.  On the host against the CPU twin and the kernel source under the SIMT emulator; on the
MI355X against libjss_decode_hip.so."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import order_cases as K  # noqa: E402
import decode_cases as D  # noqa: E402

NAMES = list(D.CASES)


@pytest.fixture(scope="module")
def twin():
    return D.twin_backend()


@pytest.fixture(scope="module")
def emu():
    return D.emu_backend()


@pytest.fixture(scope="module")
def hip():
    from jssenv_amd.env import HipBackend
    be = HipBackend("cuda:0")
    assert be.lib.jss_backend() == b"hip:gfx950"
    return be


# ---- 1. the backends against the mirror ----------------------------------------------------------------------------------------
def test_cases():
    assert set(NAMES) == set(D.REUSED) | {"hand", "zeros", "ties", "J1", "M1", "J64", "J128", "extreme", "many"}
    shapes = {name: (D.case_state(name)["env"].jmax, D.case_state(name)["env"].mmax) for name in D.OWN}
    assert shapes == {"hand": (3, 3), "zeros": (4, 3), "ties": (5, 4), "J1": (1, 4), "M1": (5, 2), "J64": (64, 3), "J128": (128, 2),
                      "extreme": (6, 4), "many": (6, 4)}
    const = D.case_state("M1")["host"]["env_const"]
    assert const[:2, 1].tolist() == [1, 1] and D.case_state("many")["par"].size == 70
    keys = D.case_state("extreme")["tables"]
    assert {D.I32_MIN, D.I32_MAX, -1} <= set(np.unique(keys).tolist()) and len(np.unique(D.case_state("ties")["tables"])) == 1
    assert (D.case_state("zeros")["host"]["ops"] & 0xFFFF == 0).sum() >= 6


@pytest.mark.parametrize("name", NAMES)
def test_against_mirror_twin(twin, name):
    D.case_against_mirror(twin, name)


@pytest.mark.parametrize("name", NAMES)
def test_against_mirror_emu(emu, name):
    D.case_against_mirror(emu, name, light=name not in ("hand", "zeros", "ties", "J1", "M1", "3x2", "1x2", "extreme"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_against_mirror_gpu(hip, name):
    D.case_against_mirror(hip, name)


def test_hand_twin(twin):
    D.case_hand(twin, mirror=True)


def test_hand_emu(emu):
    D.case_hand(emu)


@pytest.mark.gpu
def test_hand_gpu(hip):
    D.case_hand(hip)


# ---- 2. the anchors --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(D.ANCHORS), ids=lambda k: "-".join(k))
def test_anchors_twin(twin, key):
    """the makespans (and ta01 SPT's info rows) a prototype of the header's definition gave; the mirror gives them too"""
    D.case_anchor(twin, key, mirror=True)


def test_anchor_emu(emu):
    D.case_anchor(emu, ("ta01", "SPT"))


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(D.ANCHORS), ids=lambda k: "-".join(k))
def test_anchors_gpu(hip, key):
    D.case_anchor(hip, key)


def test_delta_0_of_spt_is_the_spt_rollout(twin):
    """what the issue observed: the non-delay decode of the SPT table is the env's own SPT episode on ta01"""
    env = K.rolled_out(twin, "ta01", "SPT")
    assert int(np.asarray(twin.numpy(env.makespan))[0]) == D.ANCHORS[("ta01", "SPT")][2]


# ---- 3. properties -----------------------------------------------------------------------------------------------------------------
def test_properties_seeded_twin():
    """300 seeded tiny instances, three key tables each: the round trip, a valid rank, no delay at delta 0, active at delta 1"""
    from jssenv_amd.env import CpuBackend
    total = D.case_seeded_properties(CpuBackend(threads=1), 300)
    print("seeded properties: delta = 1 info sums (conflicts, widest, delayed, 0)", total.tolist())
    assert total[0] > 0 and total[2] > 0                               # conflicts were decided, and operations were delayed


@pytest.mark.parametrize("name", D.POSITIVE)
def test_properties_twin(twin, name):
    D.case_properties(twin, name)


@pytest.mark.parametrize("name", ("hand", "ties", "J65", "3x2"))
def test_properties_emu(emu, name):
    D.case_properties(emu, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", D.POSITIVE)
def test_properties_gpu(hip, name):
    D.case_properties(hip, name)


def test_brute_force_checks_can_fail():
    """the two brute-force checks refuse a schedule that waits: a 2 x 2 instance whose second job starts late"""
    mach, dur = np.array([[0, 1], [1, 0]]), np.array([[2, 2], [2, 2]])
    good, late = np.array([[0, 2], [0, 2]]), np.array([[0, 2], [0, 3]])
    assert D.no_delay(good, mach, dur) and D.active(good, mach, dur) and D.feasible(late, mach, dur) == 5
    assert not D.no_delay(late, mach, dur) and not D.active(late, mach, dur)


# ---- 4. refusals and errors ----------------------------------------------------------------------------------------------------------
def test_refused_rows_twin(twin):
    D.case_refused_rows(twin)


def test_refused_rows_emu(emu):
    D.case_refused_rows(emu)


@pytest.mark.gpu
def test_refused_rows_gpu(hip):
    D.case_refused_rows(hip)


def test_abi_errors_twin(twin):
    D.case_abi_errors(twin)


def test_abi_errors_emu(emu):
    D.case_abi_errors(emu)


@pytest.mark.gpu
def test_abi_errors_gpu(hip):
    D.case_abi_errors(hip)


# ---- 5. evolve -------------------------------------------------------------------------------------------------------------------------
EVOLVE_IDS = ["3x8x12", "1x2x1", "rho0", "rho1", "P4096"]


@pytest.mark.parametrize("shape", D.EVOLVE_SHAPES, ids=EVOLVE_IDS)
def test_evolve_twin(twin, shape):
    out, _ = D.case_evolve(twin, shape)
    G, P, region, ne, nm, rho = shape
    if rho in (0.0, 1.0) and P > ne + nm:                              # every child is one parent's copy: an elite's at rho 1, never at rho 0
        x = D.evolve_inputs(shape)
        order = x["ref"][1][:P]
        elites = {tuple(x["keys"][p]) for p in order[:ne]}
        children = [tuple(out[c]) for c in range(ne, P - nm)]
        assert all((c in elites) == (rho == 1.0) for c in children)


@pytest.mark.parametrize("shape", D.EVOLVE_SHAPES, ids=EVOLVE_IDS)
def test_evolve_emu(emu, shape):
    D.case_evolve(emu, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", D.EVOLVE_SHAPES, ids=EVOLVE_IDS)
def test_evolve_gpu(hip, shape):
    D.case_evolve(hip, shape)


def test_evolve_fresh_twin(twin):
    D.case_evolve_fresh(twin)


def test_evolve_fresh_emu(emu):
    D.case_evolve_fresh(emu)


@pytest.mark.gpu
def test_evolve_fresh_gpu(hip):
    D.case_evolve_fresh(hip)


def test_evolve_errors_twin(twin):
    D.case_evolve_errors(twin)


def test_evolve_errors_emu(emu):
    D.case_evolve_errors(emu)


@pytest.mark.gpu
def test_evolve_errors_gpu(hip):
    D.case_evolve_errors(hip)


def test_rng_mirror_is_the_oracles():
    from jssenv_amd import search
    from oracle.oracle import rng_u32
    for seed, env_id, ep, st in ((0, 0, 0, 0), (2 ** 64 - 1, 2 ** 40 + 3, 7, 225), (0xD1B54A32D192ED03, 8191, 100, 2 ** 31)):
        assert int(search.rng_u32(seed, [env_id], ep, [st])[0]) == rng_u32(seed, env_id, ep, st)


# ---- 6. the driver -----------------------------------------------------------------------------------------------------------------
def test_driver_twin(twin):
    """brkga_search is its definition loop; history never rises; one instance and a list"""
    D.case_driver(twin, "ta01")
    res = D.case_driver(twin, ["ta01", "ta11"])
    assert res.generations == 6 and res.keys.shape == (2, 20, 15) and res.start.shape == (2, 20, 15)
    D.case_driver(twin, "ta01", population=9, generations=5, elite=0.2, mutants=0.3, rho=0.6, delta=1.0, seed_rules=(), seed=5, target=None)
    res = D.case_driver(twin, ["ta01", "ta11"], population=8, generations=9, target=[5000, 1], check_every=2)
    assert res.generations == 9 and res.optimal.tolist() == [True, False]
    res = D.case_driver(twin, "ta01", population=8, generations=9, target=5000, check_every=2)
    assert res.generations == 2 and res.optimal.tolist() == [True]       # the first check ends it


def test_driver_seed_rules_twin(twin):
    """the SPT table is individual 0 of generation 0: at delta 0.5 it decodes to 1605 on ta01"""
    from jssenv_amd import search
    res = search.brkga_search("ta01", population=16, generations=0, delta=0.5, seed_rules=("SPT",), _backend=twin)
    assert res.history.shape == (1, 1) and res.history[0, 0] <= 1605 and res.makespan[0] == res.history[0, 0]
    assert twin.numpy(res.env.evaluate_order(res.rank))[0] == res.makespan[0]


def test_driver_polish_twin(twin):
    from jssenv_amd import search
    plain = D.case_driver(twin, ["ta01", "ta11"], population=8, generations=3)
    polished = D.case_driver(twin, ["ta01", "ta11"], population=8, generations=3, polish=20)
    assert (polished.makespan <= plain.makespan).all() and np.array_equal(polished.history, plain.history)
    assert np.array_equal(polished.keys.shape, plain.keys.shape)
    again = search.brkga_search(["ta01", "ta11"], population=8, generations=3, polish=20, _backend=twin)
    assert np.array_equal(again.makespan, polished.makespan) and np.array_equal(again.rank, polished.rank)


def test_driver_emu(emu):
    """(the emulator backend carries no jss_bound: a search without a target)"""
    D.case_driver(emu, "ta01", population=3, generations=1, seed_rules=("SPT",), target=None)


@pytest.mark.gpu
def test_driver_gpu(hip):
    D.case_driver(hip, ["ta01", "ta11"], population=16, generations=6)


def test_driver_refusals(twin):
    from jssenv_amd import BatchedJssEnv, search
    for bad in (dict(population=0), dict(population=4097), dict(generations=-1), dict(polish=-1), dict(check_every=0), dict(rho=1.5),
                dict(delta=-0.1), dict(elite=0.8, mutants=0.8), dict(tenure=65), dict(target="upper"), dict(seed_rules=("FIFO",)),
                dict(population=1, seed_rules=("SPT", "MWR"))):
        with pytest.raises(ValueError):
            search.brkga_search("ta01", _backend=twin, **dict(dict(population=4, generations=1), **bad))
    with pytest.raises(ValueError):
        search.brkga_search([], _backend=twin)
    with pytest.raises(NotImplementedError):
        search.brkga_search(BatchedJssEnv("ta01", batch=2, _backend=twin))


# ---- 7. the env classes and dispatching ------------------------------------------------------------------------------------------------
def test_facade_and_refusals(twin):
    from jssenv_amd import BatchedJssEnv, dispatching
    from jssenv_amd.bucketed import BucketedJssEnv
    from jssenv_amd.facade import JssEnv
    from jssenv_amd.vector import JssVectorEnv
    n = lambda x: np.asarray(twin.numpy(x))   # noqa: E731
    spt = dispatching.rule_keys("ta01", "SPT")
    env = JssEnv({"instance_path": "ta01"}, _backend=twin)
    env.reset()
    assert env.decode_keys(spt) == 1966 and isinstance(env.decode_keys(spt, 0.5), int) and env.decode_keys(spt, 0.5) == 1605
    mk, start, info = env.decode_keys(spt, 0.0, start=True, info=True)
    assert mk == 1462 and start.shape == (15, 15) and info.tolist() == [51, 4, 0, 0] and env.evaluate_order(start) == 1462
    b = BatchedJssEnv("ta01", batch=2, _backend=twin)
    with pytest.raises(RuntimeError):
        b.decode_keys(spt)                                             # never reset
    b.reset()
    assert n(b.decode_keys(spt)).tolist() == [1966, 1966]
    assert n(b.decode_keys(np.stack([spt] * 3), [0, 1, 0], np.array([1.0, 0.5, 0.0]))).tolist() == [1966, 1605, 1462]
    assert n(b.decode_keys(spt, [1, 1, 0, 5], 0.5)).tolist() == [1605, 1605, 1605, -1]
    for bad in (dict(keys=np.zeros((15, 14), np.int32)), dict(keys=np.zeros((3, 15, 15), np.int32)), dict(keys=np.zeros(15, np.int32)),
                dict(delta=1.5), dict(delta=-0.5), dict(delta=np.array([0.5, 2.0])), dict(delta=np.array([0.5])),
                dict(keys=np.zeros((3, 15, 15), np.int32), parents=[0, 1]), dict(parents=[[0, 1]])):
        with pytest.raises(ValueError):
            b.decode_keys(**dict(dict(keys=spt), **bad))
    # evolve_keys: shapes, and the refusals of its arguments
    keys, order = b.evolve_keys((8, 15, 15), None, 4, 0, 4, seed=3)
    assert n(keys).shape == (8, 15, 15) and n(order).tolist() == [0, 1, 2, 3] * 2
    nxt, order = b.evolve_keys(keys, np.array([5, 3, -1, 3, 1, 1, 1, 0], np.int32), 4, 1, 1)
    assert n(order).tolist() == [1, 3, 0, 2, 3, 0, 1, 2] and np.array_equal(n(nxt)[0], n(keys)[1]) and np.array_equal(n(nxt)[4], n(keys)[7])
    for bad in (dict(pop=0), dict(pop=4097), dict(pop=3), dict(elite=3, mutants=2), dict(elite=0, mutants=2), dict(rho=1.5), dict(fitness=None),
                dict(fitness=np.zeros(7, np.int32)), dict(elite=-1)):
        with pytest.raises(ValueError):
            b.evolve_keys(**dict(dict(keys=keys, fitness=np.zeros(8, np.int32), pop=4, elite=1, mutants=1), **bad))
    for cls in (BucketedJssEnv, JssVectorEnv):
        for call in (cls.decode_keys, cls.evolve_keys):
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
            env.decode_keys(np.zeros((15, 15), np.int32))
    finally:
        env._session = None


def test_dispatching(twin):
    from jssenv_amd import dispatching
    spt, mwr = dispatching.rule_keys("ta01", "SPT"), dispatching.rule_keys("ta01", "MWR")
    pop = np.stack([spt, mwr])
    assert dispatching.evaluate_keys("ta01", pop, _backend=twin).tolist() == [1462, 1491]           # the default: the env's decoder
    assert dispatching.evaluate_keys("ta01", pop, _backend=twin, decoder="env").tolist() == [1462, 1491]
    assert dispatching.evaluate_keys("ta01", pop, _backend=twin, decoder="active").tolist() == [1966, 1589]
    mk, start = dispatching.evaluate_keys("ta01", pop, _backend=twin, decoder="active", delta=0.5, return_solution=True)
    assert mk.tolist() == [1605, 1521] and mk.dtype == np.int64 and start.shape == (2, 15, 15)
    with pytest.raises(ValueError):
        dispatching.evaluate_keys("ta01", pop, _backend=twin, decoder="passive")
    back = dispatching.keys_from_schedule(np.array([[0, 5, -1], [3, 0, -1]]))
    assert back.dtype == np.int32 and back.tolist() == [[0, -5, 0], [-3, 0, 0]]
    # the round trip through the population call: the start times of an active decode come back
    _, active = dispatching.evaluate_keys("ta01", pop, _backend=twin, decoder="active", return_solution=True)
    again = dispatching.evaluate_keys("ta01", dispatching.keys_from_schedule(active), _backend=twin, decoder="active", return_solution=True)
    assert again[0].tolist() == [1966, 1589] and np.array_equal(again[1], active)


# ---- 8. ABI mirror, exports and resources -----------------------------------------------------------------------------------------------
def test_abi_mirror():
    import ctypes as C
    import re
    from jssenv_amd import _abi
    assert (_abi.ABI_VERSION, _abi.ORDER_VERSION, _abi.TABU_VERSION, _abi.BLOCK_VERSION, _abi.RELINK_VERSION, _abi.DECODE_VERSION) == (14, 1, 1, 1, 1, 1)
    assert _abi.DECODE_SYMBOLS == ("jss_decode_keys", "jss_keys_evolve") and _abi.DECODE_NI == 4 and _abi.EVOLVE_MAX_POP == 4096
    others = (_abi.SYMBOLS + _abi.SEARCH_SYMBOLS + _abi.BEAM_SYMBOLS + _abi.BOUND_SYMBOLS + _abi.ORDER_SYMBOLS + _abi.TABU_SYMBOLS
              + _abi.BLOCK_SYMBOLS + _abi.RELINK_SYMBOLS)
    assert not set(_abi.DECODE_SYMBOLS) & set(others)
    header = open(os.path.join(K.ROOT, "include", "jss_decode.h")).read()
    assert "#define JSS_DECODE_VERSION 1" in header and f"#define JSS_DECODE_NI {_abi.DECODE_NI}" in header
    assert f"#define JSS_EVOLVE_SEED_XOR 0x{_abi.EVOLVE_SEED_XOR:016X}ULL" in header and f"#define JSS_EVOLVE_MAX_POP {_abi.EVOLVE_MAX_POP}" in header
    for struct, cls, ints, count in (("JssDecode", _abi.JssDecode, ("n", "stride", "delta_q16"), 9),
                                     ("JssEvolve", _abi.JssEvolve, ("groups", "pop", "region", "n_elite", "n_mutant", "rho_q16", "generation"), 12)):
        body = header[header.index(f"typedef struct {struct} {{"):header.index(f"}} {struct};")]
        names = [f for f, _ in cls._fields_]
        where = [min(body.index(t) for t in (f" {f};", f"*{f};") if t in body) for f in names]
        assert where == sorted(where) and len(set(where)) == len(where)
        assert re.sub(r"/\*.*?\*/", "", body, flags=re.S).count(";") == len(names) == count        # one member per field, and no others
        assert all((t is C.c_int32) == (f in ints) for f, t in cls._fields_ if f != "seed")
    assert dict(_abi.JssEvolve._fields_)["seed"] is C.c_uint64 and _abi.JssEvolve.seed.offset == 32 and C.sizeof(_abi.JssEvolve) == 72
    for name, version in (("jss_relink.h", "JSS_RELINK_VERSION 1"), ("jss_keys.h", "JSS_KEYS_VERSION 1"), ("jss_order.h", "JSS_ORDER_VERSION 1")):
        assert f"#define {version}" in open(os.path.join(K.ROOT, "include", name)).read()


def test_exports():
    """the two symbols come from libjss_decode_hip.so and the twin, and from none of the other seven HIP libraries, none of whose
    symbols is in the new one"""
    from jssenv_amd import _abi, build
    build.build_extension()                            # (all eight HIP libraries; nothing to do after build())
    twin_symbols, own = K.exported(build.build_cpu_twin()), K.exported(build.DECODE_OUT)
    for name in _abi.DECODE_SYMBOLS:
        assert name in own and name in twin_symbols
        for other in (build.OUT, build.BEAM_OUT, build.BOUND_OUT, build.ORDER_OUT, build.TABU_OUT, build.BLOCK_OUT, build.RELINK_OUT):
            assert name not in K.exported(other)
    for other in (_abi.SYMBOLS + _abi.SEARCH_SYMBOLS + _abi.BEAM_SYMBOLS + _abi.BOUND_SYMBOLS + _abi.ORDER_SYMBOLS + _abi.TABU_SYMBOLS
                  + _abi.BLOCK_SYMBOLS + _abi.RELINK_SYMBOLS):
        assert other not in own, other


def test_decode_kernel_resources():
    """libjss_decode_hip.so holds exactly its three kernels: no scratch, no spills; the decode kernel's LDS is the dynamic
    allocation the host sizes, at most 64 KB per wavefront (decode_lds_bytes: what a larger shape gets is JSS_E_LDS, see
    case_abi_errors); the ranking kernel's is its 16 KB of fitness values"""
    rows = D.decode_kernel_rows()
    assert [r[0].split("(")[0] for r in rows] == ["jss_decode_kernel", "jss_evolve_children_kernel", "jss_evolve_rank_kernel"]
    for _, _, _, vspill, sspill, scratch, lds in rows:
        assert scratch == 0 and vspill == 0 and sspill == 0 and lds <= 64 * 1024
    assert rows[0][6] == 0 and rows[2][6] == 4 * 4096
    for jmax, mmax, fits in ((15, 15, True), (100, 20, True), (128, 63, True), (128, 64, False)):
        entries8 = (jmax * mmax + 7) // 8 * 8
        assert (8 * entries8 + 256 <= 64 * 1024) == fits


def test_decode_library_is_ignored_by_git():
    out = subprocess.run(["git", "check-ignore", "jssenv_amd/libjss_decode_hip.so", "tests/emu/libjss_decode_emu.so"], cwd=K.ROOT,
                         capture_output=True, text=True)
    if out.returncode == 128:                          # (not a git checkout: nothing to ask)
        return
    assert out.stdout.split() == ["jssenv_amd/libjss_decode_hip.so", "tests/emu/libjss_decode_emu.so"]


# ---- 9. the twin's entry points under the sanitizers, in a program of their own ------------------------------------------------------
def test_twin_stand_alone_under_asan_and_ubsan(tmp_path):
    """tests/decode_twin_main.cpp and the twin's source in one program with AddressSanitizer and UndefinedBehaviorSanitizer: the
    "hand" and "zeros" cases and two generations; its printed lines are the mirrors' results"""
    from jssenv_amd import search
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "decode_twin_san")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(K.ROOT, "include"),
                           os.path.join(K.ROOT, "jssenv_amd", "csrc", "jss_cpu.cpp"), os.path.join(K.ROOT, "tests", "decode_twin_main.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", OMP_NUM_THREADS="2")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "DECODE-TWIN-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    lines = out.stdout.splitlines()
    want = []
    for name, keys in (("hand", D.HAND_KEYS), ("zeros", D.ZEROS_KEYS)):
        host = D.case_state(name)["host"]
        for delta in (65536, 32768, 0):
            mk, start, info = search.decode_reference(host["env_const"], host["ops"], keys, None, delta)
            want.append(f"{name} {delta} makespan {mk[0]} info {' '.join(str(x) for x in info[0])} start {' '.join(str(x) for x in start[0].reshape(-1))}")
        mk = search.decode_reference(host["env_const"], host["ops"], np.stack([np.asarray(keys)] * 4), [0, 5, 0, 1], [0, 0, 65537, 65536])[0]
        want.append(f"{name} candidates {' '.join(str(x) for x in mk)}")
    assert [D.HAND_RESULTS[d][1] for d in (65536, 32768, 0)] == [int(want[k].split()[3]) for k in range(3)]
    keys_in = ((np.arange(3 * 8 * 12, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32).reshape(24, 12)
    fitness = np.array([-1 if i % 5 == 3 else (i * 7) % 4 for i in range(24)], np.int32)

    def checksum(rows):
        total = 0
        for x in rows.reshape(-1).astype(np.int64):
            total = (total * 31 + (int(x) & 0xFFFFFFFF)) & 0xFFFFFFFF
        return total

    out_keys, by_rank = search.evolve_reference(keys_in, fitness, 3, 8, 2, 2, 45875, 4, 0x0123456789ABCDEF)
    want.append(f"evolve checksum {checksum(out_keys)} by_rank {' '.join(str(x) for x in by_rank)}")
    want.append(f"fresh checksum {checksum(search.evolve_reference(None, None, 3, 8, 0, 8, 45875, 0, 0x0123456789ABCDEF, region=12)[0])}")
    assert lines[:len(want)] == want, (lines, want)
