"""libjss_onestep_hip.so (include/jss_onestep.h, jssenv_amd/csrc/jss_onestep.hip): the one-step rollout of the flagship class --
packed flavour, one shared instance, compact records -- with write-through stores.

Without a GPU: the header, the library's exports and ``_abi.ONESTEP_SYMBOLS`` agree; descriptors outside the class get the
header's error codes before anything is launched; the shipped kernels use no scratch memory, spill no VGPR and reach the
wavefronts per SIMD that profiles/r26_onestep/kernel_resources.txt records; and the kernel source, compiled against the SIMT
emulator, leaves the bytes the library's own one-step kernel leaves on a few ragged batches.

On the MI355X (-m gpu): the reference is the existing path (``JSS_ONESTEP=0``: jss_rollout / jss_rollout_steps of
libjss_hip.so, which the suite holds to the oracle).  After K steps from identical starts the whole arena -- env headers, job
records, counters, real_obs, action_mask, reward, done, makespan --, the solution and the per-env counters are compared for
equality, through ``rollout(n_iter=1)`` in a loop, ``rollout_steps`` and ``bind_rollout_steps``."""
import contextlib
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(HERE, "emu"), os.path.join(ROOT, "tools"), ROOT]

from jssenv_amd import BatchedJssEnv, _abi, builtin_instance  # noqa: E402
from jssenv_amd.instances import Instance  # noqa: E402

HEADER = os.path.join(ROOT, "include", "jss_onestep.h")
RESOURCES = os.path.join(ROOT, "profiles", "r26_onestep", "kernel_resources.txt")


def tiny_instance():
    """3 jobs x 3 machines by hand: an episode is over after a dozen steps, so 60 steps end and restart it several times"""
    return Instance("onestep_3x3", np.array([[0, 1, 2], [1, 0, 2], [2, 1, 0]], np.int32), np.array([[3, 2, 2], [2, 4, 1], [1, 3, 5]], np.int32))


def instance_of(name):
    return tiny_instance() if name == "3x3" else builtin_instance(name)


@contextlib.contextmanager
def onestep(on):
    old = os.environ.get("JSS_ONESTEP")
    os.environ["JSS_ONESTEP"] = "1" if on else "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["JSS_ONESTEP"]
        else:
            os.environ["JSS_ONESTEP"] = old


# ---- without a GPU --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib_path():
    from jssenv_amd.build import build_onestep_extension
    return build_onestep_extension()


def test_header_exports_and_abi_agree(lib_path):
    text = open(HEADER).read()
    declared = re.findall(r"^int (jss_onestep_\w+)\(", text, flags=re.M)
    assert sorted(declared) == sorted(_abi.ONESTEP_SYMBOLS)
    assert int(re.search(r"#define JSS_ONESTEP_VERSION (\d+)", text).group(1)) == _abi.ONESTEP_VERSION
    lib = _abi.bind_onestep(C.CDLL(lib_path))
    assert lib.jss_onestep_version() == _abi.ONESTEP_VERSION
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line and "jss_" in line.split()[-1] and "_Z" not in line.split()[-1]}
    assert exported == set(_abi.ONESTEP_SYMBOLS)


def _descriptor(**kw):
    """A descriptor of the class with addresses that are never followed: the checks come before any launch."""
    fake = 0x1000
    f = dict(batch=8, jmax=15, mmax=15, n_tables=1, ops=fake, rem=fake, inst=fake, table_of_env=None, env_ids=None, env_id_base=0,
             kernel=0, threads=0, jmin=15, record_ints=_abi.NFC, cr_factor=0.0, jclass=0, mclass=0)
    f.update(kw)
    d = _abi.JssDesc(*[f[name] for name, _ in _abi.JssDesc._fields_])
    s = _abi.JssState(fake, fake, fake, fake, fake, fake)
    o = _abi.JssOut(fake, fake, fake, fake, fake)
    return d, s, o


@pytest.mark.parametrize("change, kind, code", [
    (dict(n_tables=8, record_ints=_abi.NF), 0, _abi.E_SHAPE),            # per-env tables
    (dict(n_tables=8, record_ints=_abi.NFM), 0, _abi.E_SHAPE),           # ... with medium records
    (dict(n_tables=2, table_of_env=0x1000, record_ints=_abi.NF), 0, _abi.E_SHAPE),
    (dict(record_ints=_abi.NF), 0, _abi.E_SHAPE),                        # full records on the shared table
    (dict(record_ints=0), 0, _abi.E_SHAPE),
    (dict(jmax=33), 0, _abi.E_SHAPE),
    (dict(mmax=33), 0, _abi.E_SHAPE),
    (dict(kernel=1), 0, _abi.E_KIND),                                    # JSS_KERNEL_WAVE
    (dict(), 8, _abi.E_KIND),                                            # the weighted rule's and the key tables' kinds are no stock codes
    (dict(), 9, _abi.E_KIND),
    (dict(), _abi.POLICY_CR_F64, _abi.E_KIND),
    (dict(rem=None), _abi.POLICY["MWR"], _abi.E_NULL),                   # (as jss_rollout: the rule reads the work table)
])
def test_outside_the_class_is_refused_before_any_launch(lib_path, change, kind, code):
    lib = _abi.bind_onestep(C.CDLL(lib_path))
    d, s, o = _descriptor(**change)
    streams = (C.c_void_p * 2)()
    assert lib.jss_onestep_rollout(C.byref(d), C.byref(s), C.byref(o), kind, 1, 0, 1, 1, None) == code
    assert lib.jss_onestep_rollout_steps(C.byref(d), C.byref(s), C.byref(o), kind, 1, 0, 3, 1, 2, streams) == code


def test_call_shapes_are_checked(lib_path):
    lib = _abi.bind_onestep(C.CDLL(lib_path))
    d, s, o = _descriptor()
    streams = (C.c_void_p * 2)()
    assert lib.jss_onestep_rollout(C.byref(d), C.byref(s), C.byref(o), 0, 1, 0, 2, 1, None) == _abi.E_SHAPE      # n_iter != 1
    assert lib.jss_onestep_rollout(C.byref(d), C.byref(s), C.byref(o), 0, 1, 0, 0, 1, None) == _abi.E_SHAPE
    assert lib.jss_onestep_rollout(None, C.byref(s), C.byref(o), 0, 1, 0, 1, 1, None) == _abi.E_NULL
    assert lib.jss_onestep_rollout_steps(C.byref(d), C.byref(s), C.byref(o), 0, 1, 0, 3, 1, 0, streams) == _abi.E_SHAPE
    assert lib.jss_onestep_rollout_steps(C.byref(d), C.byref(s), C.byref(o), 0, 1, 0, 3, 1, 17, streams) == _abi.E_SHAPE
    assert lib.jss_onestep_rollout_steps(C.byref(d), C.byref(s), C.byref(o), 0, 1, 0, -1, 1, 2, streams) == _abi.E_SHAPE
    assert lib.jss_onestep_rollout_steps(C.byref(d), C.byref(s), C.byref(o), 0, 1, 0, 3, 1, 2, None) == _abi.E_NULL
    assert lib.jss_onestep_rollout_steps(C.byref(d), C.byref(s), C.byref(o), 0, 1, 0, 0, 1, 2, streams) == 0     # no step: nothing is launched
    d0, _, _ = _descriptor(batch=0)
    assert lib.jss_onestep_rollout(C.byref(d0), C.byref(s), C.byref(o), 0, 1, 0, 1, 1, None) == 0                 # no env: likewise


def test_shipped_kernels_resources(lib_path):
    from kernel_resources import LLVM, kernel_resources
    assert os.path.isfile(os.path.join(LLVM, "llvm-readelf")), "the code object's notes are read with ROCm's llvm-readelf"
    recorded = {}
    for line in open(RESOURCES):
        m = re.match(r"(jss::jss_onestep_kernel<[^>]+>)\s+vgpr\s+(\d+).*waves_per_simd\s+(\d+)", line)
        if m:
            recorded[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    rows = kernel_resources(lib_path)
    assert {r[0] for r in rows} == set(recorded) and len(rows) == 2      # G = 16 and G = 32
    for name, vgpr, _sgpr, vspill, _sspill, scratch in rows:
        assert scratch == 0 and vspill == 0, (name, scratch, vspill)
        waves = min(8, 512 // ((vgpr + 7) & ~7))                         # gfx950: 512 VGPRs per lane and SIMD, granules of 8
        assert waves == recorded[name][1] == 8, (name, vgpr, waves, recorded[name])


# ---- the kernel source under the SIMT emulator ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    from emu_backend import EmuBackend, _HERE as EMU
    out = os.path.join(EMU, "libjss_onestep_emu.so")
    src = [os.path.join(ROOT, "jssenv_amd", "csrc", f) for f in ("jss_onestep.hip", "jss_packed_env.hpp", "jss_common.hpp")] + [HEADER]
    if not os.path.isfile(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in src):
        subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
                               "-Wno-unknown-pragmas", "-I" + EMU, "-I" + os.path.join(ROOT, "include"), src[0], "-o", out])

    class Backend(EmuBackend):
        @property
        def onestep_lib(self):
            return _abi.bind_onestep(C.CDLL(out))
    return Backend()


def snapshot(env):
    be = env.backend
    env.synchronize() if hasattr(env, "synchronize") else None
    return {"arena": be.numpy(env._arena), "solution": be.numpy(env.solution), "counters": be.numpy(env.counters)}


def run(be, inst, batch, K, form, on, kind="random", seed=11, explore=0.0, autoreset=True, n_sub=2, half=False):
    """K one-step rollouts of a fresh batch through `form`, on the new path or the old one; returns the snapshot"""
    with onestep(on):
        env = BatchedJssEnv(instance_of(inst), batch=batch, seed=5, _backend=be)
        assert (env._onestep_lib(_abi.policy_code(kind)) is not None) == on
        if half:
            which = (np.arange(batch) % 2 == 0).astype(np.uint8)
            if batch == 1:
                which[:] = 1
            env.reset(which)
        else:
            env.reset()
        if form == "loop":
            for _ in range(K):
                env.rollout(kind, n_iter=1, seed=seed, autoreset=autoreset, explore=explore)
        elif form == "steps":
            env.rollout_steps(kind, steps=K, n_sub=n_sub, seed=seed, autoreset=autoreset, explore=explore)
        else:
            env.bind_rollout_steps(kind, steps=K, n_sub=n_sub, seed=seed, autoreset=autoreset, explore=explore)()
        return snapshot(env)


_REFERENCE = {}


def reference(be, inst, batch, K, **kw):
    """the existing path, once per configuration (the three forms give the same bytes there: tests/test_hip_parity.py)"""
    key = (id(be), inst, batch, K, tuple(sorted((k, v) for k, v in kw.items() if k != "n_sub")))
    if key not in _REFERENCE:
        _REFERENCE[key] = run(be, inst, batch, K, "loop", False, **kw)
    return _REFERENCE[key]


def same(got, ref, what):
    for name in ref:
        diff = np.flatnonzero(got[name].reshape(-1) != ref[name].reshape(-1))
        assert diff.size == 0, f"{what}: {name} differs in {diff.size} places, first at {diff[:4]}"


FORMS = ("loop", "steps", "bind")


@pytest.mark.parametrize("batch", [1, 5, 9])
def test_emulated_kernel_equals_the_existing_one(emu, batch):
    # 16-lane groups, 4 envs per wavefront: a ragged wavefront, a whole one + a ragged one, a second workgroup
    for inst, K in (("3x3", 30), ("ta01", 12)):
        ref = reference(emu, inst, batch, K)
        for form in FORMS:
            same(run(emu, inst, batch, K, form, True), ref, f"{inst} x {batch}, {form}")


def test_emulated_kernel_32_lane_groups(emu):
    ref = reference(emu, "ta11", 3, 8)
    same(run(emu, "ta11", 3, 8, "steps", True), ref, "ta11 x 3")


# ---- on the MI355X ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    from jssenv_amd.env import HipBackend
    be = HipBackend("cuda:0")
    assert be.name == "hip" and be.onestep_lib.jss_onestep_version() == _abi.ONESTEP_VERSION
    return be


G16_BATCHES = [1, 3, 4, 5, 7, 8, 9, 31, 32, 33, 69]
G32_BATCHES = [1, 2, 3, 4, 5, 17]
SOME_G16 = [5, 33, 69]           # of G16_BATCHES: a ragged second wavefront, a ragged third workgroup, several workgroups


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("batch", G16_BATCHES)
@pytest.mark.parametrize("inst, K", [("3x3", 60), ("ta01", 300)])
def test_sixteen_lane_groups(hip, inst, K, batch, form):
    same(run(hip, inst, batch, K, form, True), reference(hip, inst, batch, K), f"{inst} x {batch}, {form}")


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("batch", G32_BATCHES)
@pytest.mark.parametrize("inst", ["ta11", "ta41"])
def test_thirty_two_lane_groups(hip, inst, batch, form):
    same(run(hip, inst, batch, 120, form, True), reference(hip, inst, batch, 120), f"{inst} x {batch}, {form}")


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["steps", "bind"])
@pytest.mark.parametrize("n_sub", [1, 2, 3])
def test_sub_batch_cuts(hip, n_sub, form):
    same(run(hip, "ta01", 200, 300, form, True, n_sub=n_sub), reference(hip, "ta01", 200, 300), f"n_sub {n_sub}, {form}")


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("batch", SOME_G16)
@pytest.mark.parametrize("autoreset", [True, False])
def test_autoreset_on_and_off(hip, autoreset, batch, form):
    # 300 steps cross the end of a ta01 episode (225 allocations + its NOPEs): reset in place, or frozen
    same(run(hip, "ta01", batch, 300, form, True, autoreset=autoreset), reference(hip, "ta01", batch, 300, autoreset=autoreset),
         f"autoreset {autoreset} x {batch}, {form}")


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("batch", SOME_G16)
@pytest.mark.parametrize("kind, seed, explore", [("random", 11, 0.0), ("random", 977, 0.25), ("SPT", 11, 0.0), ("MWR", 11, 0.125)])
def test_policies(hip, kind, seed, explore, batch, form):
    kw = dict(kind=kind, seed=seed, explore=explore)
    same(run(hip, "ta01", batch, 300, form, True, **kw), reference(hip, "ta01", batch, 300, **kw), f"{kind} x {batch}, {form}")


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("batch", SOME_G16)
def test_never_reset_envs_are_left_alone(hip, batch, form):
    got = run(hip, "ta01", batch, 300, form, True, half=True)
    same(got, reference(hip, "ta01", batch, 300, half=True), f"half reset x {batch}, {form}")
    assert (got["counters"][1::2] == 0).all() and (got["solution"][1::2] == 0).all()
