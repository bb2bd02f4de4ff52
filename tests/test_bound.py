"""jss_bound (include/jss_bound.h) and BatchedJssEnv.lower_bound: makespan lower bounds of states and of candidate moves, and the
per-operation earliest starts.  On the host against the CPU twin and the kernel source under the SIMT emulator; on the MI355X
against libjss_bound_hip.so."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import bound_cases as K  # noqa: E402

NAMES = list(K.CASES)


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


# ---- 1. anchors of the mirror --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.SIX)
def test_anchors_mirror(twin, name):
    """the NumPy mirror itself at reset: the listed lower_bound / job_bound"""
    from jssenv_amd import BatchedJssEnv
    env = BatchedJssEnv(name, batch=1, _backend=twin)
    env.reset()
    lower, jb, _ = K.reference(K.host_arrays(env))
    assert (int(lower[0]), int(jb[0])) == K.ANCHORS[name][:2]


@pytest.mark.parametrize("name", K.SIX)
def test_anchors_twin(twin, name):
    K.case_anchor(twin, name)


def test_hand_case_twin(twin):
    K.case_hand(twin)


def test_hand_case_emu(emu):
    K.case_hand(emu)


def test_hand_case_mirror():
    """the 2 x 2 hand case on the mirror alone, from arrays written out here"""
    from jssenv_amd import _abi
    hdr = np.zeros((1, _abi.NH), np.int32)
    const = np.zeros((1, _abi.NC), np.int32)
    const[0, [_abi.C_JOBS, _abi.C_MACHINES]] = 2
    ops = np.array([[[0 << 16 | 3, 1 << 16 | 2], [1 << 16 | 4, 0 << 16 | 1]]], np.int32)
    rem = np.array([[[5, 2], [5, 1]]], np.int32)
    sol = np.full((1, 2, 2), -1, np.int32)
    lower, jb, est = K.search.lower_bound_reference(hdr, const, sol, ops, rem, est_fill=K.FILL)
    assert est[0].tolist() == [[0, 3], [0, 4]] and jb.tolist() == [5] and lower.tolist() == [6]
    lower, jb, est = K.search.lower_bound_reference(hdr, const, sol, ops, rem, [0, 0, 0, 0], [1, 2, -1, 3], est_fill=K.FILL)
    assert lower.tolist() == [6, 6, 6, -1] and jb.tolist() == [6, 5, 5, -1] and (est[3] == K.FILL).all()


@pytest.mark.gpu
def test_anchors_gpu(hip):
    K.case_hand(hip)
    for name in ("ta01", "ta41"):
        K.case_anchor(hip, name)


# ---- 2. the backends against the mirror ----------------------------------------------------------------------------------------
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


def test_api_twin(twin):
    K.case_api(twin)


@pytest.mark.gpu
def test_api_gpu(hip):
    K.case_api(hip)


def test_facade_and_refusals(twin):
    from jssenv_amd import BatchedJssEnv
    from jssenv_amd.facade import JssEnv
    env = JssEnv({"instance_path": "ta01"}, _backend=twin)
    env.reset()
    assert env.lower_bound() == 1005 and isinstance(env.lower_bound(), int)
    b = BatchedJssEnv("ta01", batch=2, _backend=twin)
    with pytest.raises(RuntimeError):
        b.lower_bound()                                # never reset


# ---- 3. properties along episodes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.SIX)
def test_properties_twin(twin, name):
    """whole random episodes on the twin; the columns against lookahead("SPT") at every 5th step of ta01, rarer on the others"""
    K.case_properties(twin, name, B=4 if name == "ta01" else 2, columns_every=5 if name == "ta01" else 60)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ta01", "syn50x20"])
def test_properties_gpu(hip, name):
    from jssenv_amd import instances as I
    inst = name if name == "ta01" else I.taillard_instance(50, 20, 4711, 815, name="syn50x20")
    K.case_properties(hip, inst, B=4, columns_every=40)


# ---- 4. argument checks and bindings ----------------------------------------------------------------------------------------------
def test_abi_errors_twin(twin):
    K.case_abi_errors(twin)


def test_abi_errors_emu(emu):
    K.case_abi_errors(emu)


@pytest.mark.gpu
def test_abi_errors_gpu(hip):
    K.case_abi_errors(hip)


def test_abi_mirror():
    from jssenv_amd import _abi
    assert _abi.ABI_VERSION == 14 and _abi.BOUND_VERSION == 1 and _abi.BOUND_SYMBOLS == ("jss_bound",)
    assert "jss_bound" not in _abi.SYMBOLS + _abi.SEARCH_SYMBOLS + _abi.BEAM_SYMBOLS
    assert [f for f, _ in _abi.JssBound._fields_] == ["n", "parent", "action", "mask", "lower_bound", "job_bound", "est_start"]
    header = open(os.path.join(K.ROOT, "include", "jss_bound.h")).read()
    assert "#define JSS_BOUND_VERSION 1" in header
    order = [header.index(f" {f};") if f == "n" else header.index(f"*{f};") for f, _ in _abi.JssBound._fields_]
    assert order == sorted(order)
    assert "#define JSS_ABI_VERSION 14" in open(os.path.join(K.ROOT, "include", "jss_hip.h")).read()


def test_exports():
    """jss_bound comes from libjss_bound_hip.so and the twin, and from neither of the other two HIP libraries"""
    from jssenv_amd import build
    build.build_extension()                            # (all three HIP libraries; nothing to do after build())
    assert "jss_bound" in K.exported(build.BOUND_OUT) and "jss_bound" in K.exported(build.build_cpu_twin())
    assert "jss_bound" not in K.exported(build.OUT) and "jss_bound" not in K.exported(build.BEAM_OUT)
    assert "jss_beam_select" not in K.exported(build.BOUND_OUT) and "jss_step" not in K.exported(build.BOUND_OUT)


# ---- 5. resources -----------------------------------------------------------------------------------------------------------------
def test_bound_kernel_resources():
    """libjss_bound_hip.so holds the one kernel: no scratch, no spills, at most 64 KB of LDS"""
    rows = K.bound_kernel_rows()
    assert len(rows) == 1 and rows[0][0].startswith("jss_bound_kernel(")
    _, _, _, vspill, sspill, scratch, lds = rows[0]
    assert scratch == 0 and vspill == 0 and sspill == 0 and 0 < lds <= 64 * 1024


def test_bound_library_is_ignored_by_git():
    out = subprocess.run(["git", "check-ignore", "jssenv_amd/libjss_bound_hip.so", "tests/emu/libjss_bound_emu.so"], cwd=K.ROOT,
                         capture_output=True, text=True)
    if out.returncode == 128:                          # (not a git checkout: nothing to ask)
        return
    assert out.stdout.split() == ["jssenv_amd/libjss_bound_hip.so", "tests/emu/libjss_bound_emu.so"]
