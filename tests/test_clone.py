"""jss_clone / BatchedJssEnv.fork / copy_from / copy.deepcopy of the facade: env states cloned on the device for search.  On
the host against the CPU twin and the kernel source under the SIMT emulator; on the MI355X against the HIP library, at test
sizes and at full size against the twin."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import clone_cases as K  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def twin():
    from jssenv_amd.env import CpuBackend
    return CpuBackend()


@pytest.fixture(scope="module", params=["auto", "wave"])
def emu(request):
    from emu_backend import EmuBackend
    return EmuBackend(default_kernel=request.param)


@pytest.fixture(scope="module")
def hip():
    from jssenv_amd.env import HipBackend
    be = HipBackend("cuda:0")
    assert be.lib.jss_backend() == b"hip:gfx950"
    return be


def test_abi_mirror():
    from jssenv_amd import _abi
    assert _abi.ABI_VERSION == 14 and _abi.STATE_LAYOUT == 7 and _abi.ERR_BAD_INDEX == 16
    assert "jss_clone" in _abi.SYMBOLS
    assert [f for f, _ in _abi.JssCloneDst._fields_] == ["table_of_env", "ops", "rem", "inst"]


# ---- host: the twin ----------------------------------------------------------------------------------------------------
def test_facade_deepcopy_twin():
    K.case_facade_deepcopy(device="cpu")


@pytest.mark.parametrize("layout", K.LAYOUTS)
def test_exact_copy_and_continuation_twin(twin, layout):
    K.case_exact_copy(twin, layout)


def test_copy_from_twin(twin):
    K.case_copy_from(twin)


def test_abi_errors_twin(twin):
    K.case_abi_errors(twin)


def test_session_refused_twin(twin):
    K.case_session_refused(twin)


def test_divergence_twin(twin):
    K.case_divergence(twin)


def test_pilot_twin(twin):
    K.case_pilot(twin)


# ---- host: the kernel source under the emulator ---------------------------------------------------------------------------
def test_facade_deepcopy_emu(emu):
    K.case_facade_deepcopy(backend=emu)


@pytest.mark.parametrize("layout", K.LAYOUTS)
def test_exact_copy_and_continuation_emu(emu, layout):
    K.case_exact_copy(emu, layout, B=6, n_steps=40)


def test_copy_from_and_errors_emu(emu):
    K.case_copy_from(emu)
    K.case_abi_errors(emu)


def test_divergence_emu_equals_twin(emu, twin):
    a, b = K.case_divergence(emu), K.case_divergence(twin)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_facade_deepcopy_gpu():
    K.case_facade_deepcopy(device="cuda:0")


@pytest.mark.gpu
def test_facade_deepcopy_device_arena_gpu(monkeypatch):
    monkeypatch.setenv("JSSENV_AMD_HOST_ARENA", "0")
    K.case_facade_deepcopy(device="cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", K.LAYOUTS)
def test_exact_copy_and_continuation_gpu(hip, layout):
    K.case_exact_copy(hip, layout, B=24, by_shape=K.BY_SHAPE_FULL if layout == "by_shape" else K.BY_SHAPE_SMALL)


@pytest.mark.gpu
def test_copy_from_and_errors_gpu(hip):
    K.case_copy_from(hip)
    K.case_abi_errors(hip)
    K.case_session_refused(hip)


@pytest.mark.gpu
def test_device_index_gpu(hip, twin):
    """a device index (int64, as torch makes it): no host copy for a shared-table batch; out-of-range entries set
    ERR_BAD_INDEX and touch nothing else; the same clone on the twin gives the same bytes"""
    import torch
    from jssenv_amd import _abi
    out = []
    for be in (hip, twin):
        env = K.make_layout(be, "compact", 8, seed=4)
        env.reset()
        env.rollout("random", n_iter=25, autoreset=False)
        f = env.fork(torch.tensor([3, 3, 0], device="cuda:0") if be is hip else [3, 3, 0])
        env.rollout("random", n_iter=10, autoreset=False)
        before = K.rows_of(f)
        idx = [7, -1, 8]
        f.copy_from(env, torch.tensor(idx, device="cuda:0") if be is hip else [7, -1, 2])
        r = K.rows_of(f)
        if be is hip:
            assert int(r["env_header"][2][_abi.H_STATUS]) & _abi.ERR_BAD_INDEX
            r["env_header"][2][_abi.H_STATUS] &= ~_abi.ERR_BAD_INDEX
            for k, v in r.items():
                assert np.array_equal(v[1:], before[k][1:]), k
        out.append(r)
    for k in out[0]:
        assert np.array_equal(out[0][k][:2], out[1][k][:2]), k


@pytest.mark.gpu
def test_divergence_gpu_equals_twin(hip, twin):
    a, b = K.case_divergence(hip), K.case_divergence(twin)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.gpu
def test_pilot_gpu(hip):
    K.case_pilot(hip)


@pytest.mark.gpu
def test_pilot_full_size_gpu(hip, twin):
    """1 024 mid-episode parents x 64 children = 65 536 envs, bit-identical to the twin"""
    a, acts_a = K.case_pilot(hip, n_parents=1024, children=64, check_oracle=False)
    b, acts_b = K.case_pilot(twin, n_parents=1024, children=64, check_oracle=False)
    assert np.array_equal(acts_a, acts_b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_clone_kernel_resources():
    """the clone kernel of the built library: no scratch, no spills, at most 64 VGPRs (8 wavefronts per SIMD)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    from jssenv_amd.build import build_extension
    rows = [r for r in kernel_resources(build_extension()) if "jss_clone_kernel" in r[0]]      # (built here if build() has not run)
    assert len(rows) == 1
    _, vgpr, _, vspill, sspill, scratch = rows[0]
    assert scratch == 0 and vspill == 0 and sspill == 0 and vgpr <= 64
