"""jss_multi_step_logits: the masked draw from a policy's logits fused into the step, over several env sets in ONE grid --
BucketedJssEnv.step_logits and BatchedJssEnv.step_logits on a batch dealt out by shape class.  On the host against the CPU twin
and the kernel source under the SIMT emulator (both kernel flavours); on the MI355X against the HIP library, at test sizes and
at BASELINE config 5's full size."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import multi_logits_cases as ML  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def twin():
    from jssenv_amd.env import CpuBackend
    return CpuBackend()


@pytest.fixture(scope="module", params=["auto", "wave"])
def emu(request):
    from emu_backend import EmuBackend
    return EmuBackend(default_kernel=request.param)


@pytest.fixture(scope="module", params=["auto", "wave"])
def hip(request):
    from jssenv_amd.env import HipBackend
    be = HipBackend("cuda:0")
    assert be.lib.jss_backend() == b"hip:gfx950"
    be.default_kernel = request.param
    return be


# ---- host: the twin ----------------------------------------------------------------------------------------------------
def test_bucketed_vs_buckets_twin(twin):
    ML.case_bucketed_vs_buckets(twin, batch=24, steps=24)


def test_by_shape_vs_ranges_twin(twin):
    ML.case_by_shape_vs_ranges(twin, batch=24, steps=24)


def test_bucketed_vs_padded_twin(twin):
    ML.case_bucketed_vs_padded(twin, n_envs=24, steps=40)


def test_fallback_and_errors_twin(twin):
    ML.case_fallback_and_errors(twin)


def test_edges_through_grid_twin(twin):
    ML.case_edges_through_grid(twin, batch=24, steps=24)


def test_bucketed_step_logits_refuses_before_reset(twin):
    from jssenv_amd.bucketed import BucketedJssEnv
    env = BucketedJssEnv(ML.ragged_population(), batch=6, _backend=twin)
    per = {k: np.zeros((b.batch, b.jmax + 1), np.float32) for k, b in env._each()}
    with pytest.raises(RuntimeError):
        env.step_logits(per)
    env.reset()
    with pytest.raises(ValueError):
        env.step_logits(per, temperature=-1.0)
    k, b = env._each()[0]
    with pytest.raises(ValueError):
        env.step_logits({**per, k: np.zeros((b.batch, b.jmax), np.float32)})


# ---- host: the kernel source under the emulator --------------------------------------------------------------------------
def test_bucketed_vs_buckets_emu(emu):
    ML.case_bucketed_vs_buckets(emu, batch=12, steps=12)


def test_by_shape_vs_ranges_emu(emu):
    ML.case_by_shape_vs_ranges(emu, batch=12, steps=10)


def test_bucketed_vs_padded_emu(emu):
    ML.case_bucketed_vs_padded(emu, n_envs=12, steps=12)


def test_fallback_and_errors_emu(emu):
    ML.case_fallback_and_errors(emu, steps=2)


def test_edges_through_grid_emu(emu):
    ML.case_edges_through_grid(emu, batch=12, steps=12)


# ---- the kernel's resources -----------------------------------------------------------------------------------------------
def test_multi_logits_kernel_keeps_the_grid_step_occupancy():
    """The fused grid's kLogits kernel (jss_multi_kernel<9>) uses no scratch and runs at the wavefronts per SIMD of the grid's
    kStep kernel (jss_multi_kernel<1>): 512 / VGPRs rounded up to 8, at most 8"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import LLVM, kernel_resources
    if not os.path.isfile(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf on this host")
    from jssenv_amd.build import build_extension
    rows = {n: (v, vs, scratch) for n, v, _, vs, _, scratch in kernel_resources(build_extension())}
    occ = lambda v: min(8, 512 // ((v + 7) // 8 * 8))        # noqa: E731
    lg, step = "jss_multi_kernel<9>(MultiParams)", "jss_multi_kernel<1>(MultiParams)"
    assert lg in rows, sorted(n for n in rows if "multi" in n)
    assert rows[lg][1] == 0 and rows[lg][2] == 0, f"{lg} uses scratch: {rows[lg]}"
    assert occ(rows[lg][0]) == occ(rows[step][0]), f"{lg}: {occ(rows[lg][0])} waves per SIMD, {step}: {occ(rows[step][0])}"


# ---- the MI355X ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bucketed_vs_buckets_hip(hip):
    ML.case_bucketed_vs_buckets(hip, batch=96, steps=30)


@pytest.mark.gpu
def test_by_shape_vs_ranges_hip(hip):
    ML.case_by_shape_vs_ranges(hip, batch=96, steps=30)


@pytest.mark.gpu
def test_bucketed_vs_padded_hip(hip):
    ML.case_bucketed_vs_padded(hip, n_envs=96, steps=40)


@pytest.mark.gpu
def test_fallback_and_errors_hip(hip):
    ML.case_fallback_and_errors(hip)


@pytest.mark.gpu
def test_edges_through_grid_hip(hip):
    ML.case_edges_through_grid(hip, batch=96, steps=30)


@pytest.mark.gpu
def test_config5_full_size_hip(hip):
    if hip.default_kernel != "auto":
        pytest.skip("full size: the default kernel choice only")
    ML.case_config5_full_size(hip)
