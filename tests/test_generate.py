"""jss_generate / BatchedJssEnv.generated: Taillard instances drawn on the device, fresh for every episode.  On the host
against the CPU twin and the kernel source under the SIMT emulator; on the MI355X against the HIP library, at test sizes
and at full size against the twin."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import generate_cases as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(15, 15, (1, 99)), (20, 15, (1, 99)), (50, 20, (1, 99)), (100, 20, (1, 99)), (1, 1, (1, 99)), (64, 1, (1, 99)),
          (128, 64, (1, 99)), (128, 64, (1, 65535))]
FRESH_PATHS = ["step", "step_logits", "reset_action", "reset_which", "vector_step", "vector_step_logits"]


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


# ---- host: the twin ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J,M,dur", SHAPES)
def test_matches_host_generator_twin(twin, J, M, dur):
    inst = G.case_matches_host_generator(twin, 12, J, M, dur)
    if dur[1] == 65535:
        assert inst[:, 4].min() > 1 << 24          # sum_op beyond float32's exact integers: the reciprocal's input rounds


def test_padding_twin(twin):
    G.case_matches_host_generator(twin, 9, 7, 5, pad=(4, 3))


def test_published_ta01_twin(twin):
    G.case_published_ta01(twin)


def test_derived_seeds_twin(twin):
    G.case_derived_seeds(twin)


def test_sharding_twin(twin):
    G.case_sharding(twin)


def test_which_and_padding_twin(twin):
    G.case_which_and_padding(twin)


def test_argument_errors_twin(twin):
    G.case_argument_errors(twin.lib)


def test_same_trajectory_as_host_generator_twin(twin):
    G.case_same_trajectory_as_host_generator(twin)
    G.case_same_trajectory_as_host_generator(twin, B=6, J=20, M=20, steps=120)
    G.case_same_trajectory_as_host_generator(twin, B=3, J=40, M=8, steps=100, records="full")


@pytest.mark.parametrize("path", FRESH_PATHS)
def test_fresh_instances_twin(twin, path):
    G.case_fresh_instances(twin, path)


def test_refusals_twin(twin):
    G.case_refusals(twin)


def test_checkpoint_twin(twin, tmp_path):
    G.case_checkpoint(twin)
    G.case_checkpoint(twin, tmp_path)


def test_host_generator_defaults_unchanged():
    """the new keywords of synthetic_arrays / synthetic_packed leave what they return without them as it was"""
    from jssenv_amd import instances as I
    pk = I.synthetic_packed(5, 6, 4)
    ref = I.pack_batch(I.synthetic_batch(5, 6, 4))
    for k in ("ops", "rem", "inst", "jobs", "machines", "max_time_op", "max_time_jobs", "sum_op"):
        assert np.array_equal(getattr(pk, k), getattr(ref, k)), k
    idx = np.arange(5)
    pk2 = I.synthetic_packed(5, 6, 4, seeds=(1 + 2 * idx, 2 + 2 * idx))
    assert np.array_equal(pk2.ops, pk.ops) and np.array_equal(pk2.inst, pk.inst)


# ---- host: the kernel source under the emulator ---------------------------------------------------------------------------
@pytest.mark.parametrize("J,M,dur", [(15, 15, (1, 99)), (100, 20, (1, 99)), (1, 1, (1, 99)), (64, 1, (1, 99)),
                                     (128, 64, (1, 65535))])
def test_matches_host_generator_emu(emu, J, M, dur):
    G.case_matches_host_generator(emu, 70, J, M, dur)


def test_padding_and_ta01_emu(emu):
    G.case_matches_host_generator(emu, 9, 7, 5, pad=(4, 3))
    G.case_matches_host_generator(emu, 5, 60, 6, pad=(10, 2))      # two jobs per lane
    G.case_published_ta01(emu)


def test_derived_seeds_and_sharding_emu(emu):
    G.case_derived_seeds(emu)
    G.case_sharding(emu)


def test_which_and_padding_emu(emu):
    G.case_which_and_padding(emu)


def test_argument_errors_emu(emu):
    G.case_argument_errors(emu.lib)


def test_argument_errors_hip_library():
    """the HIP library's checks run on the host, before anything is launched"""
    import ctypes
    from jssenv_amd import _abi
    from jssenv_amd.build import build_extension
    G.case_argument_errors(_abi.bind(ctypes.CDLL(build_extension())))


def test_same_trajectory_as_host_generator_emu(emu):
    G.case_same_trajectory_as_host_generator(emu, B=8, steps=60)


@pytest.mark.parametrize("path", ["step", "step_logits", "reset_action", "vector_step"])
def test_fresh_instances_emu(emu, path):
    G.case_fresh_instances(emu, path, steps=40)


def test_checkpoint_emu(emu):
    G.case_checkpoint(emu)


def test_generate_kernel_resources():
    """the generator kernel keeps its working set in registers and LDS (no scratch, no spills: the swap loop's row lives in
    LDS) at 8 wavefronts per SIMD -- the row profiles/r09_generate/kernel_resources.txt records"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import LLVM, kernel_resources
    if not os.path.isfile(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf on this host")
    from jssenv_amd.build import build_extension
    rows = {n: r for n, *r in kernel_resources(build_extension())}
    name = "jss::jss_generate_kernel(jss::GenParams)"
    assert name in rows, sorted(rows)[:5]
    vgpr, _, vspill, sspill, scratch = rows[name]
    assert (vspill, sspill, scratch) == (0, 0, 0)
    assert min(8, 512 // ((vgpr + 7) // 8 * 8)) == 8, vgpr


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("J,M,dur", SHAPES)
def test_matches_host_generator_hip(hip, J, M, dur):
    G.case_matches_host_generator(hip, 300, J, M, dur)


@pytest.mark.gpu
def test_small_cases_hip(hip):
    G.case_matches_host_generator(hip, 9, 7, 5, pad=(4, 3))
    G.case_published_ta01(hip)
    G.case_derived_seeds(hip)
    G.case_sharding(hip)
    G.case_which_and_padding(hip)


@pytest.mark.gpu
def test_same_trajectory_and_checkpoint_hip(hip):
    G.case_same_trajectory_as_host_generator(hip)
    G.case_same_trajectory_as_host_generator(hip, B=6, J=20, M=20, steps=120)
    G.case_checkpoint(hip)
    G.case_refusals(hip)


@pytest.mark.gpu
@pytest.mark.parametrize("path", FRESH_PATHS)
def test_fresh_instances_hip(hip, path):
    G.case_fresh_instances(hip, path)


@pytest.mark.gpu
@pytest.mark.parametrize("B,J,M", [(65536, 15, 15), (8192, 50, 20)])
def test_full_size_matches_twin_hip(hip, twin, B, J, M):
    """HIP jss_generate = the twin's, bit for bit, at full size: every env, and a sparse `which` (+ -2 actions)"""
    rng = np.random.default_rng(B)
    eps = rng.integers(0, 1000, B).astype(np.int32)
    fill = rng.integers(-2**31, 2**31 - 1, (B, J, M), dtype=np.int64).astype(np.int32)
    tables = (fill, fill[:, ::-1].copy(), rng.integers(-99, 99, (B, 12)).astype(np.int32))
    which = (rng.random(B) < 1 / 225).astype(np.uint8)
    actions = np.where(rng.random(B) < 1 / 500, -2, 0).astype(np.int32)
    for kw in ({}, {"which": which}, {"which": which, "actions": actions}):
        got = G.raw_generate(hip, B, J, M, episodes=eps, seed=12345, tables=tables, env_id_base=7, **kw)
        exp = G.raw_generate(twin, B, J, M, episodes=eps, seed=12345, tables=tables, env_id_base=7, **kw)
        assert got[0] == exp[0] == 0
        for k in (1, 2, 3):
            assert np.array_equal(got[k], exp[k]), (kw.keys(), k)
    assert not np.array_equal(got[1], tables[0])


@pytest.mark.gpu
def test_fresh_vector_env_step_logits_full_size_hip(hip, twin):
    """a 65 536-env fresh=True JssVectorEnv on HIP and on the twin, fed the same logits for 300 steps, ends in the same state
    and on the same tables"""
    import torch
    from jssenv_amd.vector import JssVectorEnv
    B, J, M = 65536, 15, 15
    envs = {name: JssVectorEnv.generated(J, M, B, instance_seed=2024, _backend=be) for name, be in (("hip", hip), ("cpu", twin))}
    for v in envs.values():
        v.reset(seed=6)
    g = torch.Generator().manual_seed(6)
    for _ in range(300):
        logits = torch.randn(B, J + 1, generator=g) * 2
        envs["hip"].step_logits(logits.to(hip.device))
        envs["cpu"].step_logits(logits.numpy())
    a, b = envs["hip"].env, envs["cpu"].env
    for name in G.STATE:
        assert np.array_equal(G._host(a, name), G._host(b, name)), name
    assert np.array_equal(a.packed.ops, b.packed.ops) and np.array_equal(a.packed.inst, b.packed.inst)
    assert a.stats()["episodes"] > B // 4                      # many envs went through a regeneration
