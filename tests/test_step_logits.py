"""BatchedJssEnv.step_logits / jss_step_logits: the masked categorical draw from a policy's logits (Gumbel-max, log-probability,
entropy) fused into the step.  On the host against the CPU twin and the kernel source under the SIMT emulator (both kernel
flavours); on the MI355X against the HIP library, at test sizes and at full size against the twin."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import logits_cases as L  # noqa: E402

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


# ---- the formula itself -------------------------------------------------------------------------------------------
def test_mirror_rng_is_the_oracles():
    from oracle.oracle import rng_u32
    for seed, env_id, ep, st in ((0, 0, 0, 0), (3, 17, 2, 40), (2**63 + 5, 2**40 + 9, 7, 1)):
        assert int(L.rng_u32(seed, [env_id], [ep], [st])[0]) == rng_u32(seed, env_id, ep, st)


# ---- host: the twin --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("insts,order", [("ta01", None), ("ta41", None), ("ragged", "by_shape")])
def test_greedy_twin(twin, insts, order):
    L.case_greedy(twin, L.ragged_by_shape() if insts == "ragged" else insts, batch=8, steps=60, order=order)


@pytest.mark.parametrize("T", [1.0, 0.5])
@pytest.mark.parametrize("insts,order", [("ta01", None), ("ragged", "by_shape")])
def test_sampled_twin(twin, insts, order, T):
    L.case_sampled(twin, L.ragged_by_shape() if insts == "ragged" else insts, batch=16, steps=120, T=T, order=order)


def test_nope_and_padding_twin(twin):
    L.case_nope_and_padding(twin)


@pytest.mark.parametrize("jobs,machines", [(16, 4), (32, 8), (64, 16), (128, 16)])
def test_nope_fold_twin(twin, jobs, machines):
    L.case_nope_fold(twin, jobs, machines, batch=16)


def test_signed_zero_ties_twin(twin):
    L.case_signed_zero_ties(twin)


def test_broadcast_row_twin(twin):
    L.case_broadcast_row(twin)


def test_determinism_twin(twin):
    L.case_determinism(twin)


def test_autoreset_and_done_twin(twin):
    L.case_autoreset_and_done(twin)


def test_bf16_and_stride_twin(twin):
    L.case_bf16_and_stride(twin)


def test_bad_logits_twin(twin):
    L.case_bad_logits(twin)


def test_distribution_twin(twin):
    L.case_distribution(twin, batch=4096)


def test_vector_env_step_logits(twin):
    from jssenv_amd.vector import JssVectorEnv
    envs = JssVectorEnv("ta01", num_envs=4, to_numpy=True, _backend=twin)
    obs, _ = envs.reset(seed=3)
    for _ in range(30):
        mask = obs["action_mask"]
        obs, rew, term, trunc, infos = envs.step_logits(np.zeros(mask.shape, dtype=np.float32))
        a = infos["action"]
        assert set(infos) == {"action", "logp", "entropy"}
        assert ((a == -2) | mask[np.arange(4), np.maximum(a, 0)]).all()
        assert np.allclose(infos["logp"][a >= 0], -np.log(mask[a >= 0].sum(axis=1)), atol=2e-5)


def test_step_logits_refuses_during_a_session_and_before_reset(twin):
    from jssenv_amd import BatchedJssEnv
    env = BatchedJssEnv("ta01", batch=2, _backend=twin)
    with pytest.raises(RuntimeError):
        env.step_logits(np.zeros((2, 16), dtype=np.float32))
    env.reset()
    with pytest.raises(ValueError):
        env.step_logits(np.zeros((2, 15), dtype=np.float32))
    with pytest.raises(ValueError):
        env.step_logits(np.zeros((2, 16), dtype=np.float32), temperature=-1.0)


def test_logits_kernels_keep_their_step_twins_occupancy():
    """Every kLogits kernel (mode 9) exists for each kernel family the planner picks for kStep (mode 1), uses no scratch, and
    runs at the wavefronts per SIMD of its kStep twin (512 / VGPRs rounded up to 8, at most 8)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import LLVM, kernel_resources
    if not os.path.isfile(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf on this host")
    from jssenv_amd.build import build_extension
    rows = {n: (v, scratch) for n, v, _, vs, _, scratch in kernel_resources(build_extension())}
    occ = lambda v: min(8, 512 // ((v + 7) // 8 * 8))        # noqa: E731
    found = 0
    for fam in ("jss::jss_packed_kernel<16, {}, {}>", "jss::jss_packed_kernel<32, {}, {}>", "jss::jss_kernel<1, {}, {}>",
                "jss::jss_kernel<2, {}, {}>"):
        for tab in range(4):
            step, lg = fam.format(1, tab), fam.format(9, tab)
            assert lg in rows, lg
            assert rows[lg][1] == 0, f"{lg} uses scratch"
            assert occ(rows[lg][0]) == occ(rows[step][0]), f"{lg}: {occ(rows[lg][0])} waves per SIMD, {step}: {occ(rows[step][0])}"
            found += 1
    assert found == 16


# ---- host: the kernel source under the emulator (tiny sizes) ---------------------------------------------------------
@pytest.mark.parametrize("insts,order,steps", [("ta01", None, 30), ("ta41", None, 12), ("ragged", "by_shape", 10)])
def test_greedy_emu(emu, insts, order, steps):
    L.case_greedy(emu, L.ragged_by_shape() if insts == "ragged" else insts, batch=4, steps=steps, order=order)


@pytest.mark.parametrize("T", [1.0, 0.5])
def test_sampled_emu(emu, T):
    L.case_sampled(emu, "ta01", batch=8, steps=25, T=T)


def test_sampled_ragged_emu(emu):
    L.case_sampled(emu, L.ragged_by_shape(), batch=4, steps=10, T=1.0, order="by_shape")


def test_nope_and_padding_emu(emu):
    L.case_nope_and_padding(emu, steps=30)


@pytest.mark.parametrize("jobs,machines", [(16, 4), (32, 8), (64, 16), (128, 16)])
def test_nope_fold_emu(emu, jobs, machines):
    L.case_nope_fold(emu, jobs, machines, batch=8, steps=30)


def test_signed_zero_ties_emu(emu):
    L.case_signed_zero_ties(emu)


def test_broadcast_row_emu(emu):
    L.case_broadcast_row(emu, batch=4)


def test_determinism_emu(emu):
    L.case_determinism(emu, batch=4)


def test_autoreset_and_done_emu(emu):
    L.case_autoreset_and_done(emu, steps=30)


def test_bf16_and_stride_emu(emu):
    L.case_bf16_and_stride(emu, inst="ta01", batch=4, steps=3)


def test_bad_logits_emu(emu):
    L.case_bad_logits(emu, batch=4)


# ---- the MI355X --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("insts,order", [("ta01", None), ("ta41", None), ("ragged", "by_shape")])
def test_greedy_hip(hip, insts, order):
    L.case_greedy(hip, L.ragged_by_shape() if insts == "ragged" else insts, batch=8, steps=60, order=order)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1.0, 0.5])
@pytest.mark.parametrize("insts,order", [("ta01", None), ("ta41", None), ("ragged", "by_shape")])
def test_sampled_hip(hip, insts, order, T):
    L.case_sampled(hip, L.ragged_by_shape() if insts == "ragged" else insts, batch=64, steps=60, T=T, order=order)


@pytest.mark.gpu
def test_nope_and_padding_hip(hip):
    L.case_nope_and_padding(hip)


@pytest.mark.gpu
@pytest.mark.parametrize("jobs,machines", [(16, 4), (32, 8), (64, 16), (128, 16)])
def test_nope_fold_hip(hip, jobs, machines):
    L.case_nope_fold(hip, jobs, machines, batch=64, steps=60)


@pytest.mark.gpu
def test_signed_zero_ties_hip(hip):
    L.case_signed_zero_ties(hip)


@pytest.mark.gpu
def test_broadcast_row_hip(hip):
    L.case_broadcast_row(hip)


@pytest.mark.gpu
def test_determinism_hip(hip):
    L.case_determinism(hip)


@pytest.mark.gpu
def test_autoreset_and_done_hip(hip):
    L.case_autoreset_and_done(hip)


@pytest.mark.gpu
def test_bf16_and_stride_hip(hip):
    L.case_bf16_and_stride(hip)


@pytest.mark.gpu
def test_bad_logits_hip(hip):
    L.case_bad_logits(hip)


@pytest.mark.gpu
def test_full_size_headline_hip(hip):
    if hip.default_kernel != "auto":
        pytest.skip("full size: the default kernel choice only")
    L.case_full_size(hip, "ta01 x 65536", dict(instances="ta01", batch=65536))


@pytest.mark.gpu
def test_full_size_config5_by_shape_hip(hip):
    if hip.default_kernel != "auto":
        pytest.skip("full size: the default kernel choice only")
    from jssenv_amd import instances as I
    L.case_full_size(hip, "config 5 by shape x 32768",
                     dict(instances=[I.builtin_instance(f"ta{k:02d}") for k in range(1, 81)], batch=32768, order="by_shape"))


@pytest.mark.gpu
def test_distribution_hip(hip):
    L.case_distribution(hip, batch=65536)
