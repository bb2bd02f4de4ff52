"""Every kernel instantiation of the library against the oracle, not just the ones the feature tests happen to reach:
tests/kernel_matrix_cases.py generates one recipe per (flavour, mode, table layout) cell -- the BatchedJssEnv arguments that
make the dispatch of jss_kernels.hip choose that kernel, and the call that runs the mode.

(a) under the emulator, with its launch log on: the log shows the kernel the recipe names, and every env equals the oracle;
(b) the kernels of the built library are exactly those the recipes reach, those with modules of their own, UNREACHABLE, and
    the one kernel that cannot run under the emulator (NOT_UNDER_THE_EMULATOR);
(c) the same recipes on the MI355X (-m gpu);  (d) the same recipes on the host-core twin.
Recorded tallies and times: profiles/r13_kernel_matrix/."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [HERE, os.path.join(HERE, "emu"), os.path.join(ROOT, "tools"), ROOT]

import kernel_matrix_cases as M  # noqa: E402

RECIPES = M.recipes()

# Kernels that no argument list can make the dispatch choose, each with the line of jss_kernels.hip that rules it out.
UNREACHABLE = {}

# Kernels outside the flavour x mode x layout matrix, held to the oracle by modules of their own: the module named here must
# show launches of the kernel in profiles/r13_kernel_matrix/coverage_before.txt (tools/kernel_coverage.py).  That file is a
# recorded tally, not a live measurement: if a later change to one of these modules stops launching its kernel, this test
# does not notice -- run tools/kernel_coverage.py again to see it.
OWN_MODULES = {
    "jss_multi_kernel<0>": "kernel_emu", "jss_multi_kernel<1>": "kernel_emu", "jss_multi_kernel<3>": "kernel_emu",
    "jss_multi_kernel<5>": "kernel_emu", "jss_multi_kernel<9>": "multi_step_logits",
    "jss_clone_kernel": "clone", "jss_generate_kernel": "generate",
}

# jss_session_step_kernel posts one step and waits for the resident kernel to answer, in one launch.  The emulator runs a
# launch to completion, so under it nothing ever answers, and no non-GPU module launches it (coverage_before.txt and
# coverage_after.txt: 0).  It is reachable, so it is no entry of UNREACHABLE: the one kernel of the library that only the
# GPU run (c) launches, in every session recipe, through StepSession.step().  (The twin (d) takes the same call, but it is
# host code: it runs no kernel.)
NOT_UNDER_THE_EMULATOR = {"jss_session_step_kernel"}


def run_logged(recipe_ids, log):
    """Runs recipes under the emulator in a process of its own (the launch log is opened once per process); returns the
    launched kernels per recipe."""
    env = dict(os.environ, JSS_EMU_LAUNCH_LOG=log)
    env.pop("JSS_EMU_LAUNCH_DRY", None)
    subprocess.check_call([sys.executable, os.path.abspath(__file__), log] + list(recipe_ids), env=env)
    launched, name = {}, None
    with open(log) as f:
        lines = f.readlines()
    outer = os.environ.get("JSS_EMU_LAUNCH_LOG")          # (a tally of the whole suite, tools/kernel_coverage.py: hand the lines on)
    if outer and outer != log:
        with open(outer, "a") as f:
            f.writelines(lines)
    for line in lines:
        if line.startswith("# "):
            name = line[2:].strip()
            launched[name] = set()
        elif line.startswith("launch "):
            launched[name].add(M.short_name(line[len("launch "):].rsplit(" grid=", 1)[0]))
    return launched


def main(log, recipe_ids):
    from emu_backend import EmuBackend
    be = EmuBackend()
    fd = os.open(log, os.O_WRONLY | os.O_APPEND | os.O_CREAT)
    for r in RECIPES:
        if r.id in recipe_ids:
            os.write(fd, f"# {r.id}\n".encode())
            M.run_recipe(r, be, emulator=True)
    os.close(fd)


@pytest.mark.parametrize("flavour", list(M.FLAVOURS))
def test_recipes_reach_their_kernels_and_equal_the_oracle_emulator(flavour, tmp_path):
    mine = [r for r in RECIPES if r.flavour == flavour]
    launched = run_logged([r.id for r in mine], str(tmp_path / "launch_log.txt"))
    for r in mine:
        for kernel in (r.kernel,) + r.also:
            assert kernel in launched[r.id], f"{r.id} claims {kernel}, the emulator launched {sorted(launched[r.id])}"


def test_every_kernel_of_the_library_has_a_recipe():
    from emu_backend import build as build_emu
    kernels = set(M.library_kernels(build_emu()))
    assert len(kernels) >= 190, f"{len(kernels)} kernels: profiles/r12_launcher/kernel_resources.txt lists 190"
    from kernel_resources import LLVM
    if os.path.isfile(os.path.join(LLVM, "llvm-readelf")):              # ... and the gfx950 code object holds the same ones
        from jssenv_amd.build import build_extension
        assert set(M.code_object_kernels(build_extension())) == kernels
    reached = {k for r in RECIPES for k in (r.kernel,) + r.also}
    assert len({r.kernel for r in RECIPES}) == len(RECIPES) and len({r.id for r in RECIPES}) == len(RECIPES)
    assert reached <= kernels, f"recipes name kernels the library does not have: {sorted(reached - kernels)}"
    assert not set(UNREACHABLE) & reached and not set(OWN_MODULES) & reached
    assert NOT_UNDER_THE_EMULATOR <= kernels and not NOT_UNDER_THE_EMULATOR & (reached | set(OWN_MODULES))
    rest = kernels - reached - set(OWN_MODULES) - NOT_UNDER_THE_EMULATOR
    assert rest == set(UNREACHABLE), f"kernels without a recipe: {sorted(rest - set(UNREACHABLE))}"
    tally = {}
    with open(os.path.join(ROOT, "profiles", "r13_kernel_matrix", "coverage_before.txt")) as f:
        for line in f:
            if not line.startswith("#"):
                count, name = line.split(None, 1)
                name, _, modules = name.strip().partition("   (")
                tally[name] = (int(count), modules.rstrip(")").split(", "))
    for kernel, module in OWN_MODULES.items():
        assert kernel in kernels and tally[kernel][0] > 0 and module in tally[kernel][1], f"{kernel}: not launched by test_{module}"


@pytest.fixture(scope="module")
def cpu():
    from jssenv_amd.env import CpuBackend
    return CpuBackend()


@pytest.mark.parametrize("recipe", RECIPES, ids=[r.id for r in RECIPES])
def test_recipes_equal_the_oracle_twin(cpu, recipe):
    M.run_recipe(recipe, cpu)


@pytest.fixture(scope="module")
def hip():
    from jssenv_amd.env import HipBackend
    be = HipBackend("cuda:0")
    assert be.name == "hip" and be.lib.jss_backend() == b"hip:gfx950"
    return be


@pytest.mark.gpu
@pytest.mark.parametrize("recipe", RECIPES, ids=[r.id for r in RECIPES])
def test_recipes_equal_the_oracle_gpu(hip, recipe):
    M.run_recipe(recipe, hip)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
