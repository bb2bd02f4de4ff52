"""Builds the native libraries of the package, in-tree:

* ``libjss_hip.so``  -- the MI355X kernels + C ABI (hipcc, gfx950 only);
* ``libjss_beam_hip.so`` -- beam search's selection kernel (include/jss_beam.h), a library of its own with the same flags;
* ``libjss_bound_hip.so`` -- the lower-bound kernel (include/jss_bound.h), a third HIP library built the same way;
* ``libjss_order_hip.so`` -- the machine-order kernels (include/jss_order.h), a fourth HIP library built the same way;
* ``libjss_tabu_hip.so`` -- the tabu-search kernel (include/jss_tabu.h), a fifth HIP library built the same way;
* ``libjss_block_hip.so`` -- the block-insertion tabu kernel (include/jss_block.h), a sixth HIP library built the same way;
* ``libjss_relink_hip.so`` -- the path-relinking kernel (include/jss_relink.h), a seventh HIP library built the same way;
* ``libjss_decode_hip.so`` -- the Giffler-Thompson decoder of key tables and the BRKGA generation kernels (include/jss_decode.h),
  an eighth HIP library built the same way;
* ``libjss_machine_hip.so`` -- the one-machine relaxation and shifting bottleneck kernels (include/jss_machine.h), a ninth HIP
  library built the same way;
* ``libjss_carlier_hip.so`` -- Carlier's one-machine search and the exact shifting bottleneck kernels (include/jss_carlier.h), a
  tenth HIP library built the same way;
* ``libjss_propagate_hip.so`` -- constraint propagation on operation windows (include/jss_propagate.h), an eleventh HIP library
  built the same way;
* ``libjss_onestep_hip.so`` -- the one-step rollout of the flagship class with write-through stores (include/jss_onestep.h), a
  twelfth HIP library built the same way;
* ``libjss_cpu.so``  -- the host-core twin with the identical C ABI (g++, OpenMP).
"""
import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
SRC = os.path.join(_HERE, "csrc", "jss_kernels.hip")
OUT = os.path.join(_HERE, "libjss_hip.so")
# (the counters are bumped by one lane per env: the compiler's wave-aggregation scaffolding around every atomic --
#  mbcnt, compare, exec save / restore, popcount, multiply -- is pure overhead there)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(_ROOT, "include"),
         "-mllvm", "-amdgpu-atomic-optimizer-strategy=None"]
CPU_SRC = os.path.join(_HERE, "csrc", "jss_cpu.cpp")
CPU_OUT = os.path.join(_HERE, "libjss_cpu.so")
CPU_FLAGS = ["-O3", "-std=c++17", "-fopenmp", "-fPIC", "-shared", "-Wall", "-I" + os.path.join(_ROOT, "include")]
_HEADER = os.path.join(_ROOT, "include", "jss_hip.h")
_SEARCH = os.path.join(_ROOT, "include", "jss_search.h")     # its companion: the search calls (jss_lookahead)
_RULES = os.path.join(_ROOT, "include", "jss_rules.h")       # ... and the caller-weighted rules (jss_rule_*)
_KEYS = os.path.join(_ROOT, "include", "jss_keys.h")         # ... and the per-operation priority keys (jss_key_*)
_BEAM = os.path.join(_ROOT, "include", "jss_beam.h")         # ... and beam search's selection (jss_beam_select)
BEAM_SRC = os.path.join(_HERE, "csrc", "jss_beam.hip")       # (libjss_beam_hip.so: its kernel stays out of libjss_hip.so)
BEAM_OUT = os.path.join(_HERE, "libjss_beam_hip.so")
_BOUND = os.path.join(_ROOT, "include", "jss_bound.h")       # ... and the makespan lower bounds (jss_bound)
BOUND_SRC = os.path.join(_HERE, "csrc", "jss_bound.hip")     # (libjss_bound_hip.so: a library of its own as well)
BOUND_OUT = os.path.join(_HERE, "libjss_bound_hip.so")
_ORDER = os.path.join(_ROOT, "include", "jss_order.h")       # ... and the evaluation of machine orders (jss_order_eval, jss_order_apply)
ORDER_SRC = os.path.join(_HERE, "csrc", "jss_order.hip")     # (libjss_order_hip.so: a library of its own as well)
ORDER_OUT = os.path.join(_HERE, "libjss_order_hip.so")
_TABU = os.path.join(_ROOT, "include", "jss_tabu.h")         # ... and tabu search over machine orders (jss_tabu_search)
TABU_SRC = os.path.join(_HERE, "csrc", "jss_tabu.hip")       # (libjss_tabu_hip.so: a library of its own as well)
TABU_OUT = os.path.join(_HERE, "libjss_tabu_hip.so")
_BLOCK = os.path.join(_ROOT, "include", "jss_block.h")       # ... and the tabu walk over block insertions (jss_block_search)
BLOCK_SRC = os.path.join(_HERE, "csrc", "jss_block.hip")     # (libjss_block_hip.so: a library of its own as well)
BLOCK_OUT = os.path.join(_HERE, "libjss_block_hip.so")
_RELINK = os.path.join(_ROOT, "include", "jss_relink.h")     # ... and path relinking between machine orders (jss_relink_walk)
RELINK_SRC = os.path.join(_HERE, "csrc", "jss_relink.hip")   # (libjss_relink_hip.so: a library of its own as well)
RELINK_OUT = os.path.join(_HERE, "libjss_relink_hip.so")
_DECODE = os.path.join(_ROOT, "include", "jss_decode.h")     # ... and Giffler-Thompson decoding of key tables, one BRKGA generation
DECODE_SRC = os.path.join(_HERE, "csrc", "jss_decode.hip")   # (libjss_decode_hip.so: a library of its own as well)
DECODE_OUT = os.path.join(_HERE, "libjss_decode_hip.so")
_MACHINE = os.path.join(_ROOT, "include", "jss_machine.h")   # ... and one-machine relaxations, the shifting bottleneck construction
MACHINE_SRC = os.path.join(_HERE, "csrc", "jss_machine.hip") # (libjss_machine_hip.so: a library of its own as well)
MACHINE_OUT = os.path.join(_HERE, "libjss_machine_hip.so")
_CARLIER = os.path.join(_ROOT, "include", "jss_carlier.h")   # ... and Carlier's one-machine search, exact shifting bottleneck builds
CARLIER_SRC = os.path.join(_HERE, "csrc", "jss_carlier.hip") # (libjss_carlier_hip.so: a library of its own as well)
CARLIER_OUT = os.path.join(_HERE, "libjss_carlier_hip.so")
_PROPAGATE = os.path.join(_ROOT, "include", "jss_propagate.h")   # ... and constraint propagation on operation windows (jss_propagate)
PROPAGATE_SRC = os.path.join(_HERE, "csrc", "jss_propagate.hip") # (libjss_propagate_hip.so: a library of its own as well)
PROPAGATE_OUT = os.path.join(_HERE, "libjss_propagate_hip.so")
_ONESTEP = os.path.join(_ROOT, "include", "jss_onestep.h")       # ... and the flagship class's one-step rollout (jss_onestep_*)
ONESTEP_SRC = os.path.join(_HERE, "csrc", "jss_onestep.hip")     # (libjss_onestep_hip.so: a library of its own as well)
ONESTEP_OUT = os.path.join(_HERE, "libjss_onestep_hip.so")
_OWN_LIBRARY = (os.path.basename(BEAM_SRC), os.path.basename(BOUND_SRC), os.path.basename(ORDER_SRC),
                os.path.basename(TABU_SRC), os.path.basename(BLOCK_SRC), os.path.basename(RELINK_SRC),
                os.path.basename(DECODE_SRC), os.path.basename(MACHINE_SRC), os.path.basename(CARLIER_SRC), os.path.basename(PROPAGATE_SRC),
                os.path.basename(ONESTEP_SRC))   # sources that libjss_hip.so does not include
_CHECKS = os.path.join(_HERE, "csrc", "jss_abi_checks.hpp")     # the argument checks both libraries share
_ROWS = os.path.join(_HERE, "csrc", "jss_env_rows.hpp")         # ... and the table of an env's rows


def hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.isfile(cand):
            return cand
    raise RuntimeError("hipcc not found")


def _fresh(out, deps):
    return os.path.isfile(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)


def build_extension(force: bool = False, extra=(), out: str = OUT) -> str:
    csrc = os.path.dirname(SRC)
    deps = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".hpp")) and f not in _OWN_LIBRARY] + [_HEADER, _SEARCH, _RULES, _KEYS, _BEAM, _BOUND, _ORDER, _TABU, _BLOCK, _RELINK, _DECODE, _MACHINE, _CARLIER, _PROPAGATE]
    if out == OUT:                     # the default output: the package's other HIP libraries go with it
        build_beam_extension(force)
        build_bound_extension(force)
        build_order_extension(force)
        build_tabu_extension(force)
        build_block_extension(force)
        build_relink_extension(force)
        build_decode_extension(force)
        build_machine_extension(force)
        build_carlier_extension(force)
        build_propagate_extension(force)
        build_onestep_extension(force)
    if not force and _fresh(out, deps):
        return out
    subprocess.check_call([hipcc(), *FLAGS, *extra, SRC, "-o", out])
    return out


def build_beam_extension(force: bool = False) -> str:
    if not force and _fresh(BEAM_OUT, [BEAM_SRC, _CHECKS, _HEADER, _SEARCH, _RULES, _KEYS, _BEAM, _BOUND, _ORDER, _TABU, _BLOCK, _RELINK, _DECODE, _MACHINE, _CARLIER, _PROPAGATE]):
        return BEAM_OUT
    tmp = BEAM_OUT + f".tmp{os.getpid()}"
    subprocess.check_call([hipcc(), *FLAGS, BEAM_SRC, "-o", tmp])
    os.replace(tmp, BEAM_OUT)
    return BEAM_OUT


def build_bound_extension(force: bool = False) -> str:
    if not force and _fresh(BOUND_OUT, [BOUND_SRC, _CHECKS, _HEADER, _SEARCH, _RULES, _KEYS, _BEAM, _BOUND, _ORDER, _TABU, _BLOCK, _RELINK, _DECODE, _MACHINE, _CARLIER, _PROPAGATE]):
        return BOUND_OUT
    tmp = BOUND_OUT + f".tmp{os.getpid()}"
    subprocess.check_call([hipcc(), *FLAGS, BOUND_SRC, "-o", tmp])
    os.replace(tmp, BOUND_OUT)
    return BOUND_OUT


def build_order_extension(force: bool = False) -> str:
    if not force and _fresh(ORDER_OUT, [ORDER_SRC, _CHECKS, _HEADER, _SEARCH, _RULES, _KEYS, _BEAM, _BOUND, _ORDER, _TABU, _BLOCK, _RELINK, _DECODE, _MACHINE, _CARLIER, _PROPAGATE]):
        return ORDER_OUT
    tmp = ORDER_OUT + f".tmp{os.getpid()}"
    subprocess.check_call([hipcc(), *FLAGS, ORDER_SRC, "-o", tmp])
    os.replace(tmp, ORDER_OUT)
    return ORDER_OUT


def build_tabu_extension(force: bool = False) -> str:
    if not force and _fresh(TABU_OUT, [TABU_SRC, _CHECKS, _HEADER, _SEARCH, _RULES, _KEYS, _BEAM, _BOUND, _ORDER, _TABU, _BLOCK, _RELINK, _DECODE, _MACHINE, _CARLIER, _PROPAGATE]):
        return TABU_OUT
    tmp = TABU_OUT + f".tmp{os.getpid()}"
    subprocess.check_call([hipcc(), *FLAGS, TABU_SRC, "-o", tmp])
    os.replace(tmp, TABU_OUT)
    return TABU_OUT


def build_block_extension(force: bool = False) -> str:
    if not force and _fresh(BLOCK_OUT, [BLOCK_SRC, _CHECKS, _HEADER, _SEARCH, _RULES, _KEYS, _BEAM, _BOUND, _ORDER, _TABU, _BLOCK, _RELINK, _DECODE, _MACHINE, _CARLIER, _PROPAGATE]):
        return BLOCK_OUT
    tmp = BLOCK_OUT + f".tmp{os.getpid()}"
    subprocess.check_call([hipcc(), *FLAGS, BLOCK_SRC, "-o", tmp])
    os.replace(tmp, BLOCK_OUT)
    return BLOCK_OUT


def build_relink_extension(force: bool = False) -> str:
    if not force and _fresh(RELINK_OUT, [RELINK_SRC, _CHECKS, _HEADER, _SEARCH, _RULES, _KEYS, _BEAM, _BOUND, _ORDER, _TABU, _BLOCK, _RELINK, _DECODE, _MACHINE, _CARLIER, _PROPAGATE]):
        return RELINK_OUT
    tmp = RELINK_OUT + f".tmp{os.getpid()}"
    subprocess.check_call([hipcc(), *FLAGS, RELINK_SRC, "-o", tmp])
    os.replace(tmp, RELINK_OUT)
    return RELINK_OUT


def build_decode_extension(force: bool = False) -> str:
    if not force and _fresh(DECODE_OUT, [DECODE_SRC, _CHECKS, _HEADER, _SEARCH, _RULES, _KEYS, _BEAM, _BOUND, _ORDER, _TABU, _BLOCK, _RELINK, _DECODE, _MACHINE, _CARLIER, _PROPAGATE]):
        return DECODE_OUT
    tmp = DECODE_OUT + f".tmp{os.getpid()}"
    subprocess.check_call([hipcc(), *FLAGS, DECODE_SRC, "-o", tmp])
    os.replace(tmp, DECODE_OUT)
    return DECODE_OUT


def build_machine_extension(force: bool = False) -> str:
    if not force and _fresh(MACHINE_OUT, [MACHINE_SRC, _CHECKS, _HEADER, _SEARCH, _RULES, _KEYS, _BEAM, _BOUND, _ORDER, _TABU, _BLOCK, _RELINK, _DECODE, _MACHINE, _CARLIER, _PROPAGATE]):
        return MACHINE_OUT
    tmp = MACHINE_OUT + f".tmp{os.getpid()}"
    subprocess.check_call([hipcc(), *FLAGS, MACHINE_SRC, "-o", tmp])
    os.replace(tmp, MACHINE_OUT)
    return MACHINE_OUT


def build_carlier_extension(force: bool = False) -> str:
    if not force and _fresh(CARLIER_OUT, [CARLIER_SRC, _CHECKS, _HEADER, _SEARCH, _RULES, _KEYS, _BEAM, _BOUND, _ORDER, _TABU, _BLOCK, _RELINK, _DECODE, _MACHINE, _CARLIER, _PROPAGATE]):
        return CARLIER_OUT
    tmp = CARLIER_OUT + f".tmp{os.getpid()}"
    subprocess.check_call([hipcc(), *FLAGS, CARLIER_SRC, "-o", tmp])
    os.replace(tmp, CARLIER_OUT)
    return CARLIER_OUT


def build_propagate_extension(force: bool = False) -> str:
    if not force and _fresh(PROPAGATE_OUT, [PROPAGATE_SRC, _CHECKS, _HEADER, _SEARCH, _RULES, _KEYS, _BEAM, _BOUND, _ORDER, _TABU, _BLOCK, _RELINK, _DECODE, _MACHINE, _CARLIER, _PROPAGATE]):
        return PROPAGATE_OUT
    tmp = PROPAGATE_OUT + f".tmp{os.getpid()}"
    subprocess.check_call([hipcc(), *FLAGS, PROPAGATE_SRC, "-o", tmp])
    os.replace(tmp, PROPAGATE_OUT)
    return PROPAGATE_OUT


def build_onestep_extension(force: bool = False, extra=(), out: str = ONESTEP_OUT) -> str:
    csrc = os.path.dirname(ONESTEP_SRC)
    deps = [ONESTEP_SRC, _CHECKS, _ROWS, _ONESTEP, _HEADER, _SEARCH, _RULES, _KEYS] + \
           [os.path.join(csrc, f) for f in ("jss_common.hpp", "jss_packed_env.hpp")]
    if not force and _fresh(out, deps):
        return out
    tmp = out + f".tmp{os.getpid()}"
    subprocess.check_call([hipcc(), *FLAGS, *extra, ONESTEP_SRC, "-o", tmp])
    os.replace(tmp, out)
    return out


def build_cpu_twin(force: bool = False) -> str:
    if not force and _fresh(CPU_OUT, [CPU_SRC, _CHECKS, _ROWS, _HEADER, _SEARCH, _RULES, _KEYS, _BEAM, _BOUND, _ORDER, _TABU, _BLOCK, _RELINK, _DECODE, _MACHINE, _CARLIER, _PROPAGATE]):
        return CPU_OUT
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        raise RuntimeError("g++ not found")
    tmp = CPU_OUT + f".tmp{os.getpid()}"
    subprocess.check_call([cxx, *CPU_FLAGS, CPU_SRC, "-o", tmp])
    os.replace(tmp, CPU_OUT)     # atomic: several processes (ranks, xdist workers) may build at once
    return CPU_OUT
