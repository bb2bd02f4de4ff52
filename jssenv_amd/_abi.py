"""ctypes mirror of include/jss_hip.h (structs, constants, prototypes).

Pure declarations: no torch, no device access.  ``bind(lib)`` attaches the
prototypes to a loaded ``libjss_hip.so`` (or its host-core twin ``libjss_cpu.so``:
identical symbols) and fails loudly if a symbol the header declares is missing.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

ABI_VERSION = 14
STATE_LAYOUT = 7     # version of the state tensors' layout (checkpoints): unchanged since ABI v7
MAX_JOBS, MAX_MACHINES = 128, 64
F_TODO, F_CUR, F_LEFT, F_PERF, F_IDLE, F_IDLE_LAST, F_F4, F_NEXT, NF = 0, 1, 2, 3, 4, 5, 6, 7, 8
TODO_MASK, FLAG_LEGAL, FLAG_BLOCKED, NEXT2_SHIFT = 255, 256, 512, 10
# compact 16-byte record of shared-instance batches (JSS_FC_*): no cached ops, packed words
FC_W0, FC_LEFT_F4, FC_IDLE, FC_IDLE_LAST, NFC = 0, 1, 2, 3, 4
FC_TODO_MASK, FC_FLAG_LEGAL, FC_FLAG_BLOCKED, FC_FLAG_F4_ONE, FC_PERF_SHIFT = 127, 128, 256, 512, 10
# medium 24-byte record of per-env-instance batches with jobs, machines <= 32 (JSS_FM_*): three 21-bit cached ops, no machine clocks
FM_W0, FM_LEFT_F4, FM_PERF_NEXT, FM_NEXT_NEXT2, FM_IDLE, FM_IDLE_LAST, NFM = 0, 1, 2, 3, 4, 5, 6
FM_TODO_MASK, FM_FLAG_LEGAL, FM_FLAG_BLOCKED, FM_FLAG_F4_ONE, FM_CUR_SHIFT, FM_OP_MASK = 63, 64, 128, 256, 9, 0x1FFFFF
H_CLOCK, H_EPISODE, H_STEP, H_STATUS = 0, 1, 2, 3
NH = 4
C_JOBS, C_MACHINES, C_MAX_TIME_OP, C_TABLE, C_MAX_TIME_JOBS, C_SUM_OP = 0, 1, 2, 3, 4, 5
C_RCP_MAX_TIME_OP, C_RCP_MAX_TIME_JOBS, C_RCP_SUM_OP, C_RCP_MACHINES, NC = 6, 7, 8, 9, 12
STATUS_NOOP = 256
F4_ONE = -1
I_JOBS, I_MACHINES, I_MAX_TIME_OP, I_MAX_TIME_JOBS, I_SUM_OP = 0, 1, 2, 3, 4
I_RCP_MAX_TIME_OP, I_RCP_MAX_TIME_JOBS, I_RCP_SUM_OP, I_RCP_MACHINES, NI = 5, 6, 7, 8, 12
ERR_ILLEGAL_ACTION, ERR_NOPE_IDLE, ERR_BAD_ACTION, ERR_BAD_LOGITS, ERR_BAD_INDEX = 1, 2, 4, 8, 16
ACTION_SKIP, ACTION_RESET, ACTION_CLOSE = -1, -2, -3
POLICY = {"random": 0, "FIFO": 1, "SPT": 2, "MWR": 3, "LWR": 4, "MOR": 5, "LOR": 6, "CR": 7}
ROLLOUT_AUTORESET, ROLLOUT_FORK_JOIN = 1, 2
# jss_step_logits (JssLogits.dtype; K_LOGITS keys its Gumbel noise: rng_u32(seed ^ LOGITS_SEED_XOR, ...))
LOGITS_F32, LOGITS_BF16 = 0, 1
LOGITS_SEED_XOR = 0x2545F4914F6CDD1D
# jss_generate (JssGen): derived instance seeds are 1 + rng_u32(seed ^ GEN_SEED_XOR, env_id, episode, 0 | 1) % GEN_SEED_MOD
GEN_SEED_XOR = 0xD1B54A32D192ED03
LCG_M = 2147483647                   # the Taillard streams' modulus; seeds lie in [1, LCG_M - 1]
GEN_SEED_MOD = LCG_M - 1


def cr_kind(due_date_factor: float = 1.5):
    """The `kind` code of CriticalRatio with a due-date factor other than the default (JSS_POLICY_CR_FACTOR): factor = p / q
    with q a power of two <= 64 and p <= 255, or None when the factor has no such form (the host loop serves it then)."""
    from fractions import Fraction
    f = Fraction(due_date_factor).limit_denominator(64)
    if float(f) != float(due_date_factor) or f <= 0 or f.numerator > 255 or f.denominator & (f.denominator - 1):
        return None
    if (f.numerator, f.denominator) == (3, 2):
        return POLICY["CR"]
    return POLICY["CR"] | (f.numerator << 8) | (f.denominator << 16)


POLICY_CR_F64 = POLICY["CR"] | (1 << 24)    # JSS_POLICY_CR_F64: the factor travels as the double JssDesc.cr_factor


def policy_code(kind):
    """str | int -> the int the C ABI takes."""
    return POLICY[kind] if isinstance(kind, str) else int(kind)
# JssDesc.kernel: "wave" forces one wavefront per env; the "...-1env" forms add JSS_KERNEL_ONE_ENV_PER_WAVE (a wavefront of the
# one-step launches never serves two envs in turn: A/B runs, tests)
# ("...-2env": JSS_KERNEL_TWO_ENVS_PER_WAVE, they always do -- tests on small batches)
KERNEL = {"auto": 0, "wave": 1, "auto-1env": 2, "wave-1env": 3, "auto-2env": 4, "wave-2env": 5}
E_NULL, E_SHAPE, E_KIND, E_LDS, E_RESIDENT, E_SESSION = -1, -2, -3, -4, -5, -6
MAX_SUB_BATCHES = 16

SYMBOLS = ("jss_abi_version", "jss_error_string", "jss_backend", "jss_reset", "jss_step", "jss_advance", "jss_policy",
           "jss_rollout", "jss_rollout_steps", "jss_rollout_steps_multi", "jss_trajectory", "jss_sync_check",
           "jss_step_autoreset", "jss_policy_step_steps", "jss_steps", "jss_session_open", "jss_session_post", "jss_session_wait", "jss_session_step", "jss_session_close",
           "jss_multi_reset", "jss_multi_step", "jss_multi_policy", "jss_multi_rollout", "jss_step_logits",
           "jss_multi_step_logits", "jss_generate", "jss_clone")

# include/jss_search.h: the companion header of the search calls (its own version; ABI_VERSION and SYMBOLS do not move)
SEARCH_VERSION = 1
SEARCH_SYMBOLS = ("jss_lookahead",)

# include/jss_rules.h: the companion header of the caller-weighted rules (its own version again).  The weighted selector has no
# POLICY code: it is reached through these symbols only.
RULES_VERSION = 1
RULES_SYMBOLS = ("jss_rule_policy", "jss_rule_rollout", "jss_rule_lookahead")
RW_DUR, RW_NEXT, RW_REM, RW_TOTAL, RW_OPS, RW_WAIT, RW_IDLE, RW_NOPE, RW_N = 0, 1, 2, 3, 4, 5, 6, 7, 8
RW_NEVER_NOPE = -2**31

# include/jss_keys.h: the companion header of the per-operation priority keys (its own version).  The key selector has no POLICY
# code either: it is reached through these symbols only.
KEYS_VERSION = 1
KEYS_SYMBOLS = ("jss_key_policy", "jss_key_rollout", "jss_key_lookahead")
KEY_NEVER_NOPE = -2**31            # JssKeys.nope_key that exceeds no key: NOPE only when no job is legal

# include/jss_beam.h: the companion header of beam search's candidate selection (its own version).  The HIP library exports it
# from a library of its own, libjss_beam_hip.so; the twin from libjss_cpu.so.
BEAM_VERSION = 1
BEAM_SYMBOLS = ("jss_beam_select",)
BEAM_DEDUPE = 1

# include/jss_bound.h: the companion header of the makespan lower bounds (its own version).  The HIP library exports it from a
# third library, libjss_bound_hip.so; the twin from libjss_cpu.so.
BOUND_VERSION = 1
BOUND_SYMBOLS = ("jss_bound",)

# include/jss_order.h: the companion header of the evaluation of machine orders (its own version).  The HIP library exports it
# from a fourth library, libjss_order_hip.so; the twin from libjss_cpu.so.
ORDER_VERSION = 1
ORDER_SYMBOLS = ("jss_order_eval", "jss_order_apply")

# include/jss_tabu.h: the companion header of tabu search over machine orders (its own version).  The HIP library exports it
# from a fifth library, libjss_tabu_hip.so; the twin from libjss_cpu.so.
TABU_VERSION = 1
TABU_SYMBOLS = ("jss_tabu_search",)
TABU_NI = 4                       # info row: stop, moves, best_move, evaluations
TABU_MAX_ITERS, TABU_MAX_TENURE = 65536, 64

# include/jss_block.h: the companion header of the block-insertion tabu walk (its own version).  The HIP library exports it from
# a sixth library, libjss_block_hip.so; the twin from libjss_cpu.so.  iters, tenure and target range as in jss_tabu.h.
BLOCK_VERSION = 1
BLOCK_SYMBOLS = ("jss_block_search",)
BLOCK_NI = 8                      # info row: stop, moves, best_move, evaluations, screened, far, hits, 0
BLOCK_MAX_REACH = 65535

# include/jss_relink.h: the companion header of path relinking between machine orders (its own version).  The HIP library exports
# it from a seventh library, libjss_relink_hip.so; the twin from libjss_cpu.so.
RELINK_VERSION = 1
RELINK_SYMBOLS = ("jss_relink_walk",)
RELINK_NI = 8                     # info row: stop, moves, best_move, dist0, dist, candidates, fallbacks, retries
RELINK_MAX_STEPS = 65536

# include/jss_decode.h: the companion header of Giffler-Thompson decoding of key tables and of one BRKGA generation (its own
# version).  The HIP library exports both from an eighth library, libjss_decode_hip.so; the twin from libjss_cpu.so.
DECODE_VERSION = 1
DECODE_SYMBOLS = ("jss_decode_keys", "jss_keys_evolve")
DECODE_NI = 4                     # info row: conflicts, widest, delayed, 0
EVOLVE_SEED_XOR = 0xD1B54A32D192ED03   # keys jss_keys_evolve's counter RNG: rng_u32(seed ^ EVOLVE_SEED_XOR, row, generation, x)
EVOLVE_MAX_POP = 4096

# include/jss_machine.h: the companion header of the one-machine relaxations of partial selections and of the shifting bottleneck
# construction (its own version).  The HIP library exports both from a ninth library, libjss_machine_hip.so; the twin from
# libjss_cpu.so.
MACHINE_VERSION = 1
MACHINE_SYMBOLS = ("jss_machine_relax", "jss_bottleneck_build")
BOTTLENECK_NI = 4                 # info row: machines fixed, re-sequencings tried, re-sequencings that shortened, first bound
BOTTLENECK_MAX_REOPT = 8

# include/jss_carlier.h: the companion header of Carlier's one-machine search and of the shifting bottleneck construction that
# sequences its machines with it (its own version).  The HIP library exports both from a tenth library, libjss_carlier_hip.so;
# the twin from libjss_cpu.so.
CARLIER_VERSION = 1
CARLIER_SYMBOLS = ("jss_machine_solve", "jss_bottleneck_exact")
CARLIER_MAX_NODES = 4096
CARLIER_MAX_DEPTH = 64
EXACT_NI = 8                      # info row: BOTTLENECK_NI's, then nodes in total, most nodes of one problem, problems left open, sequences replaced by Schrage's

# include/jss_propagate.h: the companion header of constraint propagation on operation windows (its own version).  The HIP library
# exports it from an eleventh library, libjss_propagate_hip.so; the twin from libjss_cpu.so.
PROPAGATE_VERSION = 1
PROPAGATE_SYMBOLS = ("jss_propagate",)
PROPAGATE_MAX_PASSES = 4096
PROPAGATE_MAX_TIME = 0x3FFFFFFF
PROPAGATE_FIXPOINT, PROPAGATE_REFUTED, PROPAGATE_BUDGET = 0, 1, 2

# include/jss_onestep.h: the one-step rollout of the flagship class (its own version).  The HIP library exports it from a twelfth
# library, libjss_onestep_hip.so; the twin has no counterpart (jss_rollout / jss_rollout_steps are the form on the host).
ONESTEP_VERSION = 1
ONESTEP_SYMBOLS = ("jss_onestep_version", "jss_onestep_rollout", "jss_onestep_rollout_steps")
ONESTEP_MAX_GROUP = 32            # jmax, mmax of the class: a 16- or 32-lane group per env

_p = C.c_void_p


class JssDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("jmax", C.c_int32), ("mmax", C.c_int32), ("n_tables", C.c_int32),
                ("ops", _p), ("rem", _p), ("inst", _p), ("table_of_env", _p), ("env_ids", _p),
                ("env_id_base", C.c_int64), ("kernel", C.c_int32), ("threads", C.c_int32),
                ("jmin", C.c_int32), ("record_ints", C.c_int32), ("cr_factor", C.c_double),
                ("jclass", C.c_int32), ("mclass", C.c_int32)]


class JssState(C.Structure):
    _fields_ = [("env", _p), ("env_const", _p), ("job", _p), ("machine", _p), ("solution", _p), ("counters", _p)]


class JssOut(C.Structure):
    _fields_ = [("real_obs", _p), ("action_mask", _p), ("reward", _p), ("done", _p), ("makespan", _p)]


class JssTraj(C.Structure):
    _fields_ = [("real_obs", _p), ("action_mask", _p), ("action", _p), ("reward", _p), ("done", _p),
                ("stride", C.c_int64)]       # envs between two steps' slots (0 = the call's batch): a range of a larger batch


class JssSession(C.Structure):
    _fields_ = [("mail", _p), ("progress", _p), ("status", _p), ("depth", C.c_int32), ("timeout_ms", C.c_int32),
                ("slots", C.c_int32), ("reserved", C.c_int32)]


class JssLogits(C.Structure):
    _fields_ = [("logits", _p), ("row", C.c_int64), ("dtype", C.c_int32), ("temperature", C.c_float),
                ("action", _p), ("logp", _p), ("entropy", _p)]


class JssGen(C.Structure):
    _fields_ = [("ops", _p), ("rem", _p), ("inst", _p), ("time_seed", _p), ("machine_seed", _p), ("actions", _p),
                ("seed", C.c_uint64), ("jobs", C.c_int32), ("machines", C.c_int32), ("dur_low", C.c_int32),
                ("dur_high", C.c_int32)]


class JssCloneDst(C.Structure):
    _fields_ = [("table_of_env", _p), ("ops", _p), ("rem", _p), ("inst", _p)]


class JssLookahead(C.Structure):     # include/jss_search.h
    _fields_ = [("n", C.c_int32), ("parent", _p), ("action", _p), ("id_base", C.c_int64), ("makespan", _p), ("steps", _p),
                ("reward_num", _p)]


class JssRule(C.Structure):          # include/jss_rules.h
    _fields_ = [("weights", _p), ("stride", C.c_int32)]


class JssKeys(C.Structure):          # include/jss_keys.h
    _fields_ = [("keys", _p), ("stride", C.c_int32), ("nope_key", C.c_int32)]


class JssBeam(C.Structure):          # include/jss_beam.h
    _fields_ = [("n_groups", C.c_int32), ("width", C.c_int32), ("n_actions", C.c_int32), ("flags", C.c_uint32),
                ("cand_parent", _p), ("makespan", _p), ("steps", _p), ("reward_num", _p), ("done", _p), ("env_makespan", _p),
                ("src", _p), ("action", _p), ("score", _p), ("next_parent", _p), ("counts", _p)]


class JssBound(C.Structure):         # include/jss_bound.h
    _fields_ = [("n", C.c_int32), ("parent", _p), ("action", _p), ("mask", _p), ("lower_bound", _p), ("job_bound", _p),
                ("est_start", _p)]


class JssOrder(C.Structure):         # include/jss_order.h
    _fields_ = [("n", C.c_int32), ("pair_cap", C.c_int32), ("rank", _p), ("parent", _p), ("swap_a", _p), ("swap_b", _p),
                ("makespan", _p), ("start", _p), ("tail", _p), ("pair_a", _p), ("pair_b", _p), ("n_pairs", _p)]


class JssOrderApply(C.Structure):    # include/jss_order.h
    _fields_ = [("batch", C.c_int32), ("jmax", C.c_int32), ("mmax", C.c_int32), ("pair_cap", C.c_int32), ("rank", _p), ("cur", _p),
                ("makespan", _p), ("pair_a", _p), ("pair_b", _p), ("improved", _p)]


class JssTabu(C.Structure):          # include/jss_tabu.h
    _fields_ = [("iters", C.c_int32), ("tenure", C.c_int32), ("rank", _p), ("tenure_of", _p), ("target", _p),
                ("best_makespan", _p), ("best_rank", _p), ("last_rank", _p), ("info", _p), ("trace", _p)]


class JssBlock(C.Structure):         # include/jss_block.h
    _fields_ = [("iters", C.c_int32), ("tenure", C.c_int32), ("reach", C.c_int32), ("rank", _p), ("tenure_of", _p), ("target", _p),
                ("best_makespan", _p), ("best_rank", _p), ("last_rank", _p), ("info", _p), ("trace", _p), ("move_log", _p)]


class JssRelink(C.Structure):        # include/jss_relink.h
    _fields_ = [("steps", C.c_int32), ("until", C.c_int32), ("margin", C.c_int32), ("rank", _p), ("guide", _p), ("until_of", _p),
                ("best_makespan", _p), ("best_rank", _p), ("last_makespan", _p), ("last_rank", _p), ("info", _p), ("trace", _p),
                ("move_log", _p)]


class JssDecode(C.Structure):        # include/jss_decode.h
    _fields_ = [("n", C.c_int32), ("stride", C.c_int32), ("delta_q16", C.c_int32), ("parents", _p), ("keys", _p), ("delta_of", _p),
                ("makespan", _p), ("start", _p), ("info", _p)]


class JssEvolve(C.Structure):        # include/jss_decode.h
    _fields_ = [("groups", C.c_int32), ("pop", C.c_int32), ("region", C.c_int32), ("n_elite", C.c_int32), ("n_mutant", C.c_int32),
                ("rho_q16", C.c_int32), ("generation", C.c_int32), ("seed", C.c_uint64), ("fitness", _p), ("keys_in", _p),
                ("keys_out", _p), ("by_rank", _p)]


class JssMachineRelax(C.Structure):  # include/jss_machine.h
    _fields_ = [("n", C.c_int32), ("stride", C.c_int32), ("parents", _p), ("rank", _p), ("fixed", _p), ("length", _p),
                ("lower_bound", _p), ("bottleneck", _p), ("jps", _p), ("schrage", _p), ("head", _p), ("tail", _p), ("rank_out", _p)]


class JssBottleneck(C.Structure):    # include/jss_machine.h
    _fields_ = [("n", C.c_int32), ("reopt", C.c_int32), ("parents", _p), ("rank_in", _p), ("fixed_in", _p), ("bias", _p),
                ("makespan", _p), ("rank", _p), ("info", _p), ("order", _p)]


class JssMachineSolve(C.Structure):  # include/jss_carlier.h
    _fields_ = [("n", C.c_int32), ("stride", C.c_int32), ("nodes", C.c_int32), ("reserved", C.c_int32), ("parents", _p), ("rank", _p),
                ("fixed", _p), ("length", _p), ("lower_bound", _p), ("bottleneck", _p), ("opt", _p), ("low", _p), ("nodes_used", _p),
                ("proved", _p), ("head", _p), ("tail", _p), ("rank_out", _p)]


class JssBottleneckExact(C.Structure):   # include/jss_carlier.h
    _fields_ = [("n", C.c_int32), ("reopt", C.c_int32), ("nodes", C.c_int32), ("reserved", C.c_int32), ("parents", _p), ("rank_in", _p),
                ("fixed_in", _p), ("bias", _p), ("makespan", _p), ("rank", _p), ("info", _p), ("order", _p)]


class JssPropagate(C.Structure):     # include/jss_propagate.h
    _fields_ = [("n", C.c_int32), ("stride", C.c_int32), ("win_stride", C.c_int32), ("passes", C.c_int32), ("parents", _p), ("rank", _p),
                ("fixed", _p), ("ub", _p), ("est_in", _p), ("lct_in", _p), ("hyp_op", _p), ("hyp_est", _p), ("hyp_lct", _p),
                ("status", _p), ("passes_used", _p), ("est", _p), ("lct", _p)]


def library_path(name: str = "libjss_hip.so") -> str:
    """In-tree library; JSSENV_AMD_LIB points development builds at another build of the same ABI."""
    if name == "libjss_hip.so" and os.environ.get("JSSENV_AMD_LIB"):
        return os.environ["JSSENV_AMD_LIB"]
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), name)


def bind(lib):
    """Attach prototypes; raises AttributeError naming the first missing symbol."""
    for name in SYMBOLS:
        if not hasattr(lib, name):
            raise AttributeError(f"library does not export {name}")
    D, S, O = C.POINTER(JssDesc), C.POINTER(JssState), C.POINTER(JssOut)
    lib.jss_abi_version.restype, lib.jss_abi_version.argtypes = C.c_int, []
    lib.jss_error_string.restype, lib.jss_error_string.argtypes = C.c_char_p, [C.c_int]
    lib.jss_backend.restype, lib.jss_backend.argtypes = C.c_char_p, []
    lib.jss_reset.restype, lib.jss_reset.argtypes = C.c_int, [D, S, O, _p, _p]
    lib.jss_step.restype, lib.jss_step.argtypes = C.c_int, [D, S, _p, O, _p]
    lib.jss_step_autoreset.restype, lib.jss_step_autoreset.argtypes = C.c_int, [D, S, _p, O, _p]
    lib.jss_advance.restype, lib.jss_advance.argtypes = C.c_int, [D, S, _p, _p, O, _p]
    lib.jss_policy.restype, lib.jss_policy.argtypes = C.c_int, [D, S, C.c_int, C.c_uint64, C.c_uint32, _p, _p]
    lib.jss_rollout.restype = C.c_int
    lib.jss_rollout.argtypes = [D, S, O, C.c_int, C.c_uint64, C.c_uint32, C.c_int32, C.c_int32, _p]
    lib.jss_rollout_steps.restype = C.c_int
    lib.jss_rollout_steps.argtypes = [D, S, O, C.c_int, C.c_uint64, C.c_uint32, C.c_int32, C.c_int32, C.c_int32,
                                      C.POINTER(_p)]
    lib.jss_policy_step_steps.restype = C.c_int
    lib.jss_policy_step_steps.argtypes = [D, S, O, C.c_int, C.c_uint64, C.c_uint32, _p, C.c_int32, C.c_int32, C.c_int32,
                                          C.POINTER(_p)]
    lib.jss_rollout_steps_multi.restype = C.c_int
    lib.jss_rollout_steps_multi.argtypes = [C.c_int32, C.POINTER(D), C.POINTER(S), C.POINTER(O), C.c_int, C.c_uint64, C.c_uint32,
                                            C.c_int32, C.c_int32, C.POINTER(_p)]
    PD, PS, PO, PP = C.POINTER(D), C.POINTER(S), C.POINTER(O), C.POINTER(_p)
    lib.jss_multi_reset.restype, lib.jss_multi_reset.argtypes = C.c_int, [C.c_int32, PD, PS, PO, PP, _p]
    lib.jss_multi_step.restype, lib.jss_multi_step.argtypes = C.c_int, [C.c_int32, PD, PS, PP, PO, C.c_int32, _p]
    lib.jss_multi_policy.restype = C.c_int
    lib.jss_multi_policy.argtypes = [C.c_int32, PD, PS, C.c_int, C.c_uint64, C.c_uint32, PP, _p]
    lib.jss_multi_rollout.restype = C.c_int
    lib.jss_multi_rollout.argtypes = [C.c_int32, PD, PS, PO, C.c_int, C.c_uint64, C.c_uint32, C.c_int32, C.c_int32, C.c_int32, PP]
    lib.jss_trajectory.restype = C.c_int
    lib.jss_trajectory.argtypes = [D, S, O, C.POINTER(JssTraj), C.c_int, C.c_uint64, C.c_uint32, C.c_int32, C.c_int32, _p]
    lib.jss_sync_check.restype, lib.jss_sync_check.argtypes = C.c_int, [_p]
    SS = C.POINTER(JssSession)
    lib.jss_steps.restype, lib.jss_steps.argtypes = C.c_int, [D, S, O, C.POINTER(JssTraj), _p, C.c_int32, _p]
    lib.jss_session_open.restype, lib.jss_session_open.argtypes = C.c_int, [D, S, O, SS, _p]
    lib.jss_session_post.restype = C.c_int
    lib.jss_session_post.argtypes = [D, SS, _p, C.c_int32, C.c_int32, C.c_int32, _p]
    lib.jss_session_wait.restype, lib.jss_session_wait.argtypes = C.c_int, [D, SS, C.c_int32, _p]
    lib.jss_session_close.restype, lib.jss_session_close.argtypes = C.c_int, [D, SS, C.c_int32, _p]
    lib.jss_session_step.restype, lib.jss_session_step.argtypes = C.c_int, [D, SS, _p, C.c_int32, _p]
    lib.jss_step_logits.restype = C.c_int
    lib.jss_step_logits.argtypes = [D, S, C.POINTER(JssLogits), C.c_uint64, C.c_int32, O, _p]
    lib.jss_multi_step_logits.restype = C.c_int
    lib.jss_multi_step_logits.argtypes = [C.c_int32, PD, PS, C.POINTER(C.POINTER(JssLogits)), C.c_uint64, C.c_int32, PO, _p]
    lib.jss_generate.restype, lib.jss_generate.argtypes = C.c_int, [D, S, C.POINTER(JssGen), _p, _p]
    lib.jss_clone.restype, lib.jss_clone.argtypes = C.c_int, [D, S, O, C.POINTER(JssCloneDst), D, S, O, _p, _p]
    if lib.jss_abi_version() != ABI_VERSION:
        raise RuntimeError(f"library ABI {lib.jss_abi_version()} != expected {ABI_VERSION}")
    return lib


def bind_search(lib):
    """Attach the prototypes of include/jss_search.h; raises AttributeError naming the first missing symbol."""
    for name in SEARCH_SYMBOLS:
        if not hasattr(lib, name):
            raise AttributeError(f"library does not export {name}")
    lib.jss_lookahead.restype = C.c_int
    lib.jss_lookahead.argtypes = [C.POINTER(JssDesc), C.POINTER(JssState), C.POINTER(JssLookahead), C.c_int, C.c_uint64,
                                  C.c_uint32, C.c_int32, _p]
    return lib


def bind_rules(lib):
    """Attach the prototypes of include/jss_rules.h; raises AttributeError naming the first missing symbol."""
    for name in RULES_SYMBOLS:
        if not hasattr(lib, name):
            raise AttributeError(f"library does not export {name}")
    D, S, O, R = C.POINTER(JssDesc), C.POINTER(JssState), C.POINTER(JssOut), C.POINTER(JssRule)
    lib.jss_rule_policy.restype, lib.jss_rule_policy.argtypes = C.c_int, [D, S, R, C.c_uint64, C.c_uint32, _p, _p]
    lib.jss_rule_rollout.restype = C.c_int
    lib.jss_rule_rollout.argtypes = [D, S, O, R, C.c_uint64, C.c_uint32, C.c_int32, C.c_int32, _p]
    lib.jss_rule_lookahead.restype = C.c_int
    lib.jss_rule_lookahead.argtypes = [D, S, C.POINTER(JssLookahead), R, C.c_uint64, C.c_uint32, C.c_int32, _p]
    return lib


def bind_keys(lib):
    """Attach the prototypes of include/jss_keys.h; raises AttributeError naming the first missing symbol."""
    for name in KEYS_SYMBOLS:
        if not hasattr(lib, name):
            raise AttributeError(f"library does not export {name}")
    D, S, O, K = C.POINTER(JssDesc), C.POINTER(JssState), C.POINTER(JssOut), C.POINTER(JssKeys)
    lib.jss_key_policy.restype, lib.jss_key_policy.argtypes = C.c_int, [D, S, K, C.c_uint64, C.c_uint32, _p, _p]
    lib.jss_key_rollout.restype = C.c_int
    lib.jss_key_rollout.argtypes = [D, S, O, K, C.c_uint64, C.c_uint32, C.c_int32, C.c_int32, _p]
    lib.jss_key_lookahead.restype = C.c_int
    lib.jss_key_lookahead.argtypes = [D, S, C.POINTER(JssLookahead), K, C.c_uint64, C.c_uint32, C.c_int32, _p]
    return lib


def bind_beam(lib):
    """Attach the prototype of include/jss_beam.h; raises AttributeError naming the first missing symbol."""
    for name in BEAM_SYMBOLS:
        if not hasattr(lib, name):
            raise AttributeError(f"library does not export {name}")
    lib.jss_beam_select.restype, lib.jss_beam_select.argtypes = C.c_int, [C.POINTER(JssBeam), _p]
    return lib


def bind_bound(lib):
    """Attach the prototype of include/jss_bound.h; raises AttributeError naming the first missing symbol."""
    for name in BOUND_SYMBOLS:
        if not hasattr(lib, name):
            raise AttributeError(f"library does not export {name}")
    lib.jss_bound.restype = C.c_int
    lib.jss_bound.argtypes = [C.POINTER(JssDesc), C.POINTER(JssState), C.POINTER(JssBound), _p]
    return lib


def bind_order(lib):
    """Attach the prototypes of include/jss_order.h; raises AttributeError naming the first missing symbol."""
    for name in ORDER_SYMBOLS:
        if not hasattr(lib, name):
            raise AttributeError(f"library does not export {name}")
    lib.jss_order_eval.restype = C.c_int
    lib.jss_order_eval.argtypes = [C.POINTER(JssDesc), C.POINTER(JssState), C.POINTER(JssOrder), _p]
    lib.jss_order_apply.restype = C.c_int
    lib.jss_order_apply.argtypes = [C.POINTER(JssOrderApply), _p]
    return lib


def bind_tabu(lib):
    """Attach the prototype of include/jss_tabu.h; raises AttributeError naming the first missing symbol."""
    for name in TABU_SYMBOLS:
        if not hasattr(lib, name):
            raise AttributeError(f"library does not export {name}")
    lib.jss_tabu_search.restype = C.c_int
    lib.jss_tabu_search.argtypes = [C.POINTER(JssDesc), C.POINTER(JssState), C.POINTER(JssTabu), _p]
    return lib


def bind_block(lib):
    """Attach the prototype of include/jss_block.h; raises AttributeError naming the first missing symbol."""
    for name in BLOCK_SYMBOLS:
        if not hasattr(lib, name):
            raise AttributeError(f"library does not export {name}")
    lib.jss_block_search.restype = C.c_int
    lib.jss_block_search.argtypes = [C.POINTER(JssDesc), C.POINTER(JssState), C.POINTER(JssBlock), _p]
    return lib


def bind_relink(lib):
    """Attach the prototype of include/jss_relink.h; raises AttributeError naming the first missing symbol."""
    for name in RELINK_SYMBOLS:
        if not hasattr(lib, name):
            raise AttributeError(f"library does not export {name}")
    lib.jss_relink_walk.restype = C.c_int
    lib.jss_relink_walk.argtypes = [C.POINTER(JssDesc), C.POINTER(JssState), C.POINTER(JssRelink), _p]
    return lib


def bind_decode(lib):
    """Attach the prototypes of include/jss_decode.h; raises AttributeError naming the first missing symbol."""
    for name in DECODE_SYMBOLS:
        if not hasattr(lib, name):
            raise AttributeError(f"library does not export {name}")
    lib.jss_decode_keys.restype = C.c_int
    lib.jss_decode_keys.argtypes = [C.POINTER(JssDesc), C.POINTER(JssState), C.POINTER(JssDecode), _p]
    lib.jss_keys_evolve.restype = C.c_int
    lib.jss_keys_evolve.argtypes = [C.POINTER(JssEvolve), _p]
    return lib


def bind_machine(lib):
    """Attach the prototypes of include/jss_machine.h; raises AttributeError naming the first missing symbol."""
    for name in MACHINE_SYMBOLS:
        if not hasattr(lib, name):
            raise AttributeError(f"library does not export {name}")
    lib.jss_machine_relax.restype = C.c_int
    lib.jss_machine_relax.argtypes = [C.POINTER(JssDesc), C.POINTER(JssState), C.POINTER(JssMachineRelax), _p]
    lib.jss_bottleneck_build.restype = C.c_int
    lib.jss_bottleneck_build.argtypes = [C.POINTER(JssDesc), C.POINTER(JssState), C.POINTER(JssBottleneck), _p]
    return lib


def bind_carlier(lib):
    """Attach the prototypes of include/jss_carlier.h; raises AttributeError naming the first missing symbol."""
    for name in CARLIER_SYMBOLS:
        if not hasattr(lib, name):
            raise AttributeError(f"library does not export {name}")
    lib.jss_machine_solve.restype = C.c_int
    lib.jss_machine_solve.argtypes = [C.POINTER(JssDesc), C.POINTER(JssState), C.POINTER(JssMachineSolve), _p]
    lib.jss_bottleneck_exact.restype = C.c_int
    lib.jss_bottleneck_exact.argtypes = [C.POINTER(JssDesc), C.POINTER(JssState), C.POINTER(JssBottleneckExact), _p]
    return lib


def bind_propagate(lib):
    """Attach the prototype of include/jss_propagate.h; raises AttributeError naming the missing symbol."""
    for name in PROPAGATE_SYMBOLS:
        if not hasattr(lib, name):
            raise AttributeError(f"library does not export {name}")
    lib.jss_propagate.restype = C.c_int
    lib.jss_propagate.argtypes = [C.POINTER(JssDesc), C.POINTER(JssState), C.POINTER(JssPropagate), _p]
    return lib


# The entry-point families behind a selector, by the prefix of their calls: jss_<verb> (the stock rules; include/jss_hip.h is
# bound by `bind`, what may still be missing is the companion header of jss_lookahead), jss_rule_<verb>, jss_key_<verb>.
# Per family: what its companion header declares, what attaches those prototypes, and the header's name.
_FAMILIES = {"jss": (SEARCH_SYMBOLS, bind_search, "jss_search.h"), "jss_rule": (RULES_SYMBOLS, bind_rules, "jss_rules.h"),
             "jss_key": (KEYS_SYMBOLS, bind_keys, "jss_keys.h")}


def ensure_bound(lib, family: str, what: Optional[str] = None):
    """``lib`` with the prototypes of ``family``'s companion header attached (now, unless they are already).  A library that
    does not export every call of the header (a build of the same ABI version older than the header): None, and nothing is
    attached, or -- given ``what``, the caller's name for its messages -- RuntimeError."""
    symbols, binder, header = _FAMILIES[family]
    first = getattr(lib, symbols[0], None)
    if first is not None and first.argtypes is not None:                  # (attached earlier: every call is there)
        return lib
    if not all(hasattr(lib, name) for name in symbols):
        if what is None:
            return None
        raise RuntimeError(f"{what}: the loaded library does not export the {family}_* calls of include/{header}")
    return binder(lib)


def check(lib, rc: int, what: str):
    if rc != 0:
        msg = lib.jss_error_string(rc)
        raise RuntimeError(f"{what} failed: {rc} ({msg.decode() if msg else '?'})")


def bind_onestep(lib):
    """Attach the prototypes of include/jss_onestep.h; raises AttributeError naming the missing symbol."""
    for name in ONESTEP_SYMBOLS:
        if not hasattr(lib, name):
            raise AttributeError(f"library does not export {name}")
    D, S, O = C.POINTER(JssDesc), C.POINTER(JssState), C.POINTER(JssOut)
    lib.jss_onestep_version.restype = C.c_int
    lib.jss_onestep_version.argtypes = []
    lib.jss_onestep_rollout.restype = C.c_int
    lib.jss_onestep_rollout.argtypes = [D, S, O, C.c_int, C.c_uint64, C.c_uint32, C.c_int32, C.c_int32, _p]
    lib.jss_onestep_rollout_steps.restype = C.c_int
    lib.jss_onestep_rollout_steps.argtypes = [D, S, O, C.c_int, C.c_uint64, C.c_uint32, C.c_int32, C.c_int32, C.c_int32,
                                              C.POINTER(_p)]
    if lib.jss_onestep_version() != ONESTEP_VERSION:
        raise RuntimeError(f"include/jss_onestep.h version {lib.jss_onestep_version()}, this package binds {ONESTEP_VERSION}")
    return lib
