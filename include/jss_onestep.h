/*
 * include/jss_onestep.h -- the one-step rollout of the flagship class, a companion of jss_hip.h (whose JSS_ABI_VERSION it
 * leaves alone).  libjss_onestep_hip.so (jssenv_amd/csrc/jss_onestep.hip: a library of its own next to libjss_hip.so, whose
 * kernels it does not touch) exports the two entry points; pointers are device pointers.  The host-core twin has no
 * counterpart: on the host jss_rollout / jss_rollout_steps are the only form.
 *
 *   jss_onestep_rollout       <- jss_rollout with n_iter == 1
 *   jss_onestep_rollout_steps <- jss_rollout_steps
 *
 * THE CLASS.  A batch is served when all of this holds, and the calls answer with an error before anything is launched
 * when it does not:
 *   one shared instance         n_tables == 1 and no table_of_env         else JSS_E_SHAPE
 *   compact 16-byte records     record_ints == JSS_NFC                    else JSS_E_SHAPE
 *   a 16- or 32-lane group      jmax <= 32 and mmax <= 32                 else JSS_E_SHAPE
 *   the packed flavour          JssDesc.kernel without JSS_KERNEL_WAVE    else JSS_E_KIND
 *   a stock rule                kind as jss_rollout takes it (no JSS_POLICY_CR_F64, no caller's selector)   else JSS_E_KIND
 *   one iteration               jss_onestep_rollout: n_iter == 1          else JSS_E_SHAPE
 * Everything else is checked as jss_rollout / jss_rollout_steps check it, with the same codes.
 *
 * RESULTS.  State, solution, outputs and counters after a call are byte for byte those of the namesake in libjss_hip.so
 * with the same arguments: the kernel is the same body (jss_packed_env.hpp).  What differs is how its results leave the chip:
 * every store is a write-through store, so that a launch ends without dirty lines in the L2 for the next step's launch to
 * wait for (jssenv_amd/csrc/jss_onestep.hip has the measurements).
 */
#ifndef JSS_ONESTEP_H
#define JSS_ONESTEP_H

#include "jss_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JSS_ONESTEP_VERSION 1

int jss_onestep_version(void);

/* jss_rollout(desc, state, out, kind, seed, explore_q16, 1, flags, stream) */
int jss_onestep_rollout(const JssDesc *desc, const JssState *state, const JssOut *out, int kind, uint64_t seed,
                        uint32_t explore_q16, int32_t n_iter, int32_t flags, void *stream);

/* jss_rollout_steps: n_sub, streams and JSS_ROLLOUT_FORK_JOIN as there; n_steps == 0 launches nothing */
int jss_onestep_rollout_steps(const JssDesc *desc, const JssState *state, const JssOut *out, int kind, uint64_t seed,
                              uint32_t explore_q16, int32_t n_steps, int32_t flags, int32_t n_sub, void *const *streams);

#ifdef __cplusplus
}
#endif
#endif
