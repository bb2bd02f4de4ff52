/*
 * include/jss_search.h -- search extensions of libjss_hip.so and libjss_cpu.so: calls that evaluate candidate moves of a
 * batch without changing it.  A companion of jss_hip.h (whose JssDesc / JssState it takes, and whose JSS_ABI_VERSION it
 * leaves alone): a client of the v14 interface never sees these symbols.  Both libraries export them, with identical
 * semantics; pointers are device pointers for libjss_hip.so and host pointers for libjss_cpu.so, as in jss_hip.h.
 *
 *   jss_lookahead <- the pilot method's inner loop (also MCTS leaf evaluation, beam search, N random continuations of
 *                    one state): for each candidate, copy.deepcopy(env), step(action), then
 *                    DispatchingRule.run_episode (dispatching.py:55-75) to the end, and keep only the final makespan
 */
#ifndef JSS_SEARCH_H
#define JSS_SEARCH_H

#include "jss_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JSS_SEARCH_VERSION 1

/* ---- score candidate actions by rule rollouts --------------------------------------------------------------------
 * jss_lookahead evaluates la->n candidates.  Candidate k starts from env la->parent[k] of the batch (desc, state), takes the
 * forced first action la->action[k] and then follows policy `kind` until the episode ends, in registers, and writes three
 * numbers: nothing of the batch is written -- not the state, the outputs, the counters or the status -- and no copy of the
 * env is stored anywhere.
 *
 * Candidate k is defined as an exact equivalence.  Its results are what
 *       fork([parent[k]], env_id_base = id_base + k)                        (jss_clone into a fresh batch, counters 0)
 *       step(action[k])                                                      (jss_step; skipped for JSS_ACTION_SKIP)
 *       rollout(kind, n_iter, seed, explore_q16, flags = 0)                  (jss_rollout, no auto-reset)
 * would give: that fork's `makespan` output, its counters' env steps and its counters' reward numerators -- bit for bit,
 * for every policy, the random one and explore_q16 > 0 included.  The fork copies the header, so the random draws are
 * keyed by (seed, id_base + k, the parent's episode, the parent's step count); desc->env_ids is not used.
 *
 *   makespan[k] = -1, steps[k] = 0, reward_num[k] = 0 when there is nothing to evaluate: parent[k] outside [0, B), the
 *                 parent done (no legal action) or never reset, action[k] outside [-1, J(parent)], or a job / NOPE that
 *                 is not set in the parent's action mask.
 *   makespan[k] = -1 also when the continuation has not reached done after n_iter policy steps; steps[k] and
 *                 reward_num[k] then report what was done, as the fork's counters would.
 *
 * Candidates are evaluated in the caller's order, one per 16- / 32-lane group or per wavefront (the kernel flavour of the
 * batch, as jss_rollout picks it), each reading its parent's header, constants, job records and machine clocks; list the
 * candidates of one parent next to each other (parent-major) and they share the parent's cache lines.  The shared op
 * table of a one-instance batch is staged in LDS per workgroup as for the rollouts.
 *
 * Errors (checked before anything runs, the same code from both libraries; nothing is written then):
 *   JSS_E_NULL  desc, state, la, la->parent, la->action or la->makespan NULL, or what jss_rollout's desc / state checks
 *               reject as NULL (JssOut is not taken);
 *   JSS_E_SHAPE la->n < 0, n_iter < 0, or a desc / state shape jss_rollout rejects;
 *   JSS_E_KIND  an unknown kind, and JSS_POLICY_CR_F64 (the rollout kernels carry no float64 code).
 * la->n == 0 launches nothing and returns 0.  Not covered: the multi-set calls' jclass / mclass (a range of a batch dealt
 * out by shape class is evaluated on the kernel of the padded extents), and JSS_POLICY_CR_F64. */
typedef struct JssLookahead {
    int32_t n;                /* candidates                                                                         */
    const int32_t *parent;    /* [n] env of the batch candidate k starts from                                       */
    const int32_t *action;    /* [n] forced first action: job, J(parent) = NOPE; JSS_ACTION_SKIP = none             */
    int64_t id_base;          /* candidate k draws its random numbers as global env id id_base + k                  */
    int32_t *makespan;        /* [n] out: clock at done; -1 = nothing to evaluate, or not done after n_iter steps    */
    int32_t *steps;           /* [n] out or NULL: env steps taken, the forced one included                          */
    int64_t *reward_num;      /* [n] out or NULL: sum of reward numerators (reward * max_time_op)                   */
} JssLookahead;

int jss_lookahead(const JssDesc *desc, const JssState *state, const JssLookahead *la, int kind, uint64_t seed,
                  uint32_t explore_q16, int32_t n_iter, void *stream);

#ifdef __cplusplus
}
#endif
#endif
