/*
 * include/jss_rules.h -- caller-weighted dispatching rules of libjss_hip.so and libjss_cpu.so: the policy, rollout and
 * lookahead calls with a selector the CALLER parametrises, a row of integer weights over the quantities the stock rules
 * read.  A companion of jss_hip.h and jss_search.h (whose structs it takes, and whose JSS_ABI_VERSION / JSS_SEARCH_VERSION it
 * leaves alone): a client of those interfaces never sees these symbols.  Both libraries export them, with identical
 * semantics; pointers are device pointers for libjss_hip.so and host pointers for libjss_cpu.so, as in jss_hip.h.
 *
 *   jss_rule_policy    <- DispatchingRule.select_action of a user's subclass (dispatching.py), for every env of a batch
 *   jss_rule_rollout   <- DispatchingRule.run_episode with it; with one weight row per env, a whole population of candidate
 *                         rules (ES, CMA-ES, random-key GA, GP over linear rules) is one launch
 *   jss_rule_lookahead <- the pilot method / MCTS leaf evaluation with a tuned rule
 */
#ifndef JSS_RULES_H
#define JSS_RULES_H

#include "jss_hip.h"
#include "jss_search.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JSS_RULES_VERSION 1

/* ---- a weighted rule ------------------------------------------------------------------------------------------------
 * A rule is a row of JSS_RW_N int32.  Weights 0-6 multiply a quantity x_f(j) of a legal job j:                          */
#define JSS_RW_DUR 0    /* duration of its current op (what SPT reads)                                                   */
#define JSS_RW_NEXT 1   /* duration of the op after it, 0 if there is none                                               */
#define JSS_RW_REM 2    /* remaining work, the durations of its ops from the current one on (MWR / LWR)                  */
#define JSS_RW_TOTAL 3  /* job length, the durations of all its ops (CriticalRatio's)                                    */
#define JSS_RW_OPS 4    /* remaining ops, M - ops done (MOR / LOR)                                                       */
#define JSS_RW_WAIT 5   /* idle time since its last op (FIFO)                                                            */
#define JSS_RW_IDLE 6   /* total idle time of the job                                                                    */
#define JSS_RW_NOPE 7   /* NOPE bias, or JSS_RW_NEVER_NOPE                                                               */
#define JSS_RW_N 8
#define JSS_RW_NEVER_NOPE (-2147483647 - 1)
/*
 *   score(j) = sum over f < 7 of (int64) w[f] * (int64) x_f(j), in wrapping 64-bit two's-complement arithmetic.
 *
 * The action:
 *   - the legal job with the largest score, the lowest job index on ties (the strict comparisons of the stock rules);
 *   - NOPE if no job is legal and NOPE is;
 *   - NOPE if jobs are legal, NOPE is legal, w[JSS_RW_NOPE] != JSS_RW_NEVER_NOPE and (int64) w[JSS_RW_NOPE] > the best score;
 *   - then explore_q16 acts exactly as for the stock rules, with the same random key: NOPE, where it is legal, with
 *     probability explore_q16 / 65536;
 *   - -1 if nothing is legal, as jss_policy answers.
 * Everything is integer: the device, the host twin and a mirror written in any language agree bit for bit.  Float weights are
 * the caller's to quantise (scale, round); with |w| <= 2^15 no sum of the seven products can wrap.
 *
 * weights: [B][JSS_RW_N] with stride == JSS_RW_N -- env i of the batch uses row i: a population of rules -- or one row that
 * every env uses, stride == 0.  The SPT rule is {-1, 0, 0, 0, 0, 0, 0, JSS_RW_NEVER_NOPE}, MWR {0, 0, 1, 0, ...}: such a row
 * gives what the stock rule gives, bit for bit.  `weights` is 16-byte aligned (rows are read four weights at a time). */
typedef struct JssRule {
    const int32_t *weights;   /* [B][JSS_RW_N], or [JSS_RW_N] with stride 0; 16-byte aligned                            */
    int32_t stride;           /* 0 or JSS_RW_N                                                                          */
} JssRule;

/* Each call is its jss_hip.h / jss_search.h namesake with the selector above in place of `kind`: outputs, counters, flags,
 * random keying and the order of the argument checks are those of jss_policy / jss_rollout / jss_lookahead.
 *
 * jss_rule_lookahead: candidate k uses the row of la->parent[k] (stride JSS_RW_N) or the shared row.  As an exact
 * equivalence, its results are what
 *       fork([parent[k]], env_id_base = id_base + k)
 *       step(action[k])                                                      (skipped for JSS_ACTION_SKIP)
 *       jss_rule_rollout(rule' , n_iter, seed, explore_q16, flags = 0)
 * would give, where rule' is the fork's one row: row parent[k] of `rule`, or its shared row -- makespan, env steps and
 * reward numerators, bit for bit.
 *
 * Errors, checked before anything runs, the same code from both libraries, nothing written: what the namesake answers, and
 * in the place of its kind check
 *   JSS_E_NULL  rule or rule->weights NULL, or a batch without the remaining-work table (JssDesc.rem);
 *   JSS_E_SHAPE rule->stride neither 0 nor JSS_RW_N, or rule->weights not 16-byte aligned.
 * Not covered: the windowed and recording calls (jss_rollout_steps, jss_trajectory, ...), the multi-set calls and the step
 * session. */
int jss_rule_policy(const JssDesc *desc, const JssState *state, const JssRule *rule, uint64_t seed, uint32_t explore_q16,
                    int32_t *actions, void *stream);
int jss_rule_rollout(const JssDesc *desc, const JssState *state, const JssOut *out, const JssRule *rule, uint64_t seed,
                     uint32_t explore_q16, int32_t n_iter, int32_t flags, void *stream);
int jss_rule_lookahead(const JssDesc *desc, const JssState *state, const JssLookahead *la, const JssRule *rule,
                       uint64_t seed, uint32_t explore_q16, int32_t n_iter, void *stream);

#ifdef __cplusplus
}
#endif
#endif
