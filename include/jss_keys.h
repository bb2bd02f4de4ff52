/*
 * include/jss_keys.h -- per-operation priority keys of libjss_hip.so and libjss_cpu.so: the policy, rollout and lookahead
 * calls with a selector the CALLER tabulates, one int32 priority per operation of the instance -- Bean's random keys, BRKGA,
 * priority-list decoding, a network that ranks every operation once.  A companion of jss_hip.h, jss_search.h and jss_rules.h
 * (it takes the structs of the first two, and leaves JSS_ABI_VERSION / JSS_SEARCH_VERSION / JSS_RULES_VERSION alone): a client
 * of those interfaces never sees these symbols.  Both libraries export them, with identical semantics; pointers are device
 * pointers for libjss_hip.so and host pointers for libjss_cpu.so, as in jss_hip.h.
 *
 *   jss_key_policy    <- a priority-list decoder's next move, for every env of a batch
 *   jss_key_rollout   <- the decoder itself: a chromosome is a key table, its fitness the makespan; with one table per env a
 *                        whole population (GA, BRKGA, CMA-ES over keys, local search on key vectors) is one launch
 *   jss_key_lookahead <- the pilot method / MCTS leaf evaluation with a key table as the continuation
 */
#ifndef JSS_KEYS_H
#define JSS_KEYS_H

#include "jss_hip.h"
#include "jss_search.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JSS_KEYS_VERSION 1

/* ---- a key table ----------------------------------------------------------------------------------------------------
 *   key(j) = keys[env][j][k],  k = the number of operations job j has completed: the index of its current operation
 *            (the `todo` of its record).
 * The table is row-major over the batch's PADDED extents, [jmax][mmax] int32 per env, whatever J(env) and M(env) are;
 * entries with j >= J(env) or k >= M(env) are never read.
 *
 * The action:
 *   - the legal job with the largest key as a signed int32, the lowest job index on ties (the strict comparisons of the stock
 *     rules).  Every int32 value is a valid key, INT32_MIN included;
 *   - NOPE if no job is legal and NOPE is;
 *   - NOPE if jobs are legal, NOPE is legal and nope_key > the best key.  INT32_MIN exceeds nothing: it means "never",
 *     without a special case;
 *   - then explore_q16 acts exactly as for the stock rules, with the same random key: NOPE, where it is legal, with
 *     probability explore_q16 / 65536;
 *   - -1 if nothing is legal, as jss_policy answers.
 * Everything is integer: the device, the host twin and a mirror written in any language agree bit for bit.  Float priorities
 * are the caller's to map to int32 (an order-preserving map exists: dispatching.keys_from_floats).
 *
 * keys: [B][jmax][mmax] with stride == jmax * mmax -- env i of the batch uses table i: a population of chromosomes -- or one
 * table that every env uses, stride == 0.  -duration is SPT, remaining work MWR, ...: such a table gives what the stock rule
 * gives, bit for bit.  No alignment beyond an int32's 4 bytes is asked for. */
typedef struct JssKeys {
    const int32_t *keys;   /* [B][jmax][mmax] with stride == jmax*mmax (env i uses table i), or [jmax][mmax] with stride 0 */
    int32_t stride;        /* 0 or desc->jmax * desc->mmax, in int32s                                                       */
    int32_t nope_key;      /* NOPE's key, the same for every env; INT32_MIN = NOPE only when no job is legal                */
} JssKeys;                 /* 16 bytes, like JssRule */

/* Each call is its jss_hip.h / jss_search.h namesake with the selector above in place of `kind`: outputs, counters, flags,
 * random keying and the order of the argument checks are those of jss_policy / jss_rollout / jss_lookahead.
 *
 * jss_key_lookahead: candidate k uses the table of la->parent[k] (stride jmax * mmax) or the shared table.  As an exact
 * equivalence, its results are what
 *       fork([parent[k]], env_id_base = id_base + k)
 *       step(action[k])                                                      (skipped for JSS_ACTION_SKIP)
 *       jss_key_rollout(keys' , n_iter, seed, explore_q16, flags = 0)
 * would give, where keys' is the fork's one table: table parent[k] of `keys`, or its shared table, with the same nope_key --
 * makespan, env steps and reward numerators, bit for bit.
 *
 * Errors, checked before anything runs, the same code from both libraries, nothing written: what the namesake answers, and
 * in the place of its kind check
 *   JSS_E_NULL  keys or keys->keys NULL;
 *   JSS_E_SHAPE keys->stride neither 0 nor desc->jmax * desc->mmax.
 * The remaining-work table (JssDesc.rem) is not needed: the selector does not read it.
 * Not covered: the windowed and recording calls (jss_rollout_steps, jss_trajectory, ...), the multi-set calls and the step
 * session.  A batch dealt out by shape class runs on the padded extents' kernel, its tables indexed by the env's position in
 * the batch. */
int jss_key_policy(const JssDesc *desc, const JssState *state, const JssKeys *keys, uint64_t seed, uint32_t explore_q16,
                   int32_t *actions, void *stream);
int jss_key_rollout(const JssDesc *desc, const JssState *state, const JssOut *out, const JssKeys *keys, uint64_t seed,
                    uint32_t explore_q16, int32_t n_iter, int32_t flags, void *stream);
int jss_key_lookahead(const JssDesc *desc, const JssState *state, const JssLookahead *la, const JssKeys *keys,
                      uint64_t seed, uint32_t explore_q16, int32_t n_iter, void *stream);

#ifdef __cplusplus
}
#endif
#endif
