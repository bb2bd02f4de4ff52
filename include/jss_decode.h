/*
 * include/jss_decode.h -- Giffler-Thompson decoding of per-operation priority keys and one BRKGA generation, the eleventh
 * companion of jss_hip.h (whose JSS_ABI_VERSION it leaves alone, as it leaves JSS_KEYS_VERSION, JSS_ORDER_VERSION, JSS_TABU_VERSION,
 * JSS_BLOCK_VERSION and JSS_RELINK_VERSION).  libjss_decode_hip.so (jssenv_amd/csrc/jss_decode.hip: a library of its own next to
 * libjss_hip.so, libjss_beam_hip.so, libjss_bound_hip.so, libjss_order_hip.so, libjss_tabu_hip.so, libjss_block_hip.so and
 * libjss_relink_hip.so, whose kernels it does not touch) and libjss_cpu.so export the two entry points, with identical semantics;
 * pointers are device pointers for the HIP library and host pointers for the twin, as in jss_hip.h.
 *
 *   jss_decode_keys <- a key table (jss_keys.h: one int32 priority per operation) decoded into an ACTIVE schedule by Giffler and
 *                      Thompson's procedure, or with a delay parameter into Bierwirth and Mattfeld's hybrid between non-delay and
 *                      active schedules: the makespan, the start times (a machine order for jss_order.h, jss_tabu.h, jss_block.h
 *                      and jss_relink.h) and three counters.  One decode per candidate; no env is stepped.
 *   jss_keys_evolve <- one generation of a biased random-key genetic algorithm on plain arrays: ranking, elite copies,
 *                      mutants, biased uniform crossover.
 */
#ifndef JSS_DECODE_H
#define JSS_DECODE_H

#include "jss_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JSS_DECODE_VERSION 1

#define JSS_DECODE_NI 4     /* info row: conflicts, widest, delayed, 0 */

#define JSS_EVOLVE_SEED_XOR 0xD1B54A32D192ED03ULL   /* keys the counter RNG of jss_keys_evolve */
#define JSS_EVOLVE_MAX_POP 4096

/* ---- the decode ----------------------------------------------------------------------------------------------------------------
 * Integer arithmetic only: both libraries (and jssenv_amd.search.decode_reference, the NumPy mirror) give the same bits.
 * Candidate c looks at env i = parents[c] of the batch (desc, state) -- env c where parents is NULL -- and reads env_const[i]
 * (JSS_C_JOBS, JSS_C_MACHINES, JSS_C_TABLE) and the op table only.  Nothing of the batch is written.  Its key table is
 * keys[c] (stride == jmax * mmax: indexed by the CANDIDATE, not by the parent) or the one shared table (stride == 0); its delay
 * parameter delta is delta_of[c] where delta_of is given, else delta_q16.
 *
 * Refused (makespan[c] = -1; the candidate's rows of start and info keep what they held): the parent is outside [0, B); the
 * parent's JSS_C_JOBS < 1 (never reset) or what else jss_order_eval refuses of an env; delta outside [0, 65536].
 *
 * Setup.  J, M and the table from env_const[i]; mach(j,k), d(j,k) the op table's entry, machine << 16 | duration.  Per job j:
 * k_j = 0 operations scheduled, jobend_j = 0.  Per machine m: rel_m = 0.  The current operation of an unfinished job (k_j < M) is
 * (j, k_j), with m_j = mach(j, k_j), d_j = d(j, k_j) and the key keys[..][j][k_j] as a signed int32.
 *
 * Repeat J * M times:
 *   1. for every unfinished job: est_j = max(jobend_j, rel[m_j]), ect_j = est_j + d_j;
 *   2. j* the unfinished job with the lowest (ect_j, j); c* = ect_j*, m* = m_j*;
 *   3. e0 = the minimum of est_j over the unfinished jobs with m_j == m*;
 *   4. the conflict set: the unfinished jobs with m_j == m* and either est_j == e0 or
 *          (int64)(est_j - e0) * 65536 < (int64)delta * (c* - e0).
 *      delta == 65536 is Giffler and Thompson's est_j < c* (active schedules); delta == 0 keeps only the operations that can
 *      start earliest (non-delay schedules);
 *   5. the chosen job: the one of the set with the LARGEST key, the lowest job index on ties (jss_keys.h's comparison; every
 *      int32 is a valid key);
 *   6. it starts at s = est_j: start[c][j][k_j] = s, jobend_j = rel[m*] = s + d_j, k_j += 1.
 * Durations of 0 are well defined.
 *
 * Outputs.  makespan[c] = max jobend.  start[c] (where given) holds the start times, -1 in the padding: a rank tensor for
 * jss_order_eval, which returns the same makespan and the same starts.  info[c] (where given) = (conflicts, widest, delayed, 0):
 * the iterations whose conflict set held more than one job, the size of the largest set, the iterations whose chosen start
 * exceeded e0.
 *
 * One wavefront per candidate.  The HIP library holds a candidate's op row, key row and one word per machine in LDS:
 *     8 bytes per entry of a [jmax][mmax] row (the entries rounded up to a multiple of 8) plus 256
 * and a batch shape that needs more than 64 KB for one candidate (beyond 8160 entries; 128 x 63 fits, 128 x 64 does not) is
 * JSS_E_LDS, from both libraries.
 *
 * Errors (checked before anything runs, the same code from both libraries; nothing is written then):
 *   JSS_E_NULL  desc, state, dc, dc->keys or dc->makespan NULL, or what jss_order_eval's desc / state checks reject;
 *   JSS_E_SHAPE dc->n < 0; dc->stride neither 0 nor jmax * mmax; dc->delta_q16 outside [0, 65536]; dc->parents == NULL with
 *               dc->n != desc->batch; or a desc / state shape jss_order_eval rejects;
 *   JSS_E_LDS   see above.
 * dc->n == 0 launches nothing and returns 0. */
typedef struct JssDecode {
    int32_t n;                  /* candidates */
    int32_t stride;             /* 0: one table for all; jmax * mmax: table c for candidate c */
    int32_t delta_q16;          /* [0, 65536]; used where delta_of is NULL */
    const int32_t *parents;     /* [n] or NULL: candidate c is env c (n must equal desc->batch) */
    const int32_t *keys;        /* [n][jmax][mmax] or [jmax][mmax] */
    const int32_t *delta_of;    /* [n] or NULL */
    int32_t *makespan;          /* [n] out; -1 refused */
    int32_t *start;             /* [n][jmax][mmax] out or NULL */
    int32_t *info;              /* [n][JSS_DECODE_NI] out or NULL */
} JssDecode;

int jss_decode_keys(const JssDesc *desc, const JssState *state, const JssDecode *dc, void *stream);

/* ---- one BRKGA generation -------------------------------------------------------------------------------------------------------
 * Plain arrays, no desc.  G groups of P individuals, each a row of `region` int32 keys; individual p of group g is row
 * i = g * P + p.
 *
 * Ranking.  by_rank[g * P + r] = the p with the r-th lowest (fitness < 0, fitness, p) of group g: lower is better, a negative
 * fitness (a refused decode) ranks behind every non-negative one.
 *
 * Child c of group g, row i = g * P + c of keys_out, with R(x) = rng_u32(seed ^ JSS_EVOLVE_SEED_XOR, i, generation, x), rng_u32
 * the counter RNG of jss_step_logits and jss_generate (oracle/jss_oracle.c orc_rng_u32):
 *   c < n_elite          a copy of row by_rank[c] of the group;
 *   c >= P - n_mutant    entry e is (int32_t)R(e);
 *   otherwise            the elite parent is by_rank[R(region) % n_elite], the other parent
 *                        by_rank[n_elite + R(region + 1) % (P - n_elite)]; entry e comes from the elite parent iff
 *                        (R(e) >> 16) < rho_q16.
 * Padding entries are entries like any other.  n_elite == 0 with n_mutant == P makes an initial population: fitness and
 * keys_in are not read then and may be NULL, and by_rank, where given, lists every group's individuals in their own order.
 * Without a by_rank the HIP library ranks into device memory of the call's own, and freeing it waits for the device: a
 * caller that wants no such wait gives a by_rank.
 *
 * Errors (before anything runs; nothing is written then):
 *   JSS_E_NULL  ev or keys_out NULL; fitness or keys_in NULL unless n_elite == 0 and n_mutant == pop; keys_out == keys_in;
 *   JSS_E_SHAPE pop < 1; pop > JSS_EVOLVE_MAX_POP; region < 1; groups < 0; n_elite < 0; n_mutant < 0; rho_q16 outside
 *               [0, 65536]; n_elite + n_mutant > pop; n_elite + n_mutant < pop with n_elite < 1.
 * groups == 0 launches nothing and returns 0. */
typedef struct JssEvolve {
    int32_t groups;             /* G */
    int32_t pop;                /* P, [1, 4096] */
    int32_t region;             /* entries per key table */
    int32_t n_elite;
    int32_t n_mutant;
    int32_t rho_q16;            /* [0, 65536]: the elite parent's share of a crossover child */
    int32_t generation;
    uint64_t seed;
    const int32_t *fitness;     /* [G * P] */
    const int32_t *keys_in;     /* [G * P][region] */
    int32_t *keys_out;          /* [G * P][region] out; must not alias keys_in */
    int32_t *by_rank;           /* [G * P] out or NULL */
} JssEvolve;

int jss_keys_evolve(const JssEvolve *ev, void *stream);

#ifdef __cplusplus
}
#endif
#endif
