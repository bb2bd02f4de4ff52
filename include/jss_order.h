/*
 * include/jss_order.h -- exact evaluation of machine orders, the seventh companion of jss_hip.h (whose JSS_ABI_VERSION it leaves
 * alone).  libjss_order_hip.so (jssenv_amd/csrc/jss_order.hip: a library of its own next to libjss_hip.so, libjss_beam_hip.so and
 * libjss_bound_hip.so, whose kernels it does not touch) and libjss_cpu.so export the two entry points, with identical semantics;
 * pointers are device pointers for the HIP library and host pointers for the twin, as in jss_hip.h.
 *
 *   jss_order_eval  <- what every improvement method asks (tabu search, annealing, machine-permutation GAs, a policy that
 *                      proposes an order): given this order of the operations on each machine, what is the schedule and how long
 *                      is it?  Also every operation's tail, the critical operations and the swap neighbourhood.
 *   jss_order_apply <- one steepest-descent step's bookkeeping on the device: the best swap candidate of every env, taken if it
 *                      improves.
 */
#ifndef JSS_ORDER_H
#define JSS_ORDER_H

#include "jss_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JSS_ORDER_VERSION 1

/* ---- the semi-active schedule of a machine order -----------------------------------------------------------------------------
 * Integer arithmetic only: both libraries (and jssenv_amd.search.order_eval_reference, the NumPy mirror) give the same bits.
 * Candidate c looks at env i = parent[c] of the batch (desc, state) and reads env_const[i] (JSS_C_JOBS, JSS_C_MACHINES,
 * JSS_C_TABLE) and the op table only -- not the clock, not the solution.  Nothing of the batch is written.
 *
 *   J, M, table         env_const[i];  mach(j,k), d(j,k): the op table entry of the env's table, machine << 16 | duration
 *   real operations     (j,k) with j < J and k < M; every other entry of a [jmax][mmax] row is padding
 *   r(j,k)              rank[i][j][k], after the candidate's swap: if swap_a[c] = a and swap_b[c] = b are given and not both -1,
 *                       the entries at the flat indices a and b (flat = j * mmax + k) are exchanged first.  The exchange is the
 *                       callee's own: rank is never written.  a == b is allowed and changes nothing.
 *   order on machine m  its operations -- the real (j,k) with mach(j,k) == m -- ascending by (r, j, k)
 *   start(j,k)          max(start(j,k-1) + d(j,k-1), start(p) + d(p)), p the operation before (j,k) on its machine; a missing
 *                       predecessor (k == 0, first on the machine) counts as 0
 *   makespan            max over the real operations of start + d
 *   tail(j,k)           max(d(j,k+1) + tail(j,k+1), d(s) + tail(s)), s the operation behind (j,k) on its machine; a missing
 *                       successor counts as 0
 *   critical            start + d + tail == makespan
 *   pair                two operations u, v, v directly behind u on one machine's order, of different jobs, both critical, with
 *                       start(v) == start(u) + d(u): the arcs whose reversal can shorten the schedule.  Listed by machine
 *                       ascending, then by u's position ascending, as flat indices (pair_a = u, pair_b = v).
 * Machines may repeat within a job or be unused by the instance.
 *
 * makespan[c] = -1 (refused) when: parent[c] is outside [0, B); the parent was never reset (JSS_C_JOBS == 0); a real operation's
 * rank (as stored) is negative -- so the solution of an unfinished env is refused; exactly one of the swap indices is -1; or a
 * swap index other than the pair (-1, -1) is outside [0, jmax * mmax) or names a padding entry.
 * makespan[c] = -2 when the order is cyclic with the job chains (no schedule exists).
 * In both cases the candidate's rows of start, tail, pair_a, pair_b and its n_pairs keep what they held.
 *
 * Otherwise, each where given: start[c] and tail[c] hold the values above, -1 in the padding; n_pairs[c] is the number of pairs
 * found -- also when that exceeds pair_cap, so the caller sees the truncation -- pair_a[c], pair_b[c] hold the first
 * min(n_pairs[c], pair_cap) of them and -1 behind.
 *
 * One wavefront per candidate, in the caller's order.  The HIP library holds a candidate's op row and sequences in LDS:
 * 12 bytes per entry of a [jmax][mmax] row (the entries rounded up to a multiple of 8) plus 1280; a batch shape that needs more
 * than 64 KB for one candidate (beyond 5352 entries; 100 x 20 and 128 x 40 fit) is JSS_E_LDS, from both libraries.
 *
 * Errors (checked before anything runs, the same code from both libraries; nothing is written then):
 *   JSS_E_NULL  desc, state, o, o->rank or o->makespan NULL, or what jss_lookahead's desc / state checks reject;
 *   JSS_E_SHAPE o->n < 0; o->parent == NULL with o->n != desc->batch; one of swap_a / swap_b without the other; some but not all
 *               of pair_a, pair_b, n_pairs; pair outputs with pair_cap < 1; or a desc / state shape jss_lookahead rejects;
 *   JSS_E_LDS   see above.
 * o->n == 0 launches nothing and returns 0. */
typedef struct JssOrder {
    int32_t n;              /* candidates */
    int32_t pair_cap;       /* entries per row of pair_a / pair_b (looked at only when they are given) */
    const int32_t *rank;    /* [B][jmax][mmax], one row per env: the shape of the solution and of the key tables */
    const int32_t *parent;  /* [n], or NULL: candidate k is env k (n must equal desc->batch) */
    const int32_t *swap_a;  /* [n] flat indices, or NULL (with swap_b): no swaps */
    const int32_t *swap_b;  /* [n] */
    int32_t *makespan;      /* [n] out: the makespan, -1 refused, -2 cyclic */
    int32_t *start;         /* [n][jmax][mmax] out or NULL */
    int32_t *tail;          /* [n][jmax][mmax] out or NULL */
    int32_t *pair_a;        /* [n][pair_cap] out or NULL (with pair_b and n_pairs) */
    int32_t *pair_b;        /* [n][pair_cap] */
    int32_t *n_pairs;       /* [n] */
} JssOrder;

int jss_order_eval(const JssDesc *desc, const JssState *state, const JssOrder *o, void *stream);

/* ---- one descent step's bookkeeping --------------------------------------------------------------------------------------------
 * Per env i of the batch rows: among the candidates k < pair_cap with makespan[i][k] >= 0 and both pair_a[i][k] and pair_b[i][k]
 * inside [0, jmax * mmax), the one with the lowest (makespan, k).  If there is one and its makespan is < cur[i], the entries of
 * rank[i] at its two flat indices are exchanged, cur[i] becomes that makespan and improved[i] = 1; otherwise improved[i] = 0 and
 * nothing else of the env is written.  This is what follows two jss_order_eval calls (the rows with pairs out, then the
 * batch * pair_cap swap candidates) in a descent, so that an iteration needs no host round trip.
 *
 * Errors (before anything runs): JSS_E_NULL for a NULL a or member pointer; JSS_E_SHAPE for batch < 0, jmax outside
 * [1, JSS_MAX_JOBS], mmax outside [1, JSS_MAX_MACHINES] or pair_cap < 1.  batch == 0 launches nothing and returns 0. */
typedef struct JssOrderApply {
    int32_t batch, jmax, mmax, pair_cap;
    int32_t *rank;            /* [batch][jmax][mmax] in / out */
    int32_t *cur;             /* [batch] in / out: the current makespans */
    const int32_t *makespan;  /* [batch][pair_cap] the candidates' makespans */
    const int32_t *pair_a;    /* [batch][pair_cap] */
    const int32_t *pair_b;    /* [batch][pair_cap] */
    int32_t *improved;        /* [batch] out: 0 or 1 */
} JssOrderApply;

int jss_order_apply(const JssOrderApply *a, void *stream);

#ifdef __cplusplus
}
#endif
#endif
