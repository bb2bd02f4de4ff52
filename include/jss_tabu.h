/*
 * include/jss_tabu.h -- tabu search over machine orders, the eighth companion of jss_hip.h (whose JSS_ABI_VERSION it leaves
 * alone, as it leaves JSS_ORDER_VERSION).  libjss_tabu_hip.so (jssenv_amd/csrc/jss_tabu.hip: a library of its own next to
 * libjss_hip.so, libjss_beam_hip.so, libjss_bound_hip.so and libjss_order_hip.so, whose kernels it does not touch) and
 * libjss_cpu.so export the entry point, with identical semantics; pointers are device pointers for the HIP library and host
 * pointers for the twin, as in jss_hip.h.
 *
 *   jss_tabu_search <- a whole walk per env in one launch: from a machine order, up to `iters` moves over the swap neighbourhood
 *                      of jss_order.h (adjacent critical operations on a machine), the best neighbour taken also when it is worse,
 *                      the pairs of the last `tenure` moves tabu unless they beat the best schedule seen (aspiration).
 */
#ifndef JSS_TABU_H
#define JSS_TABU_H

#include "jss_order.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JSS_TABU_VERSION 1

#define JSS_TABU_NI 4           /* info row: stop, moves, best_move, evaluations */

/* ---- the walk ------------------------------------------------------------------------------------------------------------------
 * Integer arithmetic only: both libraries (and jssenv_amd.search.tabu_reference, the NumPy mirror) give the same bits.  Walker i
 * is env i of the batch (desc, state).  It reads env_const[i] and the op table only, as jss_order_eval does; nothing of the batch
 * is written.  Order on a machine, start, makespan, tail, critical, pair and the pairs' listing order, refused and cyclic mean
 * what they mean in jss_order.h.
 *
 * Start.  Walker i is refused (best_makespan[i] = -1) where jss_order_eval would refuse row i of `rank` (no parents, no swaps),
 * and where tenure_of is given and tenure_of[i] is outside [0, 64]; otherwise it is cyclic (-2) where jss_order_eval says so.
 * In both cases the walker's rows of best_rank, last_rank and trace keep what they held and its info row is (-1 or -2, 0, 0, 0).
 * Otherwise the current order is the machines' orders by (rank, j, k); from here on it is held as positions, pos(j,k) being the
 * operation's index on its machine.  cur = best = its makespan, the best order is the current order, the tabu list is empty,
 * moves = best_move = evaluations = 0.  If target is given and best <= target[i]: stop = 2 and the walk ends.
 *
 * Move t = 1 ... iters.  Let (a_k, b_k), k = 0 ... n-1, be ALL the pairs of the current order in jss_order.h's listing order
 * (no cap), and mk_k the makespan of the current order with those two operations exchanged on their machine.
 * evaluations += n.  Neighbour k is usable when mk_k >= 0 (one without a schedule is left out; with durations >= 1 there is
 * none, since reversing a critical arc keeps the graph acyclic).  If none is usable (n = 0 included): stop = 1 and the walk
 * ends -- with positive durations no critical machine arc exists then and the schedule is optimal.
 * Neighbour k is tabu when the unordered pair {a_k, b_k} is the pair of one of this walker's last L moves (t-L ... t-1), L its
 * tenure (tenure_of[i], else tenure); with L = 0 nothing is tabu.  It is admissible when it is usable and either not tabu or
 * mk_k < best (aspiration).  The move taken is the admissible neighbour with the lowest (mk_k, k); if none is admissible, the
 * usable neighbour whose most recent entry in the list is the oldest (entries carry distinct move numbers: no ties).
 * The two operations exchange positions, cur = mk_k, the pair enters the list, moves = t, trace[i][t-1] = cur.  If cur < best:
 * best = cur, the best order becomes the current order, best_move = t.  If target is given and best <= target[i]: stop = 2 and
 * the walk ends.
 *
 * End.  After iters moves: stop = 0.  iters == 0 is a plain evaluation: best = the start, best_rank the normalised rank,
 * stop = 0 or 2.
 *
 * Outputs.  best_makespan[i] = best.  best_rank[i] and last_rank[i] hold the positions of the best and of the current order,
 * -1 in the padding; either one, given to jss_order_eval as rank, reproduces its schedule.  info[i] = (stop, moves, best_move,
 * evaluations).  trace[i] holds cur after every move and -1 behind the last one.
 *
 * One wavefront per walker.  The HIP library holds a walker's op row and sequences in LDS for the whole walk:
 *     12 bytes per entry of a [jmax][mmax] row (the entries rounded up to a multiple of 8) plus 1280
 * -- jss_order.h's formula -- and a batch shape that needs more than 64 KB for one walker is JSS_E_LDS, from both libraries.
 *
 * Errors (checked before anything runs, the same code from both libraries; nothing is written then):
 *   JSS_E_NULL  desc, state, t, t->rank, t->best_makespan or t->best_rank NULL, or what jss_order_eval's desc / state checks
 *               reject;
 *   JSS_E_SHAPE t->iters outside [0, 65536]; t->tenure outside [0, 64] while t->tenure_of is NULL; or a desc / state shape
 *               jss_order_eval rejects;
 *   JSS_E_LDS   see above.
 * desc->batch == 0 launches nothing and returns 0. */
typedef struct JssTabu {
    int32_t iters;              /* moves per walker at most, [0, 65536] */
    int32_t tenure;             /* [0, 64]; used where tenure_of is NULL */
    const int32_t *rank;        /* [B][jmax][mmax] the starting orders, as in jss_order.h */
    const int32_t *tenure_of;   /* [B] or NULL: one tenure per walker */
    const int32_t *target;      /* [B] or NULL: stop once best <= target[i] */
    int32_t *best_makespan;     /* [B] out: best makespan, -1 refused, -2 cyclic start */
    int32_t *best_rank;         /* [B][jmax][mmax] out */
    int32_t *last_rank;         /* [B][jmax][mmax] out or NULL */
    int32_t *info;              /* [B][JSS_TABU_NI] out or NULL */
    int32_t *trace;             /* [B][iters] out or NULL */
} JssTabu;

int jss_tabu_search(const JssDesc *desc, const JssState *state, const JssTabu *t, void *stream);

#ifdef __cplusplus
}
#endif
#endif
