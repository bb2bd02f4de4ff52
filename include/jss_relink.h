/*
 * include/jss_relink.h -- path relinking between machine orders, the tenth companion of jss_hip.h (whose JSS_ABI_VERSION it
 * leaves alone, as it leaves JSS_ORDER_VERSION, JSS_TABU_VERSION and JSS_BLOCK_VERSION).  libjss_relink_hip.so
 * (jssenv_amd/csrc/jss_relink.hip: a library of its own next to libjss_hip.so, libjss_beam_hip.so, libjss_bound_hip.so,
 * libjss_order_hip.so, libjss_tabu_hip.so and libjss_block_hip.so, whose kernels it does not touch) and libjss_cpu.so export the
 * entry point, with identical semantics; pointers are device pointers for the HIP library and host pointers for the twin, as in
 * jss_hip.h.
 *
 *   jss_relink_walk <- per env the distance between two machine orders and a walk from the one (the source) towards the other
 *                      (the guide) in one launch: every move swaps two operations that are adjacent on a machine and that the
 *                      guide has the other way round, so every move lowers the distance by one and every order on the way has a
 *                      schedule.  The candidates are scored from the heads and tails of the current schedule as in jss_block.h,
 *                      and only the move taken is re-timed exactly.
 */
#ifndef JSS_RELINK_H
#define JSS_RELINK_H

#include "jss_block.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JSS_RELINK_VERSION 1

#define JSS_RELINK_NI 8     /* info row: stop, moves, best_move, dist0, dist, candidates, fallbacks, retries */

/* ---- the walk ------------------------------------------------------------------------------------------------------------------
 * Integer arithmetic only: both libraries (and jssenv_amd.search.relink_reference, the NumPy mirror) give the same bits.  Walker i
 * is env i of the batch (desc, state).  It reads env_const[i] and the op table only; nothing of the batch is written.  Order on a
 * machine, start, tail, makespan, refused and cyclic mean what they mean in jss_order.h.  The notation st, d, tl, E, Q, JP, JS,
 * MP, MS is jss_block.h's, for the exact schedule of the current order; E, Q, st and tl of a missing neighbour are 0.
 *
 * Start.  Walker i is refused (best_makespan[i] = -1) where jss_order_eval would refuse row i of `rank` or row i of `guide`, and
 * where until_of is given and until_of[i] < 0; otherwise it is cyclic (-2) where jss_order_eval says so of either row (the source
 * is looked at first; the code is the same).  In both cases the walker's rows of best_rank, last_rank, trace and move_log keep
 * what they held, last_makespan[i] takes the same code and its info row is (-1 or -2, 0, ..., 0).  Otherwise the current order
 * is the machines' orders by (rank, j, k) and the guide order the machines' orders by (guide, j, k), both held as positions from
 * here on; g(e) is e's position on its machine in the guide order.  cur = the current order's makespan, moves = 0.
 *
 * Distance.  dist is the number of unordered pairs of operations of one machine that the current order and the guide order put
 * the other way round, summed over the machines; dist0 its value at the start.  A swap of two operations u, v adjacent in the
 * current order (u before v) with g(u) > g(v) lowers it by exactly 1, and while dist > 0 some machine has such a pair.
 *
 * Stop checks, at the start and after every move, in this order: dist == 0: stop = 1, arrived; dist <= until (until_of[i] where
 * until_of is given): stop = 2; moves == steps: stop = 0.  steps == 0 is therefore a plain evaluation that also gives the
 * distance.
 *
 * Move t = 1 ... steps.
 *   Candidates, in listing order (machines ascending, positions ascending): every position `at` of a machine whose operations
 *   u at `at` and v at `at` + 1 have g(u) > g(v).  candidates += their number.  (Two operations of one job are never a candidate:
 *   both orders have schedules, so both keep them in job order.)
 *   Screen.  With s = JS(u) and p = JP(v), a candidate is sure when u has no job successor, or v has no job predecessor, or
 *   s != p and st(p) < st(s) + d(s).  (A path from u to v other than the arc itself leaves u through s and enters v through p:
 *   it forces s == p or st(p) >= E(s), durations of 0 included.  A sure swap closes no cycle.)
 *   Estimate, jss_block.h's for a move of distance 1:
 *     h(v) = max(E(JP(v)), E(MP(u)))        h(u) = max(E(JP(u)), h(v) + d(v))
 *     T(u) = d(u) + max(Q(JS(u)), Q(MS(v)))  T(v) = d(v) + max(Q(JS(v)), T(u))
 *     est  = max(h(v) + T(v), h(u) + T(u))
 *   Choice.  The sure candidate with the lowest (est, listing order).  If none is sure: fallbacks += 1, and the candidates are
 *   tried in ascending (est, listing order): each is swapped and re-timed; one that has no schedule is swapped back with
 *   retries += 1; the first that has a schedule is the move.  If none has, the walk ends with stop = 4 and nothing of move t
 *   recorded.  That is unreachable: let len(u, v) be the longest path from u to v in the current graph.  Among the inverted
 *   adjacent pairs take one with the smallest len.  A second path from u to v must contain a machine arc that runs backwards in a
 *   topological order of the guide, since job arcs never do; the machine stretch under that arc holds an inverted adjacent pair
 *   with a strictly shorter len.  So the pair has len = 1: the arc is the only path, and its swap keeps a schedule.
 *   The move.  u and v change places and the order is re-timed exactly, once (that forward pass is the next move's too):
 *   cur = that makespan, moves = t, dist -= 1, trace[i][t-1] = cur, move_log[i][t-1] = (u, v) as flat indices.
 *
 * Best.  The order after move t (t = 0: the source) is eligible when t >= margin and its dist >= margin.  best is the lowest
 * makespan among the eligible orders, at its first occurrence; best_move its t; best_rank its order.  If no order was eligible:
 * best_makespan[i] = cur at the end, best_rank[i] the last order, best_move = -1.
 *
 * Outputs.  best_makespan[i], best_rank[i] as above; last_makespan[i] and last_rank[i] the makespan and the order at the end;
 * info[i] = (stop, moves, best_move, dist0, dist, candidates, fallbacks, retries).  Ranks are positions, -1 in the padding.
 * trace[i] and move_log[i] hold -1 behind the last move.
 *
 * One wavefront per walker.  The HIP library holds a walker's op row, starts, tails, sequence, scratch row and guide positions
 * in LDS for the whole walk:
 *     18 bytes per entry of a [jmax][mmax] row (the entries rounded up to a multiple of 8) plus 1024
 * -- three int32 rows and three uint16 rows, and four 64-word blocks -- and a batch shape that needs more than 64 KB for one
 * walker (beyond 3584 entries; 100 x 20 and 128 x 28 fit, 128 x 29 does not) is JSS_E_LDS, from both libraries.
 *
 * Errors (checked before anything runs, the same code from both libraries; nothing is written then):
 *   JSS_E_NULL  desc, state, r, r->rank, r->guide, r->best_makespan or r->best_rank NULL, or what jss_order_eval's desc / state
 *               checks reject;
 *   JSS_E_SHAPE r->steps outside [0, 65536]; r->until < 0; r->margin < 0; or a desc / state shape jss_order_eval rejects;
 *   JSS_E_LDS   see above.
 * desc->batch == 0 launches nothing and returns 0. */
typedef struct JssRelink {
    int32_t steps;              /* moves per walker at most, [0, 65536] */
    int32_t until;              /* >= 0; used where until_of is NULL: stop once the distance is <= until */
    int32_t margin;             /* >= 0: orders nearer than this to either end are not eligible as the best */
    const int32_t *rank;        /* [B][jmax][mmax] the sources, as in jss_order.h */
    const int32_t *guide;       /* [B][jmax][mmax] the guides, read the same way */
    const int32_t *until_of;    /* [B] or NULL */
    int32_t *best_makespan;     /* [B] out; -1 refused, -2 cyclic */
    int32_t *best_rank;         /* [B][jmax][mmax] out */
    int32_t *last_makespan;     /* [B] out or NULL */
    int32_t *last_rank;         /* [B][jmax][mmax] out or NULL */
    int32_t *info;              /* [B][JSS_RELINK_NI] out or NULL */
    int32_t *trace;             /* [B][steps] out or NULL */
    int32_t *move_log;          /* [B][steps][2] out or NULL */
} JssRelink;

int jss_relink_walk(const JssDesc *desc, const JssState *state, const JssRelink *r, void *stream);

#ifdef __cplusplus
}
#endif
#endif
