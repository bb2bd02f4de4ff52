/*
 * include/jss_carlier.h -- Carlier's branch and bound for the one-machine problems of partial selections and shifting bottleneck
 * constructions that sequence every machine with it, the thirteenth companion of jss_hip.h (whose JSS_ABI_VERSION it leaves alone,
 * as it leaves every other companion's version, JSS_MACHINE_VERSION included).  libjss_carlier_hip.so
 * (jssenv_amd/csrc/jss_carlier.hip: a library of its own next to the other nine HIP libraries, whose kernels it does not touch)
 * and libjss_cpu.so export the two entry points, with identical semantics; pointers are device pointers for the HIP library and
 * host pointers for the twin, as in jss_hip.h.
 *
 *   jss_machine_solve    <- jss_machine_relax (include/jss_machine.h) with every free machine's one-machine problem SOLVED, within a
 *                           budget of search nodes: the optimum (or the best schedule found), whether it is proved, a bound that is
 *                           never weaker than Jackson's preemptive one, and the best schedule's starts.
 *   jss_bottleneck_exact <- jss_bottleneck_build's loop with the machines sequenced by the search's best schedule instead of
 *                           Schrage's: the shifting bottleneck procedure as Adams, Balas and Zawack state it.
 */
#ifndef JSS_CARLIER_H
#define JSS_CARLIER_H

#include "jss_hip.h"
#include "jss_machine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JSS_CARLIER_VERSION 1

#define JSS_CARLIER_MAX_NODES 4096  /* the largest budget of one one-machine search */
#define JSS_CARLIER_MAX_DEPTH 64    /* the deepest node, the root at depth 1 */
#define JSS_EXACT_NI 8              /* info row: machines fixed, re-sequencings tried, re-sequencings that shortened, first bound,
                                       nodes in total, most nodes of one problem, problems left open, sequences replaced by Schrage's */

/* ---- the one-machine search ------------------------------------------------------------------------------------------------------
 * Integer arithmetic only: both libraries (and jssenv_amd.search.solve_reference, the NumPy mirror) give the same bits, so the
 * tie rules below are part of the definition.
 *
 * The problem is that of jss_machine.h: O_m, the real operations on a free machine m, listed by ascending flat index
 * j * mmax + k, each with r = head, p = d, q = tail of the partial selection.
 *
 * State: working copies of r and q, which the search only raises; best, a value (+infinity at the start) with the starts that
 * gave it; a count of nodes; a flag `open` (0 at the start).  The search is node() at depth 1.
 *
 * node(), at depth D:
 *   1. The node is counted.  Schrage's schedule of the working r and q, by exactly jss_machine.h's rule (t = min r; among the
 *      unscheduled operations with r <= t the largest q, the lowest flat index on ties, starts at s = t; t = s + p, and where
 *      operations remain t = max(t, min r of the rest)), gives starts s and V = max(s + p + q).  If V < best (strictly), best = V
 *      and these starts are kept.
 *   2. With positions in the order Schrage scheduled the operations: b = the lowest position whose s + p + q equals V; a = the
 *      position reached by walking back from b while s[i] == s[i-1] + p[i-1] (the start of the maximal block without idle time);
 *      c = the highest position in [a, b) with q < q[b].  No such c: the node is solved, return.
 *   3. J = the positions c+1 .. b; rJ = min r, qJ = min q, pJ = sum p over J.
 *      If max(rJ + pJ + qJ, min(rJ, r[c]) + pJ + p[c] + min(qJ, q[c])) >= best: return.
 *   4. If this node is node number `nodes` (the caller's budget is spent) or D == JSS_CARLIER_MAX_DEPTH, no child of it could be
 *      entered: open = 1, return, and its children are not looked at.  (So a budget of one node never claims more than Schrage's
 *      schedule and Jackson's bound give.)
 *      Else two children in this order: "c before J", q[c] = max(q[c], pJ + qJ); then "c after J", r[c] = max(r[c], rJ + pJ).
 *      For each: if open is set, nothing more is done (return).  Else the value is set and Jackson's preemptive value of the
 *      modified problem computed.  If that is < best AS IT IS THEN, the child is to be entered: if it would be node number
 *      > nodes it is not entered and open = 1 instead, so that no further node of this problem is entered; else node() at depth
 *      D + 1.  Then the old value is restored.
 *
 * When the search ends r and q are what they were.  Per machine: opt = best; proved = !open; low = opt when proved, else
 * Jackson's preemptive value of the unmodified problem (jps of jss_machine.h); nodes_used = the count; the starts of best.  With
 * nodes == 1 the result is Schrage's schedule itself, and opt == schrage, low == jps of jss_machine_relax.  (A root that ends in step
 * 2 or 3 is solved and its V equals jps: V is then min r + sum p + min q of a set of operations, which jps is never below.)
 *
 * The textbook case: r = 11 14 12 21 31 1 31, p = 5 6 7 4 3 6 2, q = 8 27 25 22 9 18 1.  Schrage gives 55 and Jackson 51; the
 * optimum is 52, found and proved at node 2, with starts 29 19 12 25 34 1 37; with nodes == 1: opt 55, not proved, low 51; with
 * nodes == 2: opt 52 with those starts, not proved, low 51 (node 2 has a c, and the budget's last node may not branch: the proof,
 * both its children closed by Jackson's value, takes nodes >= 3 and still counts 2 nodes).
 *
 * ---- jss_machine_solve ----------------------------------------------------------------------------------------------------------
 * Candidates, parents, rank / stride, fixed, the graph, head, tail, length, the refusals (length[c] = -1), cycles (-2) -- in both
 * cases the candidate's other output rows keep what they held -- are those of jss_machine_relax, word for word.  For every free
 * machine with operations the search above runs with the budget ms->nodes.
 *
 * Outputs, each where given: length[c]; lower_bound[c] = max(length, max_m low); bottleneck[c], the free machine with operations
 * that has the greatest (low, then lowest m), -1 when there is none; opt[c][mmax], low[c][mmax], nodes_used[c][mmax], -1 for fixed
 * machines and machines without operations; proved[c], a 64-bit mask with bit m set where machine m's search ended with open == 0
 * (0 for fixed and unused machines); head[c], tail[c], [jmax][mmax] with -1 in the padding; rank_out[c]: operations on fixed
 * machines keep their rank as read, operations on free machines get the start of their machine's best schedule, -1 in the padding;
 * it must not alias rank.
 *
 * One wavefront per candidate.  The HIP library holds what libjss_machine_hip.so holds (the op row, the rank row, heads, tails, a
 * scratch row, two rows of machine-sorted sequences) and a row of best starts (int32) in LDS, and the undo stack of
 * JSS_CARLIER_MAX_DEPTH entries of three words (the operation and which of r or q; the old value; the value of the second child):
 *     28 bytes per entry of a [jmax][mmax] row (the entries rounded up to a multiple of 8) plus 1024 plus 768
 * and a batch shape that needs more than 64 KB for one candidate (beyond 2272 entries; 100 x 20 and 128 x 17 fit, 128 x 18 does
 * not) is JSS_E_LDS, from both libraries.
 *
 * Errors (checked before anything runs, the same code from both libraries; nothing is written then):
 *   JSS_E_NULL  desc, state, ms or ms->length NULL; ms->rank NULL while ms->fixed is given; ms->rank_out == ms->rank (not NULL);
 *               or what jss_order_eval's desc / state checks reject;
 *   JSS_E_SHAPE ms->n < 0; ms->nodes outside [1, JSS_CARLIER_MAX_NODES]; ms->stride neither 0 nor jmax * mmax; ms->parents == NULL
 *               with ms->n != desc->batch; or a desc / state shape jss_order_eval rejects;
 *   JSS_E_LDS   see above.
 * ms->n == 0 launches nothing and returns 0. */
typedef struct JssMachineSolve {
    int32_t n;                  /* candidates */
    int32_t stride;             /* 0: one rank table for all; jmax * mmax: table c for candidate c */
    int32_t nodes;              /* [1, JSS_CARLIER_MAX_NODES]: the budget of every one-machine search */
    int32_t reserved;           /* not read */
    const int32_t *parents;     /* [n] or NULL: candidate c is env c (n must equal desc->batch) */
    const int32_t *rank;        /* [n][jmax][mmax] or [jmax][mmax]; NULL only with fixed == NULL */
    const uint64_t *fixed;      /* [n] or NULL: nothing fixed */
    int32_t *length;            /* [n] out; -1 refused, -2 cyclic */
    int32_t *lower_bound;       /* [n] out or NULL */
    int32_t *bottleneck;        /* [n] out or NULL */
    int32_t *opt;               /* [n][mmax] out or NULL */
    int32_t *low;               /* [n][mmax] out or NULL */
    int32_t *nodes_used;        /* [n][mmax] out or NULL */
    uint64_t *proved;           /* [n] out or NULL */
    int32_t *head;              /* [n][jmax][mmax] out or NULL */
    int32_t *tail;              /* [n][jmax][mmax] out or NULL */
    int32_t *rank_out;          /* [n][jmax][mmax] out or NULL; must not alias rank */
} JssMachineSolve;

int jss_machine_solve(const JssDesc *desc, const JssState *state, const JssMachineSolve *ms, void *stream);

/* ---- the shifting bottleneck construction, machines sequenced exactly ----------------------------------------------------------
 * jss_bottleneck_build's loop (include/jss_machine.h), word for word: candidates, parents, rank_in / fixed_in, bias, the choice of
 * m* by jps + bias in 64 bits (jps, not the search's bound), the reopt rounds, the `new <= cur` rule, the refusals.  One change:
 *
 *   in steps 2 and 5 the machine's operations get the starts of the SEARCH'S BEST SCHEDULE (budget be->nodes) as ranks.  If the
 *   selection with those ranks is cyclic, they get their Schrage starts instead -- the starts of jss_machine.h's Schrage schedule
 *   of the same relaxation -- and the replacement is counted.  (A machine that repeats within a job can make the best schedule
 *   run against a job arc, which the one-machine problem does not see; Schrage's schedule never reverses a path on positive
 *   durations.)  If that selection is cyclic too, which only durations of 0 allow, step 2 ends the build with -2 and step 5
 *   keeps the machine's old ranks, as today.
 *
 * Outputs: makespan, rank and order as in jss_bottleneck_build; -1 refused, -2 cyclic, and then the candidate's rows of rank, info
 * and order keep what they held.  info[c] (where given), JSS_EXACT_NI entries: machines fixed by this call; re-sequencings tried;
 * re-sequencings that shortened the schedule; lower_bound of the first relaxation as jss_machine_solve gives it with the same
 * budget (max of the length and every free machine's low; those searches are not counted below; they are run only where info is
 * given); the nodes of all searches of steps 2 and 5; the most nodes of one of them; how many of them ended open; how many
 * sequences were replaced by Schrage's.
 *
 * One wavefront per candidate, the same LDS as jss_machine_solve.
 *
 * Errors (before anything runs; nothing is written then):
 *   JSS_E_NULL  desc, state, be, be->makespan or be->rank NULL; exactly one of rank_in / fixed_in; be->rank == be->rank_in (not
 *               NULL); or what jss_order_eval's desc / state checks reject;
 *   JSS_E_SHAPE be->n < 0; be->reopt outside [0, JSS_BOTTLENECK_MAX_REOPT]; be->nodes outside [1, JSS_CARLIER_MAX_NODES];
 *               be->parents == NULL with be->n != desc->batch; or a desc / state shape jss_order_eval rejects;
 *   JSS_E_LDS   as above.
 * be->n == 0 launches nothing and returns 0. */
typedef struct JssBottleneckExact {
    int32_t n;                  /* candidates */
    int32_t reopt;              /* [0, JSS_BOTTLENECK_MAX_REOPT] */
    int32_t nodes;              /* [1, JSS_CARLIER_MAX_NODES] */
    int32_t reserved;           /* not read */
    const int32_t *parents;     /* [n] or NULL: candidate c is env c (n must equal desc->batch) */
    const int32_t *rank_in;     /* [n][jmax][mmax] or NULL (with fixed_in) */
    const uint64_t *fixed_in;   /* [n] or NULL (with rank_in) */
    const int32_t *bias;        /* [n][mmax] or NULL */
    int32_t *makespan;          /* [n] out; -1 refused, -2 cyclic */
    int32_t *rank;              /* [n][jmax][mmax] out; must not alias rank_in */
    int32_t *info;              /* [n][JSS_EXACT_NI] out or NULL */
    int32_t *order;             /* [n][mmax] out or NULL */
} JssBottleneckExact;

int jss_bottleneck_exact(const JssDesc *desc, const JssState *state, const JssBottleneckExact *be, void *stream);

#ifdef __cplusplus
}
#endif
#endif
