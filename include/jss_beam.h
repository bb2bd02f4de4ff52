/*
 * include/jss_beam.h -- beam search's candidate selection, the fifth companion of jss_hip.h (whose JSS_ABI_VERSION it leaves
 * alone).  libjss_beam_hip.so (jssenv_amd/csrc/jss_beam.hip: a library of its own next to libjss_hip.so, whose kernels it does
 * not touch) and libjss_cpu.so export the one entry point, with identical semantics; pointers are device pointers for the
 * HIP library and host pointers for the twin, as in jss_hip.h.
 *
 *   jss_beam_select <- one level of a beam search over a batch: of the candidates jss_lookahead (jss_search.h) has scored,
 *                      keep the W best of every problem, duplicates merged; say which env to clone into which slot
 *                      (jss_clone) and which action to step it by (jss_step)
 */
#ifndef JSS_BEAM_H
#define JSS_BEAM_H

#include "jss_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JSS_BEAM_VERSION 1

/* ---- a segmented, ordered, deduplicating top-W ---------------------------------------------------------------------------
 * A beam is G groups (problems) of W slots each over a batch of S = G * W envs: slot s = g * W + w is env s.  With A = jmax + 1
 * actions, candidate c = s * A + a is "slot s takes action a" -- the parent-major order jss_lookahead is given.  Everything
 * below is integer arithmetic: both libraries give the same bits.
 *
 * Per group g:
 *   slot s is LIVE when cand_parent[s * A] == s, and RUNNING when it is live and done[s] == 0.
 *   A group with no running slot is FINISHED: every slot gets src = -1, action = JSS_ACTION_SKIP, score = -1, its part of
 *   next_parent is a copy of cand_parent and its counts are {0, 0, 0, 0} -- further levels are exact no-ops on it.
 *   VALID candidates of an unfinished group:
 *     a live, done slot s   c = s * A only, with the triple (env_makespan[s], 0, 0) and action JSS_ACTION_SKIP: a finished
 *                           schedule stays in the beam and competes;
 *     a running slot s      every c with makespan[c] >= 0, with the triple (makespan[c], steps[c], reward_num[c]), action a;
 *     a dead slot           none.
 *   ORDER: ascending (makespan, c); width 1 is the pilot method's arg-min, ties to the lowest index.
 *   DEDUPE (flags & JSS_BEAM_DEDUPE): a valid candidate is dropped when a valid candidate of the group with a lower c has an
 *   equal triple.  Equal continuations almost always come from permutations of one partial schedule; the identity is a
 *   heuristic one all the same -- two different states with the same (makespan, steps, return) are merged.
 *   The first W survivors, in order, fill slots g * W, g * W + 1, ...: src = the candidate's slot s (absolute), action and
 *   score = its action and makespan.  Slots left over get -1 / JSS_ACTION_SKIP / -1.  next_parent[d * A + a] = d when
 *   src[d] >= 0, else -1, for every a.
 *   counts[g] = { slots filled, running slots on input, candidates dropped as duplicates ahead of the last slot filled
 *   (all of the group's duplicates when fewer than W survive), valid candidates }.
 *
 * Errors (checked before anything runs, the same code from both libraries; nothing is written then):
 *   JSS_E_NULL  b or any pointer of it NULL;
 *   JSS_E_SHAPE n_groups < 0, width < 1, n_actions < 2, width * n_actions > 65536, or next_parent == cand_parent.
 * n_groups == 0 launches nothing and returns 0. */
#define JSS_BEAM_DEDUPE 1u
typedef struct JssBeam {
    int32_t n_groups, width, n_actions;
    uint32_t flags;
    const int32_t *cand_parent;   /* [S*A] what jss_lookahead was given as parent: s for a live slot, -1 for a dead one */
    const int32_t *makespan;      /* [S*A] jss_lookahead's three outputs */
    const int32_t *steps;
    const int64_t *reward_num;
    const uint8_t *done;          /* [S] the batch's own outputs */
    const int32_t *env_makespan;  /* [S] */
    int32_t *src;                 /* [S]   out: slot to clone into this slot, -1 = leave the env as it is */
    int32_t *action;              /* [S]   out: action to take after the clone, JSS_ACTION_SKIP = none */
    int32_t *score;               /* [S]   out: makespan of the chosen candidate, -1 = none */
    int32_t *next_parent;         /* [S*A] out: the next level's cand_parent; must not alias cand_parent */
    int32_t *counts;              /* [G][4] out: selected, running slots on input, duplicates dropped, valid candidates */
} JssBeam;

int jss_beam_select(const JssBeam *b, void *stream);

#ifdef __cplusplus
}
#endif
#endif
