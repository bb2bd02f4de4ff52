// jssenv_amd/csrc/jss_abi_checks.hpp -- the argument checks of the C ABI (include/jss_hip.h), the one piece of code that
// libjss_hip.so (jss_kernels.hip) and its host-core twin libjss_cpu.so (jss_cpu.cpp) share.  Every entry point of both
// libraries starts with the check_<entry point> below and does nothing else before it: an argument error gets the same
// code from either library, and it touches nothing -- a multi-set call checks every set before it runs any.  What stays
// with each library is what depends on it: JSS_E_LDS (the HIP library's launch plan), JSS_E_RESIDENT and the session
// registry's JSS_E_SESSION answers.  A check reads only its arguments: the structs and pointer arrays passed by address,
// never the buffers they describe.  Plain C++17, no HIP.
#pragma once

#include <cstdint>

#include "jss_hip.h"
#include "jss_search.h"
#include "jss_rules.h"
#include "jss_keys.h"
#include "jss_beam.h"
#include "jss_bound.h"
#include "jss_order.h"
#include "jss_tabu.h"
#include "jss_block.h"
#include "jss_relink.h"
#include "jss_decode.h"
#include "jss_machine.h"
#include "jss_carlier.h"
#include "jss_propagate.h"

namespace jss_abi {

// ---- building blocks ----------------------------------------------------------------------------------------------
// One env set's JssDesc / JssState / JssOut; need_out: the call writes `out` (all but jss_policy)
inline int check_args(const JssDesc *d, const JssState *s, const JssOut *o, bool need_out) {
    if (!d || !s) return JSS_E_NULL;
    if (!d->ops || !d->inst) return JSS_E_NULL;
    if (!s->env || !s->env_const || !s->job || !s->solution) return JSS_E_NULL;
    if (!s->machine && d->record_ints != JSS_NFC && d->record_ints != JSS_NFM) return JSS_E_NULL;   // compact / medium batches keep no machine clocks
    if (need_out && (!o || !o->real_obs || !o->action_mask || !o->reward || !o->done || !o->makespan)) return JSS_E_NULL;
    if (d->batch < 0 || d->jmax < 1 || d->jmax > JSS_MAX_JOBS || d->mmax < 2 || d->mmax > JSS_MAX_MACHINES ||
        d->n_tables < 1)
        return JSS_E_SHAPE;
    if (!d->table_of_env && d->n_tables != 1 && d->n_tables != d->batch) return JSS_E_SHAPE;
    if (d->kernel & ~(JSS_KERNEL_WAVE | JSS_KERNEL_ONE_ENV_PER_WAVE | JSS_KERNEL_TWO_ENVS_PER_WAVE)) return JSS_E_KIND;
    if (d->record_ints != 0 && d->record_ints != JSS_NF && d->record_ints != JSS_NFC && d->record_ints != JSS_NFM) return JSS_E_SHAPE;
    if (d->record_ints == JSS_NFC && d->n_tables != 1) return JSS_E_SHAPE;   // compact records need the ONE table in LDS
    // medium records: 21-bit ops (machines <= 32, whatever the number of jobs), per-env tables
    if (d->record_ints == JSS_NFM && (d->mmax > 32 || d->n_tables == 1)) return JSS_E_SHAPE;
    return 0;
}

// ints per job record of a batch that passed check_args
inline int record_ints_of(const JssDesc &d) { return d.record_ints == JSS_NFC ? JSS_NFC : d.record_ints == JSS_NFM ? JSS_NFM : JSS_NF; }

// f64_ok: the call's policy is a launch of its own (the kernels that carry JSS_POLICY_CR_F64's float64 selector)
inline int check_kind(const JssDesc *d, int kind_arg, bool f64_ok = false) {
    const int kind = kind_arg & 0xFF, fp = (kind_arg >> 8) & 0xFF, fq = (kind_arg >> 16) & 0xFF;
    if (kind_arg < 0 || (kind_arg >> 25) || kind >= JSS_N_POLICIES) return JSS_E_KIND;
    if ((kind_arg >> 24) & 1) {                      // JSS_POLICY_CR_F64: the factor is JssDesc.cr_factor
        if (!f64_ok || kind != JSS_POLICY_CR || fp || fq || !(d->cr_factor > 0.0) || !(d->cr_factor < 1e300)) return JSS_E_KIND;
    }
    if (fp || fq) {                                  // a due-date factor p / q: CriticalRatio only, q a power of two <= 64
        if (kind != JSS_POLICY_CR || fp < 1 || fq < 1 || fq > 64 || (fq & (fq - 1))) return JSS_E_KIND;
    }
    if ((kind == JSS_POLICY_MWR || kind == JSS_POLICY_LWR || kind == JSS_POLICY_CR) && !d->rem) return JSS_E_NULL;
    return 0;
}

// a JssRule, where its call's namesake checks `kind`: the selector reads the remaining-work table whatever the weights are
inline int check_rule(const JssDesc *d, const JssRule *rule) {
    if (!rule || !rule->weights || !d->rem) return JSS_E_NULL;
    if (reinterpret_cast<uintptr_t>(rule->weights) & 15) return JSS_E_SHAPE;      // rows are read four weights at a time
    return rule->stride == 0 || rule->stride == JSS_RW_N ? 0 : JSS_E_SHAPE;
}

// a JssKeys, where its call's namesake checks `kind` (the selector reads no table of the batch's own: JssDesc.rem may be NULL)
inline int check_keys(const JssDesc *d, const JssKeys *keys) {
    if (!keys || !keys->keys) return JSS_E_NULL;
    return keys->stride == 0 || keys->stride == d->jmax * d->mmax ? 0 : JSS_E_SHAPE;
}

// What picks the actions of a jss_policy / jss_rollout / jss_lookahead call and of their jss_rule_* (include/jss_rules.h) and
// jss_key_* (include/jss_keys.h) namesakes: a stock rule's `kind`, the caller's weight rows or the caller's key tables.  The
// three are one call each, checked, planned and launched by one path in either library.
struct SelectorArg {
    enum Which { kStock, kRule, kKeys } which;
    int kind;                // kStock
    const JssRule *rule;     // kRule (may be NULL: check_rule says so)
    const JssKeys *keys;     // kKeys (likewise)
};
inline SelectorArg stock_selector(int kind) { return {SelectorArg::kStock, kind, nullptr, nullptr}; }
inline SelectorArg rule_selector(const JssRule *rule) { return {SelectorArg::kRule, 0, rule, nullptr}; }
inline SelectorArg keys_selector(const JssKeys *keys) { return {SelectorArg::kKeys, 0, nullptr, keys}; }

// f64_ok: as for check_kind (the caller's selectors have no such form)
inline int check_selector(const JssDesc *d, const SelectorArg &sel, bool f64_ok = false) {
    return sel.which == SelectorArg::kRule ? check_rule(d, sel.rule) : sel.which == SelectorArg::kKeys ? check_keys(d, sel.keys)
                                                                                                      : check_kind(d, sel.kind, f64_ok);
}

// a JssLogits against its set's description
inline int check_logits(const JssDesc *d, const JssLogits *lg) {
    if (!lg || !lg->logits || !lg->action) return JSS_E_NULL;
    if (lg->row != 0 && lg->row < (int64_t)d->jmax + 1) return JSS_E_SHAPE;
    if (lg->row > (1 << 24)) return JSS_E_SHAPE;                         // (lane offsets are 32-bit)
    if (lg->dtype != JSS_LOGITS_F32 && lg->dtype != JSS_LOGITS_BF16) return JSS_E_KIND;
    if (!(lg->temperature >= 0.f)) return JSS_E_KIND;                    // < 0 or NaN
    return 0;
}

// the sets of a jss_multi_* call: the arrays, their count, then check_args of every set
inline int check_multi(int32_t n_sets, const JssDesc *const *descs, const JssState *const *states, const JssOut *const *outs,
                       bool need_out) {
    if (!descs || !states || (need_out && !outs)) return JSS_E_NULL;
    if (n_sets < 1 || n_sets > 16) return JSS_E_SHAPE;
    for (int i = 0; i < n_sets; ++i) {
        const int rc = check_args(descs[i], states[i], need_out ? outs[i] : nullptr, need_out);
        if (rc) return rc;
    }
    return 0;
}

// jss_clone's table kind of a batch: 0 one shared table, 1 table_of_env, 2 one table per env, 3 one env on one table (either
// of 0 and 2)
inline int clone_table_kind(const JssDesc *d) {
    if (d->table_of_env) return 1;
    if (d->n_tables == 1) return d->batch == 1 ? 3 : 0;
    return 2;                                                              // n_tables == batch (check_args)
}

// ---- one check per entry point, or per group of entry points that take the same arguments --------------------------
// A multi-step call with n_steps == 0 does nothing: once its check has passed, the entry point returns 0 without
// launching or running anything.

// jss_reset, jss_advance
inline int check_reset(const JssDesc *d, const JssState *s, const JssOut *o) { return check_args(d, s, o, true); }

// jss_step, jss_step_autoreset
inline int check_step(const JssDesc *d, const JssState *s, const int32_t *actions, const JssOut *o) {
    const int rc = check_args(d, s, o, true);
    if (rc) return rc;
    return actions ? 0 : JSS_E_NULL;
}

inline int check_step_logits(const JssDesc *d, const JssState *s, const JssLogits *lg, const JssOut *o) {
    const int rc = check_args(d, s, o, true);
    return rc ? rc : check_logits(d, lg);
}

// jss_policy, jss_rule_policy, jss_key_policy
inline int check_policy(const JssDesc *d, const JssState *s, const SelectorArg &sel, const int32_t *actions) {
    const int rc = check_args(d, s, nullptr, false);
    if (rc) return rc;
    if (!actions) return JSS_E_NULL;
    return check_selector(d, sel, true);
}

// jss_rollout, jss_rule_rollout, jss_key_rollout
inline int check_rollout(const JssDesc *d, const JssState *s, const JssOut *o, const SelectorArg &sel, int32_t n_iter) {
    int rc = check_args(d, s, o, true);
    if (rc) return rc;
    if ((rc = check_selector(d, sel))) return rc;
    return n_iter < 0 ? JSS_E_SHAPE : 0;
}

inline int check_trajectory(const JssDesc *d, const JssState *s, const JssOut *o, const JssTraj *traj, int kind, int32_t n_steps) {
    int rc = check_args(d, s, o, true);
    if (rc) return rc;
    if (!traj) return JSS_E_NULL;
    if ((rc = check_kind(d, kind))) return rc;
    return n_steps < 0 ? JSS_E_SHAPE : 0;
}

// (n_steps == 0: `actions` is not looked at -- an empty action buffer has no address)
inline int check_steps(const JssDesc *d, const JssState *s, const JssOut *o, const int32_t *actions, int32_t n_steps) {
    const int rc = check_args(d, s, o, true);
    if (rc) return rc;
    if (n_steps < 0) return JSS_E_SHAPE;
    if (n_steps == 0) return 0;
    return actions ? 0 : JSS_E_NULL;
}

inline int check_rollout_steps(const JssDesc *d, const JssState *s, const JssOut *o, int kind, int32_t n_steps, int32_t n_sub,
                               void *const *streams) {
    int rc = check_args(d, s, o, true);
    if (rc) return rc;
    if ((rc = check_kind(d, kind))) return rc;
    if (n_steps < 0 || n_sub < 1 || n_sub > 16) return JSS_E_SHAPE;
    return streams ? 0 : JSS_E_NULL;
}

inline int check_policy_step_steps(const JssDesc *d, const JssState *s, const JssOut *o, int kind, const int32_t *actions,
                                   int32_t n_steps, int32_t n_sub, void *const *streams) {
    int rc = check_args(d, s, o, true);
    if (rc) return rc;
    if ((rc = check_kind(d, kind, true))) return rc;
    if (n_steps < 0 || n_sub < 1 || n_sub > 16) return JSS_E_SHAPE;
    return streams && actions ? 0 : JSS_E_NULL;
}

// ---- the step session: the pure-argument part (the registry of open sessions is each library's own) ----------------
inline int check_session_open(const JssDesc *d, const JssState *s, const JssOut *o, const JssSession *session) {
    const int rc = check_args(d, s, o, true);
    if (rc) return rc;
    if (!session || !session->mail || !session->progress || !session->status) return JSS_E_NULL;
    if (session->depth < 1 || session->timeout_ms < 0 || d->batch < 1) return JSS_E_SHAPE;
    const int want = session->slots;
    if (want != 0 && want != 1 && want != 2 && want != 4 && want != 8) return JSS_E_SHAPE;
    return 0;
}

inline int check_session_post(const JssDesc *d, const JssSession *session, const int32_t *actions, int32_t first_step,
                              int32_t n_steps, int32_t waited) {
    if (!d || !session || !session->mail || !actions) return JSS_E_NULL;
    if (first_step < 0 || n_steps < 1 || waited < 0 || waited > first_step || first_step + n_steps - waited > session->depth)
        return JSS_E_SESSION;
    return 0;
}

inline int check_session_wait(const JssDesc *d, const JssSession *session, int32_t steps_done) {
    if (!d || !session || !session->progress || !session->status) return JSS_E_NULL;
    return steps_done < 0 ? JSS_E_SESSION : 0;
}

inline int check_session_step(const JssDesc *d, const JssSession *session, const int32_t *actions, int32_t step) {
    if (!d || !session || !session->mail || !session->progress || !session->status || !actions) return JSS_E_NULL;
    return step < 0 ? JSS_E_SESSION : 0;
}

inline int check_session_close(const JssDesc *d, const JssSession *session, int32_t next_step) {
    if (!d || !session || !session->mail) return JSS_E_NULL;
    return next_step < 0 ? JSS_E_SESSION : 0;
}

// ---- several env sets per call: every set is checked before any set is touched --------------------------------------
inline int check_multi_reset(int32_t n_sets, const JssDesc *const *descs, const JssState *const *states, const JssOut *const *outs) {
    return check_multi(n_sets, descs, states, outs, true);
}

inline int check_multi_step(int32_t n_sets, const JssDesc *const *descs, const JssState *const *states,
                            const int32_t *const *actions, const JssOut *const *outs) {
    const int rc = check_multi(n_sets, descs, states, outs, true);
    if (rc) return rc;
    if (!actions) return JSS_E_NULL;
    for (int i = 0; i < n_sets; ++i)
        if (!actions[i]) return JSS_E_NULL;
    return 0;
}

// (every set's description first, then every set's logits)
inline int check_multi_step_logits(int32_t n_sets, const JssDesc *const *descs, const JssState *const *states,
                                   const JssLogits *const *lgs, const JssOut *const *outs) {
    if (!lgs) return JSS_E_NULL;
    int rc = check_multi(n_sets, descs, states, outs, true);
    for (int i = 0; i < n_sets && !rc; ++i) rc = check_logits(descs[i], lgs[i]);
    return rc;
}

inline int check_multi_policy(int32_t n_sets, const JssDesc *const *descs, const JssState *const *states, int kind,
                              int32_t *const *actions) {
    int rc = check_multi(n_sets, descs, states, nullptr, false);
    if (rc) return rc;
    if (!actions) return JSS_E_NULL;
    for (int i = 0; i < n_sets; ++i) {
        if (!actions[i]) return JSS_E_NULL;
        if ((rc = check_kind(descs[i], kind, true))) return rc;
    }
    return 0;
}

inline int check_multi_rollout(int32_t n_sets, const JssDesc *const *descs, const JssState *const *states,
                               const JssOut *const *outs, int kind, int32_t n_steps, int32_t n_sub, void *const *streams) {
    int rc = check_multi(n_sets, descs, states, outs, true);
    if (rc) return rc;
    if (n_steps < 0 || n_sub < 1 || n_sub > 16) return JSS_E_SHAPE;
    if (!streams) return JSS_E_NULL;
    for (int i = 0; i < n_sets && !rc; ++i) rc = check_kind(descs[i], kind);
    return rc;
}

// (set by set: its description, then the kind against it)
inline int check_rollout_steps_multi(int32_t n_sets, const JssDesc *const *descs, const JssState *const *states,
                                     const JssOut *const *outs, int kind, int32_t n_steps, void *const *streams) {
    if (!descs || !states || !outs || !streams) return JSS_E_NULL;
    if (n_sets < 1 || n_sets > 16 || n_steps < 0) return JSS_E_SHAPE;
    for (int i = 0; i < n_sets; ++i) {
        int rc = check_args(descs[i], states[i], outs[i], true);
        if (!rc) rc = check_kind(descs[i], kind);
        if (rc) return rc;
    }
    return 0;
}

// ---- instances and clones -----------------------------------------------------------------------------------------
inline int check_generate(const JssDesc *d, const JssState *s, const JssGen *g) {
    if (!d || !g || !g->ops || !g->rem || !g->inst) return JSS_E_NULL;
    if (!g->time_seed != !g->machine_seed) return JSS_E_NULL;                 // both seed arrays or neither
    if (!g->time_seed && (!s || !s->env)) return JSS_E_NULL;                  // derived seeds read the episode
    if (d->batch < 0 || d->jmax < 1 || d->jmax > JSS_MAX_JOBS || d->mmax < 1 || d->mmax > JSS_MAX_MACHINES) return JSS_E_SHAPE;
    if (d->n_tables != d->batch || d->table_of_env) return JSS_E_SHAPE;        // table i is env i's alone
    if (g->jobs < 1 || g->jobs > d->jmax || g->machines < 1 || g->machines > d->mmax) return JSS_E_SHAPE;
    if (g->dur_low < 1 || g->dur_low > g->dur_high || g->dur_high > 0xFFFF) return JSS_E_SHAPE;
    return 0;
}

// *mode: what of the instance assignment is copied -- 0 nothing (the shared table), 1 the table_of_env entry, 2 the env's
// own op / work / instance table rows
inline int check_clone(const JssDesc *dd, const JssState *ds, const JssOut *dout, const JssCloneDst *dt, const JssDesc *sd,
                       const JssState *ss, const JssOut *sout, const int32_t *src_of_dst, int *mode) {
    if (!src_of_dst) return JSS_E_NULL;
    int rc = check_args(dd, ds, dout, true);
    if (!rc) rc = check_args(sd, ss, sout, true);
    if (rc) return rc;
    if (dd->jmax != sd->jmax || dd->mmax != sd->mmax || record_ints_of(*dd) != record_ints_of(*sd)) return JSS_E_SHAPE;
    const int a = clone_table_kind(dd), b = clone_table_kind(sd);
    if (a == 1 || b == 1) {
        if (a != b || dd->n_tables != sd->n_tables) return JSS_E_SHAPE;
        *mode = 1;
    } else if (a == 0 || b == 0) {
        if (a == 2 || b == 2) return JSS_E_SHAPE;                           // (both have the one table)
        *mode = 0;
    } else {
        *mode = 2;
    }
    if (*mode == 1 && (!dt || !dt->table_of_env)) return JSS_E_SHAPE;
    if (*mode == 2 && (!dt || !dt->ops || !dt->rem || !dt->inst)) return JSS_E_SHAPE;
    if (*mode == 2 && !sd->rem) return JSS_E_NULL;
    return 0;
}

// ---- search (include/jss_search.h) ---------------------------------------------------------------------------------
// jss_lookahead, jss_rule_lookahead, jss_key_lookahead: the batch as jss_rollout checks it, without a JssOut (nothing of the
// batch is written); the fused rollouts' kinds (no JSS_POLICY_CR_F64)
inline int check_lookahead(const JssDesc *d, const JssState *s, const JssLookahead *la, const SelectorArg &sel, int32_t n_iter) {
    if (!d || !s || !la) return JSS_E_NULL;
    int rc = check_args(d, s, nullptr, false);
    if (rc) return rc;
    if (!la->parent || !la->action || !la->makespan) return JSS_E_NULL;
    if (la->n < 0 || n_iter < 0) return JSS_E_SHAPE;
    return check_selector(d, sel);
}

// ---- beam search (include/jss_beam.h) ------------------------------------------------------------------------------
// jss_beam_select (libjss_beam_hip.so and the twin): width * n_actions <= 65536 -- a candidate's index within its group is half
// of a 64-bit sort key, and one workgroup serves a group
inline int check_beam_select(const JssBeam *b) {
    if (!b) return JSS_E_NULL;
    if (!b->cand_parent || !b->makespan || !b->steps || !b->reward_num || !b->done || !b->env_makespan || !b->src ||
        !b->action || !b->score || !b->next_parent || !b->counts)
        return JSS_E_NULL;
    if (b->n_groups < 0 || b->width < 1 || b->n_actions < 2 || (int64_t)b->width * b->n_actions > 65536) return JSS_E_SHAPE;
    return b->next_parent == b->cand_parent ? JSS_E_SHAPE : 0;
}

// ---- lower bounds (include/jss_bound.h) ----------------------------------------------------------------------------
// jss_bound (libjss_bound_hip.so and the twin): the batch as jss_lookahead checks it, and the work table, which the bound reads
inline int check_bound(const JssDesc *d, const JssState *s, const JssBound *b) {
    if (!d || !s || !b) return JSS_E_NULL;
    const int rc = check_args(d, s, nullptr, false);
    if (rc) return rc;
    if (!d->rem || !b->lower_bound) return JSS_E_NULL;
    if (b->n < 0 || (!b->parent && b->n != d->batch)) return JSS_E_SHAPE;
    return 0;
}

// ---- machine orders (include/jss_order.h) ----------------------------------------------------------------------------
// What libjss_order_hip.so keeps in LDS for one candidate: the op row and the start / tail row (int32), the machines' sequences
// and the pair marks (uint16) over the entries of a [jmax][mmax] row rounded up to a multiple of 8, and five 64-word blocks.
constexpr long long kOrderLdsLimit = 64 * 1024;
inline long long order_entries8(int jmax, int mmax) { return ((long long)jmax * mmax + 7) / 8 * 8; }
inline long long order_lds_bytes(int jmax, int mmax) { return 12 * order_entries8(jmax, mmax) + 5 * 64 * 4; }

// jss_order_eval (libjss_order_hip.so and the twin): the batch as jss_lookahead checks it
inline int check_order_eval(const JssDesc *d, const JssState *s, const JssOrder *o) {
    if (!d || !s || !o) return JSS_E_NULL;
    const int rc = check_args(d, s, nullptr, false);
    if (rc) return rc;
    if (!o->rank || !o->makespan) return JSS_E_NULL;
    if (o->n < 0 || (!o->parent && o->n != d->batch)) return JSS_E_SHAPE;
    if (!o->swap_a != !o->swap_b) return JSS_E_SHAPE;
    const int pairs = (o->pair_a != nullptr) + (o->pair_b != nullptr) + (o->n_pairs != nullptr);
    if ((pairs != 0 && pairs != 3) || (pairs == 3 && o->pair_cap < 1)) return JSS_E_SHAPE;
    return order_lds_bytes(d->jmax, d->mmax) > kOrderLdsLimit ? JSS_E_LDS : 0;
}

inline int check_order_apply(const JssOrderApply *a) {
    if (!a || !a->rank || !a->cur || !a->makespan || !a->pair_a || !a->pair_b || !a->improved) return JSS_E_NULL;
    if (a->batch < 0 || a->jmax < 1 || a->jmax > JSS_MAX_JOBS || a->mmax < 1 || a->mmax > JSS_MAX_MACHINES || a->pair_cap < 1)
        return JSS_E_SHAPE;
    return 0;
}

// ---- tabu search (include/jss_tabu.h) --------------------------------------------------------------------------------
// What libjss_tabu_hip.so keeps in LDS for one walker, for the whole walk: the same rows as one candidate of jss_order_eval.
inline long long tabu_lds_bytes(int jmax, int mmax) { return order_lds_bytes(jmax, mmax); }

// jss_tabu_search (libjss_tabu_hip.so and the twin): the batch as jss_order_eval checks it
inline int check_tabu_search(const JssDesc *d, const JssState *s, const JssTabu *t) {
    if (!d || !s || !t) return JSS_E_NULL;
    const int rc = check_args(d, s, nullptr, false);
    if (rc) return rc;
    if (!t->rank || !t->best_makespan || !t->best_rank) return JSS_E_NULL;
    if (t->iters < 0 || t->iters > 65536) return JSS_E_SHAPE;
    if (!t->tenure_of && (t->tenure < 0 || t->tenure > 64)) return JSS_E_SHAPE;
    return tabu_lds_bytes(d->jmax, d->mmax) > kOrderLdsLimit ? JSS_E_LDS : 0;
}

// ---- block insertions (include/jss_block.h) ----------------------------------------------------------------------------
// What libjss_block_hip.so keeps in LDS for one walker, for the whole walk: jss_order_eval's rows, and over the same entries
// the tails (int32) and the list of the marked positions (uint16).
inline long long block_lds_bytes(int jmax, int mmax) { return 18 * order_entries8(jmax, mmax) + 5 * 64 * 4; }

// jss_block_search (libjss_block_hip.so and the twin): the batch as jss_order_eval checks it
inline int check_block_search(const JssDesc *d, const JssState *s, const JssBlock *b) {
    if (!d || !s || !b) return JSS_E_NULL;
    const int rc = check_args(d, s, nullptr, false);
    if (rc) return rc;
    if (!b->rank || !b->best_makespan || !b->best_rank) return JSS_E_NULL;
    if (b->iters < 0 || b->iters > 65536) return JSS_E_SHAPE;
    if (!b->tenure_of && (b->tenure < 0 || b->tenure > 64)) return JSS_E_SHAPE;
    if (b->reach < 0 || b->reach > 65535) return JSS_E_SHAPE;
    return block_lds_bytes(d->jmax, d->mmax) > kOrderLdsLimit ? JSS_E_LDS : 0;
}

// ---- path relinking (include/jss_relink.h) -------------------------------------------------------------------------------
// What libjss_relink_hip.so keeps in LDS for one walker, for the whole walk: jss_order_eval's rows (with four blocks of one
// word per machine), and over the same entries the tails (int32) and the guide positions (uint16).
inline long long relink_lds_bytes(int jmax, int mmax) { return 18 * order_entries8(jmax, mmax) + 4 * 64 * 4; }

// jss_relink_walk (libjss_relink_hip.so and the twin): the batch as jss_order_eval checks it
inline int relink_check(const JssDesc *d, const JssState *s, const JssRelink *r) {
    if (!d || !s || !r) return JSS_E_NULL;
    const int rc = check_args(d, s, nullptr, false);
    if (rc) return rc;
    if (!r->rank || !r->guide || !r->best_makespan || !r->best_rank) return JSS_E_NULL;
    if (r->steps < 0 || r->steps > 65536) return JSS_E_SHAPE;
    if (r->until < 0 || r->margin < 0) return JSS_E_SHAPE;
    return relink_lds_bytes(d->jmax, d->mmax) > kOrderLdsLimit ? JSS_E_LDS : 0;
}

// ---- Giffler-Thompson decoding of key tables, one BRKGA generation (include/jss_decode.h) ------------------------------------
// What libjss_decode_hip.so keeps in LDS for one candidate, for the whole decode: the op row and the key row (int32) over the
// entries of a [jmax][mmax] row rounded up to a multiple of 8, and one word per machine.
inline long long decode_lds_bytes(int jmax, int mmax) { return 8 * order_entries8(jmax, mmax) + 64 * 4; }

// jss_decode_keys (libjss_decode_hip.so and the twin): the batch as jss_order_eval checks it
inline int decode_check(const JssDesc *d, const JssState *s, const JssDecode *k) {
    if (!d || !s || !k) return JSS_E_NULL;
    const int rc = check_args(d, s, nullptr, false);
    if (rc) return rc;
    if (!k->keys || !k->makespan) return JSS_E_NULL;
    if (k->n < 0 || (!k->parents && k->n != d->batch)) return JSS_E_SHAPE;
    if (k->stride != 0 && k->stride != d->jmax * d->mmax) return JSS_E_SHAPE;
    if (k->delta_q16 < 0 || k->delta_q16 > 65536) return JSS_E_SHAPE;
    return decode_lds_bytes(d->jmax, d->mmax) > kOrderLdsLimit ? JSS_E_LDS : 0;
}

// jss_keys_evolve (libjss_decode_hip.so and the twin)
inline int evolve_check(const JssEvolve *e) {
    if (!e || !e->keys_out) return JSS_E_NULL;
    if (e->pop < 1 || e->pop > JSS_EVOLVE_MAX_POP || e->region < 1 || e->groups < 0) return JSS_E_SHAPE;
    if (e->n_elite < 0 || e->n_mutant < 0 || e->rho_q16 < 0 || e->rho_q16 > 65536) return JSS_E_SHAPE;
    if ((long long)e->n_elite + e->n_mutant > e->pop) return JSS_E_SHAPE;
    if (e->n_elite + e->n_mutant < e->pop && e->n_elite < 1) return JSS_E_SHAPE;
    const bool all_mutants = e->n_elite == 0 && e->n_mutant == e->pop;
    if (!all_mutants && (!e->fitness || !e->keys_in)) return JSS_E_NULL;
    if (e->keys_out == e->keys_in) return JSS_E_NULL;
    return 0;
}

// ---- one-machine relaxations and the shifting bottleneck construction (include/jss_machine.h) ---------------------------------
// What libjss_machine_hip.so keeps in LDS for one candidate, for the whole call: the op row, the rank row, the heads, the tails
// and a scratch row (int32) and two rows of machine-sorted sequences (uint16) over the entries of a [jmax][mmax] row rounded up
// to a multiple of 8, and four blocks of one word per machine.
inline long long machine_lds_bytes(int jmax, int mmax) { return 24 * order_entries8(jmax, mmax) + 4 * 64 * 4; }

// jss_machine_relax (libjss_machine_hip.so and the twin): the batch as jss_order_eval checks it
inline int machine_relax_check(const JssDesc *d, const JssState *s, const JssMachineRelax *r) {
    if (!d || !s || !r) return JSS_E_NULL;
    const int rc = check_args(d, s, nullptr, false);
    if (rc) return rc;
    if (!r->length || (!r->rank && r->fixed) || (r->rank_out && r->rank_out == r->rank)) return JSS_E_NULL;
    if (r->n < 0 || (!r->parents && r->n != d->batch)) return JSS_E_SHAPE;
    if (r->stride != 0 && r->stride != d->jmax * d->mmax) return JSS_E_SHAPE;
    return machine_lds_bytes(d->jmax, d->mmax) > kOrderLdsLimit ? JSS_E_LDS : 0;
}

// jss_bottleneck_build (libjss_machine_hip.so and the twin)
inline int bottleneck_check(const JssDesc *d, const JssState *s, const JssBottleneck *b) {
    if (!d || !s || !b) return JSS_E_NULL;
    const int rc = check_args(d, s, nullptr, false);
    if (rc) return rc;
    if (!b->makespan || !b->rank || !b->rank_in != !b->fixed_in || b->rank == b->rank_in) return JSS_E_NULL;
    if (b->n < 0 || (!b->parents && b->n != d->batch)) return JSS_E_SHAPE;
    if (b->reopt < 0 || b->reopt > JSS_BOTTLENECK_MAX_REOPT) return JSS_E_SHAPE;
    return machine_lds_bytes(d->jmax, d->mmax) > kOrderLdsLimit ? JSS_E_LDS : 0;
}

// ---- Carlier's one-machine search, shifting bottleneck constructions sequenced by it (include/jss_carlier.h) --------------------
// What libjss_carlier_hip.so keeps in LDS for one candidate: what machine_lds_bytes counts, a row of best starts (int32) and the
// undo stack of JSS_CARLIER_MAX_DEPTH entries of three words.
inline long long carlier_lds_bytes(int jmax, int mmax) {
    return 28 * order_entries8(jmax, mmax) + 4 * 64 * 4 + 3 * JSS_CARLIER_MAX_DEPTH * 4;
}

// jss_machine_solve (libjss_carlier_hip.so and the twin): the batch as jss_order_eval checks it
inline int machine_solve_check(const JssDesc *d, const JssState *s, const JssMachineSolve *r) {
    if (!d || !s || !r) return JSS_E_NULL;
    const int rc = check_args(d, s, nullptr, false);
    if (rc) return rc;
    if (!r->length || (!r->rank && r->fixed) || (r->rank_out && r->rank_out == r->rank)) return JSS_E_NULL;
    if (r->n < 0 || (!r->parents && r->n != d->batch)) return JSS_E_SHAPE;
    if (r->nodes < 1 || r->nodes > JSS_CARLIER_MAX_NODES) return JSS_E_SHAPE;
    if (r->stride != 0 && r->stride != d->jmax * d->mmax) return JSS_E_SHAPE;
    return carlier_lds_bytes(d->jmax, d->mmax) > kOrderLdsLimit ? JSS_E_LDS : 0;
}

// jss_bottleneck_exact (libjss_carlier_hip.so and the twin)
inline int bottleneck_exact_check(const JssDesc *d, const JssState *s, const JssBottleneckExact *b) {
    if (!d || !s || !b) return JSS_E_NULL;
    const int rc = check_args(d, s, nullptr, false);
    if (rc) return rc;
    if (!b->makespan || !b->rank || !b->rank_in != !b->fixed_in || b->rank == b->rank_in) return JSS_E_NULL;
    if (b->n < 0 || (!b->parents && b->n != d->batch)) return JSS_E_SHAPE;
    if (b->reopt < 0 || b->reopt > JSS_BOTTLENECK_MAX_REOPT) return JSS_E_SHAPE;
    if (b->nodes < 1 || b->nodes > JSS_CARLIER_MAX_NODES) return JSS_E_SHAPE;
    return carlier_lds_bytes(d->jmax, d->mmax) > kOrderLdsLimit ? JSS_E_LDS : 0;
}

// ---- constraint propagation on operation windows (include/jss_propagate.h) -------------------------------------------------------
// What libjss_propagate_hip.so keeps in LDS for one candidate: the op row, the rank row and both generations of est and of lct
// (int32) and three rows of machine-sorted sequences (uint16) over the entries of a [jmax][mmax] row rounded up to a multiple of
// 8, and four blocks of one word per machine.
inline long long propagate_lds_bytes(int jmax, int mmax) { return 30 * order_entries8(jmax, mmax) + 4 * 64 * 4; }

// jss_propagate (libjss_propagate_hip.so and the twin): the batch as jss_order_eval checks it
inline int propagate_check(const JssDesc *d, const JssState *s, const JssPropagate *r) {
    if (!d || !s || !r) return JSS_E_NULL;
    const int rc = check_args(d, s, nullptr, false);
    if (rc) return rc;
    if (!r->status || !r->ub || (!r->rank && r->fixed) || !r->est_in != !r->lct_in) return JSS_E_NULL;
    if (!r->hyp_op != !r->hyp_est || !r->hyp_op != !r->hyp_lct) return JSS_E_NULL;
    if (r->est && (r->est == r->est_in || r->est == r->lct_in)) return JSS_E_NULL;
    if (r->lct && (r->lct == r->est_in || r->lct == r->lct_in)) return JSS_E_NULL;
    if (r->n < 0 || (!r->parents && r->n != d->batch)) return JSS_E_SHAPE;
    if (r->passes < 1 || r->passes > JSS_PROPAGATE_MAX_PASSES) return JSS_E_SHAPE;
    if (r->stride != 0 && r->stride != d->jmax * d->mmax) return JSS_E_SHAPE;
    if (r->win_stride != 0 && r->win_stride != d->jmax * d->mmax) return JSS_E_SHAPE;
    return propagate_lds_bytes(d->jmax, d->mmax) > kOrderLdsLimit ? JSS_E_LDS : 0;
}

// jss_error_string's text for 0 and the argument codes; nullptr for any other code (each library words those itself)
inline const char *arg_error_string(int code) {
    switch (code) {
    case 0: return "ok";
    case JSS_E_NULL: return "null pointer in JssDesc/JssState/JssOut or arguments";
    case JSS_E_SHAPE: return "bad shape (batch/jmax/mmax/n_tables/n_sub)";
    case JSS_E_KIND: return "unknown policy kind or kernel flavour";
    case JSS_E_LDS: return "batch shape needs more LDS per workgroup than the device provides";
    case JSS_E_RESIDENT: return "the batch does not fit the chip as one round of resident workgroups (step session)";
    case JSS_E_SESSION: return "step session: bad step range (mailbox ring overrun, or the session was never opened)";
    default: return nullptr;
    }
}

}  // namespace jss_abi
