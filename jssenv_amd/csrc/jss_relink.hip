// jssenv_amd/csrc/jss_relink.hip -- libjss_relink_hip.so: jss_relink_walk (include/jss_relink.h), per env the distance between two
// machine orders and a whole walk from the one towards the other in one launch on the MI355X.  A library of its own:
// libjss_hip.so, libjss_beam_hip.so, libjss_bound_hip.so, libjss_order_hip.so, libjss_tabu_hip.so, libjss_block_hip.so and their
// kernels are not touched by it (the device helpers it has in common with jss_block.hip are written out again here for that
// reason).  It shares jss_abi_checks.hpp (the argument checks and the LDS a walker needs) with the host-core twin, which carries
// the same entry point.
//
// jss_relink_kernel: one wavefront per walker, walker i being env i; everything a branch or a loop around a cross-lane operation
// depends on is wave-uniform, so every way out of the kernel takes the whole wavefront.  Job j sits on lane j % 64, slot j / 64
// (two slots beyond 64 jobs).  No workgroup barrier is used: the wavefronts of a workgroup only share its LDS allocation, each
// with a region of its own (relink_lds_bytes), and the host picks 4, 2 or 1 of them per workgroup by that size.  The semantics
// are the header's; the form:
//
//   once    as jss_block_kernel: the op words into LDS (with the operation's index in its job in the word's free top byte) and
//           the machines sorted by (key, flat index) into seq[], machine-major and position ascending -- first with the guide as
//           the key, which is timed once for its cycle check and leaves g[], every operation's position in the guide order, then
//           with the source.  seq[] and g[] stay in LDS for the whole walk; a move exchanges two entries of seq[].
//   dist0   counted once: a lane per position, along seq[] to the end of its machine's segment, the entries whose guide position
//           is lower.  After that the distance only counts down.
//   a move  backward over the current order, whose starts the last forward pass left: the tails, stored.  Then 64 adjacent
//           positions at a time, a lane each: guide comparison, screen and estimate out of LDS.  The choice is a wave minimum and
//           a ballot per chunk, the chunks in listing order.  Two entries of seq[] are exchanged, and ONE forward pass re-times
//           the new order exactly: it is also the next move's forward pass.
//   fallback  (no candidate passed the screen) the candidates in ascending (estimate, position), each found by one more sweep
//           over the chunks behind the one tried last: exchanged, timed by the same forward pass without its stores -- so the
//           starts and tails the estimates come from stay whole -- and exchanged back where the pass reports a cycle.  At most
//           as many tries as the move has candidates.
//   out     best_rank is written to global memory in a coalesced pass whenever the best improves (the positions are gathered
//           through slot[]), so the best order needs no LDS copy; last_rank once, at the end.  A move's only other global
//           traffic is its trace word and its two move_log words.
//
// Every loop is bounded: the rounds of a pass by the operation count (a round that fires nothing ends it early), a lane's count
// by its machine's segment, the chunks by the operation count, the fallback's tries by the candidates, the moves by steps.  Every
// index into LDS is a position below the operation count or the flat index of a real operation.  No scratch memory, no spilled
// registers, LDS only as dynamic allocation of at most 64 KB (tests/test_relink.py reads the code object's notes); only vector
// stores; only what the tests' SIMT emulator provides is used, so the unmodified source runs there.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "jss_abi_checks.hpp"

namespace {

constexpr int kWave = 64;
constexpr int kDurMask = 0xffff;
constexpr int kNever = 0x7fffffff;

// what the kernel reads of (desc, state, r): the members by value, so that the kernel's arguments stay few
struct RelinkParams {
    const int32_t *env_const, *ops, *rank, *guide, *until_of;
    int32_t *best_makespan, *best_rank, *last_makespan, *last_rank, *info, *trace, *move_log;
    int32_t steps, until, margin, batch, jmax, mmax, n_tables;
    int32_t waves_per_block;
    int32_t wave_lds_ints;        // relink_lds_bytes / 4
    int32_t entries8;             // order_entries8
};

// a walker's LDS and shape, as every pass sees them
struct Walker {
    int32_t *val;                 // sorting: keys in segment order; then the starts of the current order, by flat index
    int32_t *opw;                 // the op words, by flat index: k << 24 | machine << 16 | duration
    int32_t *tl;                  // the tails of the current order, by flat index
    uint16_t *slot;               // sorting: flat indices as dealt; output: positions
    uint16_t *seq;                // the order: flat indices, machine-major, position ascending
    uint16_t *g;                  // the guide order: every operation's position on its machine, by flat index
    int32_t *m_off, *m_cnt;       // the machines' segments of seq[]: first entry and length
    int32_t *m_cur, *m_rel;
    int lane, J, M, mmax, total;
};

__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }

// LDS writes of one wave consumed by other lanes of the same wave
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = imax(v, __shfl_xor(v, off));
    return v;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = imin(v, __shfl_xor(v, off));
    return v;
}

// lanes below this one whose bit is set in `mask`
__device__ __forceinline__ int lanes_below(unsigned long long mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Forward over seq[]: the makespan, or -1 when the order has no schedule (wave-uniform either way).  kStore: the starts go to
// val[].  What lane 0 wrote to seq[] before the call is seen by the first round (the sync behind the cursors' reset).
template <bool kStore>
__device__ __forceinline__ int forward_pass(const Walker &w) {
    const int lane = w.lane, J = w.J, M = w.M, mmax = w.mmax;
    w.m_cur[lane] = w.m_off[lane], w.m_rel[lane] = 0;
    wave_lds_sync();
    int next_k[2] = {0, 0}, job_end[2] = {0, 0}, op_now[2] = {0, 0};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int j = s * kWave + lane;
        if (j < J) op_now[s] = w.opw[j * mmax];
    }
    // a round fires one operation at least, so total rounds place everything; one that fires nothing ends the pass early
#pragma unroll 1
    for (int round = 0; round < w.total; ++round) {
        bool ready[2] = {false, false};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (s * kWave >= J) break;
            const int j = s * kWave + lane;
            if (j < J && next_k[s] < M) ready[s] = w.seq[w.m_cur[(op_now[s] >> 16) & 63]] == j * mmax + next_k[s];
        }
        if (!__ballot(ready[0] || ready[1])) break;                   // (all lanes have looked before any lane writes)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (!ready[s]) continue;
            const int j = s * kWave + lane, m = (op_now[s] >> 16) & 63, x = j * mmax + next_k[s];
            const int st = imax(job_end[s], w.m_rel[m]);
            if (kStore) w.val[x] = st;
            job_end[s] = st + (op_now[s] & kDurMask);
            w.m_rel[m] = job_end[s], w.m_cur[m] += 1;                 // (one operation per machine per round: no collision)
            next_k[s] += 1;
            if (next_k[s] < M) op_now[s] = w.opw[x + 1];
        }
        wave_lds_sync();
    }
    const bool open = (lane < J && next_k[0] < M) || (kWave + lane < J && next_k[1] < M);
    if (__ballot(open)) return -1;                                    // operations remain and none can start: a cycle
    return wave_max(imax(job_end[0], job_end[1]));
}

// Backward over seq[] behind a forward pass that stored the starts' order: the tails go to tl[].  The operation behind on the
// machine was placed in an earlier round and has left, per machine, its duration and tail.
__device__ __forceinline__ void backward_pass(const Walker &w) {
    const int lane = w.lane, J = w.J, M = w.M, mmax = w.mmax;
    w.m_cur[lane] = w.m_off[lane] + w.m_cnt[lane] - 1, w.m_rel[lane] = 0;
    wave_lds_sync();
    int next_k[2] = {M - 1, M - 1}, job_tail[2] = {0, 0}, op_now[2] = {0, 0};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int j = s * kWave + lane;
        if (j < J) op_now[s] = w.opw[j * mmax + M - 1];
    }
#pragma unroll 1
    for (int round = 0; round < w.total; ++round) {
        bool ready[2] = {false, false};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (s * kWave >= J) break;
            const int j = s * kWave + lane;
            if (j < J && next_k[s] >= 0) ready[s] = w.seq[w.m_cur[(op_now[s] >> 16) & 63]] == j * mmax + next_k[s];
        }
        if (!__ballot(ready[0] || ready[1])) break;                   // everything is placed (a forward pass has ended on this order)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (!ready[s]) continue;
            const int j = s * kWave + lane, m = (op_now[s] >> 16) & 63, x = j * mmax + next_k[s];
            const int dur = op_now[s] & kDurMask;
            const int tl = imax(job_tail[s], w.m_rel[m]);
            w.tl[x] = tl;
            job_tail[s] = dur + tl;
            w.m_rel[m] = dur + tl, w.m_cur[m] -= 1;
            next_k[s] -= 1;
            if (next_k[s] >= 0) op_now[s] = w.opw[x - 1];
        }
        wave_lds_sync();
    }
}

// The order of seq[] as positions on the machines, -1 in the padding, in a coalesced pass: gathered by flat index through slot[],
// which is idle once the machines are sorted.  (The last chunk's spare lanes repeat its last entry -- the
// same value to the same place -- so that no lane predicate has to live in registers through the walk.)
__device__ __forceinline__ void write_positions(const Walker &w, int32_t *out, int jmax) {
    wave_lds_sync();                                                  // (the exchange in seq[])
#pragma unroll 1
    for (int i0 = 0; i0 < w.total; i0 += kWave) {
        const int i = imin(i0 + w.lane, w.total - 1), e = w.seq[i];
        w.slot[e] = (uint16_t)(i - w.m_off[(w.opw[e] >> 16) & 63]);
    }
    wave_lds_sync();
    const int region = jmax * w.mmax;
#pragma unroll 1
    for (int e0 = 0; e0 < region; e0 += kWave) {
        const int e = imin(e0 + w.lane, region - 1), j = e / w.mmax, k = e - j * w.mmax;
        out[e] = j < w.J && k < w.M ? (int)w.slot[e] : -1;
    }
}

// The machines' orders by (key, flat index) into seq[], through slot[] and val[] (jss_order_eval_kernel's deal and count).
__device__ __forceinline__ void sort_machines(const Walker &w, const int32_t *key, int region) {
    const int lane = w.lane, J = w.J, M = w.M, mmax = w.mmax;
    w.m_cur[lane] = 0;
    wave_lds_sync();
#pragma unroll 1
    for (int e = lane; e < region; e += kWave) {
        const int j = e / mmax, k = e - j * mmax;
        const int r = key[e];
        if (j < J && k < M) {
            const int m = (w.opw[e] >> 16) & 63;
            const int at = w.m_off[m] + atomicAdd(&w.m_cur[m], 1);
            w.slot[at] = (uint16_t)e, w.val[at] = r;
        }
    }
    wave_lds_sync();
#pragma unroll 1
    for (int x0 = lane; x0 < w.total; x0 += kWave) {
        const int x = w.slot[x0], r = w.val[x0], m = (w.opw[x] >> 16) & 63;
        const int lo = w.m_off[m], hi = lo + w.m_cnt[m];
        int pos = 0;
#pragma unroll 1
        for (int t = lo; t < hi; t += 4) {
            int y[4], ry[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int at = imin(t + u, hi - 1);                   // (clamped, not branched around: the loads go out together)
                y[u] = w.slot[at], ry[u] = w.val[at];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) pos += (t + u < hi && (ry[u] < r || (ry[u] == r && y[u] < x))) ? 1 : 0;
        }
        w.seq[lo + pos] = (uint16_t)x;
    }
    wave_lds_sync();                                                  // (val[] and slot[] are free from here)
}

// The candidate at position x0 + lane of seq[], if there is one: bit 0 of the result says that the entries at and behind the
// position are on one machine with the guide having them the other way round, bit 1 that the screen calls the swap sure; *est its
// estimate.  A lane without a candidate reads what a neighbour reads: no nest of branches.
__device__ __forceinline__ int candidate(const Walker &w, int x0, int *est) {
    const int M = w.M;
    const int at = imin(x0 + w.lane, w.total - 1);
    const int u = w.seq[at], ou = w.opw[u], m = (ou >> 16) & 63, m_lo = w.m_off[m], m_hi = m_lo + w.m_cnt[m];
    const int v = w.seq[imin(at + 1, m_hi - 1)], ov = w.opw[v];
    const bool cand = x0 + w.lane < w.total && at + 1 < m_hi && w.g[u] > w.g[v];
    const int ku = ou >> 24, kv = ov >> 24, du = ou & kDurMask, dv = ov & kDurMask;
    const bool has_s = ku + 1 < M, has_p = kv > 0;
    const int s = u + (has_s ? 1 : 0), p = v - (has_p ? 1 : 0);      // JS(u), JP(v)
    const int up = u - (ku > 0 ? 1 : 0), down = v + (kv + 1 < M ? 1 : 0);   // JP(u), JS(v)
    const int before = w.seq[imax(at - 1, m_lo)], after = w.seq[imin(at + 2, m_hi - 1)];
    const int end_s = w.val[s] + (w.opw[s] & kDurMask);
    const int head = at > m_lo ? w.val[before] + (w.opw[before] & kDurMask) : 0;
    const int behind = at + 2 < m_hi ? (w.opw[after] & kDurMask) + w.tl[after] : 0;
    const int hv = imax(has_p ? w.val[p] + (w.opw[p] & kDurMask) : 0, head);
    const int hu = imax(ku > 0 ? w.val[up] + (w.opw[up] & kDurMask) : 0, hv + dv);
    const int tu = du + imax(has_s ? (w.opw[s] & kDurMask) + w.tl[s] : 0, behind);
    const int tv = dv + imax(kv + 1 < M ? (w.opw[down] & kDurMask) + w.tl[down] : 0, tu);
    *est = imax(hv + tv, hu + tu);
    const bool sure = !has_s || !has_p || (s != p && w.val[p] < end_s);
    return (cand ? 1 : 0) | (cand && sure ? 2 : 0);
}

// the entries at `at` and `at` + 1 of seq[] change places (every lane has read what it needed: a cross-lane operation lies between)
__device__ __forceinline__ void exchange(const Walker &w, int at) {
    if (w.lane == 0) {
        const uint16_t a = w.seq[at];
        w.seq[at] = w.seq[at + 1], w.seq[at + 1] = a;
    }
}

// (the lane index from the lane masks, here and at the kernel's end: the predicates are made where they are used and not
// carried in registers through everything in between)
__device__ __forceinline__ void refuse(const RelinkParams &p, long long i, int code) {
    const int late = lanes_below(~0ull);
    if (late == 0) p.best_makespan[i] = code;
    if (late == 0 && p.last_makespan) p.last_makespan[i] = code;
    if (p.info && late < JSS_RELINK_NI) p.info[i * JSS_RELINK_NI + late] = late == 0 ? code : 0;
}

__global__ __launch_bounds__(256) void jss_relink_kernel(RelinkParams p) {
    HIP_DYNAMIC_SHARED(int32_t, lds)

    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    const long long i = (long long)blockIdx.x * p.waves_per_block + wv;
    if (i >= p.batch) return;                                         // (the whole wavefront, like every return below)
    const int jmax = p.jmax, mmax = p.mmax, region = jmax * mmax;
    const int32_t *ec = p.env_const + (size_t)i * JSS_NC;
    const int J = __builtin_amdgcn_readfirstlane(ec[JSS_C_JOBS]), M = __builtin_amdgcn_readfirstlane(ec[JSS_C_MACHINES]);
    const int tab = __builtin_amdgcn_readfirstlane(ec[JSS_C_TABLE]);
    const int until = __builtin_amdgcn_readfirstlane(p.until_of ? p.until_of[i] : p.until);
    // (J == 0: never reset.  The rest holds for every env a reset has written; it keeps the walks inside the rows)
    if (!(J >= 1 && J <= jmax && M >= 1 && M <= mmax && tab >= 0 && tab < p.n_tables) || until < 0) return refuse(p, i, -1);
    const int32_t *rank = p.rank + (size_t)i * region, *guide = p.guide + (size_t)i * region;
    const int32_t *ops = p.ops + (size_t)tab * region;

    // this wavefront's LDS: four blocks of one word per machine (at fixed offsets, which cost no register), then three int32 rows
    // and three uint16 rows over the entries
    Walker w;
    w.m_off = lds + (size_t)wv * p.wave_lds_ints;
    w.m_cnt = w.m_off + kWave;
    w.m_cur = w.m_cnt + kWave;
    w.m_rel = w.m_cur + kWave;
    w.val = w.m_rel + kWave;
    w.opw = w.val + p.entries8;
    w.tl = w.opw + p.entries8;
    w.slot = reinterpret_cast<uint16_t *>(w.tl + p.entries8);
    w.seq = w.slot + p.entries8;
    w.g = w.seq + p.entries8;
    w.lane = lane, w.J = J, w.M = M, w.mmax = mmax, w.total = J * M;
    const int total = w.total;

    // ---- once: op words, the check of both rows, the machines' counts and offsets (jss_order_eval_kernel 1-2) ------------------
    w.m_cnt[lane] = 0;
    wave_lds_sync();
    bool bad = false;
#pragma unroll 1
    for (int e = lane; e < region; e += kWave) {
        const int j = e / mmax, k = e - j * mmax;
        const int r = rank[e], gd = guide[e], o = ops[e];
        if (j < J && k < M) {
            bad |= r < 0 || gd < 0;
            w.opw[e] = (o & 0x3fffff) | k << 24;
            atomicAdd(&w.m_cnt[(o >> 16) & 63], 1);
        }
    }
    if (__ballot(bad)) return refuse(p, i, -1);
    wave_lds_sync();
    {
        const int mine_cnt = w.m_cnt[lane];
        int incl = mine_cnt;
#pragma unroll
        for (int dlt = 1; dlt < kWave; dlt <<= 1) {
            const int below = __shfl(incl, (lane - dlt) & 63);
            if (lane >= dlt) incl += below;
        }
        w.m_off[lane] = incl - mine_cnt;
    }
    wave_lds_sync();

    // ---- the guide: its order, its cycle check, g[] ----------------------------------------------------------------------------
    sort_machines(w, guide, region);
    const bool guide_cyclic = forward_pass<false>(w) < 0;
#pragma unroll 1
    for (int x0 = 0; x0 < total; x0 += kWave) {
        const int x = imin(x0 + lane, total - 1), e = w.seq[x];       // (spare lanes repeat the last entry)
        w.g[e] = (uint16_t)(x - w.m_off[(w.opw[e] >> 16) & 63]);
    }
    wave_lds_sync();

    // ---- the start -----------------------------------------------------------------------------------------------------------
    sort_machines(w, rank, region);
    int cur = forward_pass<true>(w);
    if (cur < 0 || guide_cyclic) return refuse(p, i, -2);
    int dist = 0;
#pragma unroll 1
    for (int x0 = 0; x0 < total; x0 += kWave) {
        const int x = imin(x0 + lane, total - 1), e = w.seq[x], m = (w.opw[e] >> 16) & 63, hi = w.m_off[m] + w.m_cnt[m];
        const int ge = w.g[e];
        int n = 0;
#pragma unroll 1
        for (int y = x + 1; y < hi; ++y) n += ge > (int)w.g[w.seq[y]] ? 1 : 0;
        dist += wave_sum(x0 + lane < total ? n : 0);
    }
    const int dist0 = dist, margin = p.margin, steps = p.steps;
    int best = 0, moves = 0, best_move = -1, candidates = 0, fallbacks = 0, retries = 0;
    int32_t *trace = p.trace ? p.trace + (size_t)i * steps : nullptr;
    int32_t *moved = p.move_log ? p.move_log + (size_t)i * steps * 2 : nullptr;
    if (margin == 0) {                              // the source as the best, where eligible
        best = cur, best_move = 0;
        write_positions(w, p.best_rank + (size_t)i * region, jmax);
    }
    int stop = dist == 0 ? 1 : dist <= until ? 2 : 0;

    // ---- the walk ------------------------------------------------------------------------------------------------------------
#pragma unroll 1
    for (int t = 1; t <= steps && stop == 0; ++t) {
        backward_pass(w);                                             // (val[] holds the starts of this order: the last forward pass)
        int found = 0, take = -1, take_est = 0;
#pragma unroll 1
        for (int x0 = 0; x0 < total; x0 += kWave) {
            int est;
            const int flags = candidate(w, x0, &est);
            const bool sure = (flags & 2) != 0;
            found += __popcll(__ballot(flags & 1));
            if (__ballot(sure)) {                                     // the lowest (estimate, listing order)
                const int low = __builtin_amdgcn_readfirstlane(wave_min(sure ? est : kNever));
                const int who = __ffsll(__ballot(sure && est == low)) - 1;
                if (take < 0 || low < take_est) take = x0 + who, take_est = low;
            }
        }
        candidates += found;
        int mk = -1;
        if (take >= 0) {
            exchange(w, take);
            mk = __builtin_amdgcn_readfirstlane(forward_pass<true>(w));   // the exact re-timing, and the next move's starts
            if (mk < 0) exchange(w, take);                            // (unreachable: the screen)
        } else {
            fallbacks += 1;
            int last_est = -1, last_at = -1;                          // the candidate tried last
#pragma unroll 1
            for (int tries = 0; tries < found; ++tries) {
                int next = -1, next_est = 0;
#pragma unroll 1
                for (int x0 = 0; x0 < total; x0 += kWave) {
                    int est;
                    const int flags = candidate(w, x0, &est);
                    const bool open = (flags & 1) != 0 && (est > last_est || (est == last_est && x0 + lane > last_at));
                    if (__ballot(open)) {
                        const int low = __builtin_amdgcn_readfirstlane(wave_min(open ? est : kNever));
                        const int who = __ffsll(__ballot(open && est == low)) - 1;
                        if (next < 0 || low < next_est) next = x0 + who, next_est = low;
                    }
                }
                if (next < 0) break;
                exchange(w, next);
                mk = __builtin_amdgcn_readfirstlane(forward_pass<false>(w));   // (no stores: the estimates' starts and tails stay whole)
                if (mk >= 0) {
                    take = next;
                    break;
                }
                exchange(w, next);
                wave_lds_sync();
                retries += 1, last_est = next_est, last_at = next;
            }
            if (mk >= 0) mk = __builtin_amdgcn_readfirstlane(forward_pass<true>(w));
        }
        if (mk < 0) {                                                 // (unreachable: jss_relink.h says why)
            if (take >= 0) forward_pass<true>(w);                     // the starts of the order left behind
            stop = 4;
            break;
        }
        cur = mk, moves = t, dist -= 1;
        if (lane == ((t - 1) & 63)) {                                 // (seq[take] is v now, seq[take + 1] is u)
            if (trace) trace[t - 1] = cur;
            if (moved) moved[2 * (t - 1)] = w.seq[take + 1], moved[2 * (t - 1) + 1] = w.seq[take];
        }
        if (t >= margin && dist >= margin && (best_move < 0 || cur < best)) {
            best = cur, best_move = t;
            write_positions(w, p.best_rank + (size_t)i * region, jmax);
        }
        stop = dist == 0 ? 1 : dist <= until ? 2 : 0;
    }

    // ---- the end -------------------------------------------------------------------------------------------------------------
    if (best_move < 0) {                                              // no order was eligible: the last one
        best = cur;
        write_positions(w, p.best_rank + (size_t)i * region, jmax);
    }
    const int late = lanes_below(~0ull);
    if (late == 0) p.best_makespan[i] = best;
    if (late == 0 && p.last_makespan) p.last_makespan[i] = cur;
    if (p.info && late < JSS_RELINK_NI)
        p.info[i * JSS_RELINK_NI + late] = late == 0 ? stop : late == 1 ? moves : late == 2 ? best_move : late == 3 ? dist0
                                         : late == 4 ? dist : late == 5 ? candidates : late == 6 ? fallbacks : retries;
    if (p.last_rank) write_positions(w, p.last_rank + (size_t)i * region, jmax);
    if (trace)
        for (int x = moves + lane; x < steps; x += kWave) trace[x] = -1;
    if (moved)
        for (int x = 2 * moves + lane; x < 2 * steps; x += kWave) moved[x] = -1;
}

}  // namespace

extern "C" {

int jss_relink_walk(const JssDesc *desc, const JssState *state, const JssRelink *r, void *stream) {
    if (const int rc = jss_abi::relink_check(desc, state, r)) return rc;
    if (desc->batch == 0) return 0;
    RelinkParams p;
    p.env_const = state->env_const, p.ops = desc->ops, p.rank = r->rank, p.guide = r->guide, p.until_of = r->until_of;
    p.best_makespan = r->best_makespan, p.best_rank = r->best_rank, p.last_makespan = r->last_makespan, p.last_rank = r->last_rank;
    p.info = r->info, p.trace = r->trace, p.move_log = r->move_log;
    p.steps = r->steps, p.until = r->until, p.margin = r->margin;
    p.batch = desc->batch, p.jmax = desc->jmax, p.mmax = desc->mmax, p.n_tables = desc->n_tables;
    const long long bytes = jss_abi::relink_lds_bytes(desc->jmax, desc->mmax);
    p.entries8 = (int32_t)jss_abi::order_entries8(desc->jmax, desc->mmax);
    p.wave_lds_ints = (int32_t)(bytes / 4);
    // wavefronts per workgroup: they only share the LDS allocation, and small allocations pack a CU's 160 KB better
    p.waves_per_block = 4 * bytes <= 32 * 1024 ? 4 : 2 * bytes <= 32 * 1024 ? 2 : 1;
    const size_t shmem = (size_t)bytes * p.waves_per_block;          // at most 64 KB (relink_check): no function attribute to raise
    const long long blocks = ((long long)desc->batch + p.waves_per_block - 1) / p.waves_per_block;
    hipLaunchKernelGGL(jss_relink_kernel, dim3((unsigned)blocks), dim3((unsigned)(kWave * p.waves_per_block)), shmem,
                       reinterpret_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

}  // extern "C"
