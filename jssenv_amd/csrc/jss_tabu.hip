// jssenv_amd/csrc/jss_tabu.hip -- libjss_tabu_hip.so: jss_tabu_search (include/jss_tabu.h), a whole tabu walk per env in one launch
// on the MI355X.  A library of its own: libjss_hip.so, libjss_beam_hip.so, libjss_bound_hip.so, libjss_order_hip.so and their
// kernels are not touched by it (the few device helpers it has in common with jss_order.hip are written out again here for that
// reason).  It shares jss_abi_checks.hpp (the argument checks and the LDS a walker needs) with the host-core twin, which carries
// the same entry point.
//
// jss_tabu_kernel: one wavefront per walker, walker i being env i; everything a branch or a loop depends on is wave-uniform, so
// every way out of the kernel takes the whole wavefront.  Job j sits on lane j % 64, slot j / 64 (two slots beyond 64 jobs).  No
// workgroup barrier is used: the wavefronts of a workgroup only share its LDS allocation, each with a region of its own
// (tabu_lds_bytes), and the host picks 4, 2 or 1 of them per workgroup by that size.  The semantics are the header's; the form:
//
//   once    the op words into LDS and the machines sorted by (rank, flat index) -- steps 1 to 3 of jss_order_eval_kernel -- which
//           leaves seq[], machine-major and position ascending.  seq[] stays in LDS for the whole walk: a move is the exchange of
//           two neighbouring entries, and the rank row is not looked at again.
//   a move  forward over the current order, in rounds (a job whose next operation stands at its machine's cursor starts it), for
//           the starts; backward, the mirror image, which marks the pairs; the marks are compacted in place into the list of the
//           pairs' positions, in the header's listing order.  Then, pair by pair: lane 0 exchanges the two entries, a forward pass
//           gives the makespan and nothing else, lane 0 exchanges them back.  Only listed pairs are timed, and none re-sorts.
//   tabu    the list lives in registers: lane l holds the pair (min << 16 | max of the two flat indices, both below 5352) and the
//           number of move s with (s - 1) % 64 == l; 64 entries cover the largest tenure.  A tabu test is one compare and a
//           ballot, the "oldest" choice a wave maximum per tabu neighbour and a running minimum.
//   out     best_rank is written to global memory in a coalesced pass whenever the best improves (the positions are gathered
//           through the then idle pair list), so the best order needs no LDS copy; last_rank once, at the end.  A move's only
//           other global traffic is its trace word.
//
// Every loop is bounded: the rounds of a pass by the operation count (a round that fires nothing ends it early), the pairs by
// the operation count, the moves by iters.  No scratch memory, no spilled registers, LDS only as dynamic allocation of at most
// 64 KB (tests/test_tabu.py reads the code object's notes); only vector stores; only what the tests' SIMT emulator provides is
// used, so the unmodified source runs there.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "jss_abi_checks.hpp"

namespace {

constexpr int kWave = 64;
constexpr int kDurMask = 0xffff;

// what the kernel reads of (desc, state, t): the members by value, so that the kernel's arguments stay few
struct TabuParams {
    const int32_t *env_const, *ops, *rank, *tenure_of, *target;
    int32_t *best_makespan, *best_rank, *last_rank, *info, *trace;
    int32_t iters, tenure, batch, jmax, mmax, n_tables;
    int32_t waves_per_block;
    int32_t wave_lds_ints;        // tabu_lds_bytes / 4
    int32_t entries8;             // order_entries8
};

// a walker's LDS and shape, as every pass sees them
struct Walker {
    int32_t *val;                 // sorting: ranks in segment order; then the starts of the current order, by flat index
    int32_t *opw;                 // the op words, by flat index
    uint16_t *slot;               // sorting: flat indices as dealt; a move: pair marks -> the pairs' positions; output: positions
    uint16_t *seq;                // the order: flat indices, machine-major, position ascending
    int32_t *m_off, *m_cnt;       // the machines' segments of seq[]: first entry and length
    int32_t *m_cur, *m_rel, *m_crit;
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

// lanes below this one whose bit is set in `mask`
__device__ __forceinline__ int lanes_below(unsigned long long mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
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

// Backward over seq[] behind a forward pass that stored the starts: slot[at] = 1 where the entries at and at + 1 are a pair.
// The operation behind on the machine was placed in an earlier round and has left, per machine, its start if it is critical.
__device__ __forceinline__ void backward_marks(const Walker &w, int makespan) {
    const int lane = w.lane, J = w.J, M = w.M, mmax = w.mmax;
    w.m_cur[lane] = w.m_off[lane] + w.m_cnt[lane] - 1, w.m_rel[lane] = 0, w.m_crit[lane] = -1;
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
            const int dur = op_now[s] & kDurMask, at = w.m_cur[m];
            const int st = w.val[x], tl = imax(job_tail[s], w.m_rel[m]);
            const bool critical = st + dur + tl == makespan;
            // the operation behind on the machine: critical and starting as this one ends -- then of another job?
            bool pair = critical && w.m_crit[m] == st + dur && at + 1 < w.m_off[m] + w.m_cnt[m];
            if (pair) pair = (int)w.seq[at + 1] / mmax != j;
            w.slot[at] = pair ? 1 : 0;
            job_tail[s] = dur + tl;
            w.m_rel[m] = dur + tl, w.m_crit[m] = critical ? st : -1, w.m_cur[m] = at - 1;
            next_k[s] -= 1;
            if (next_k[s] >= 0) op_now[s] = w.opw[x - 1];
        }
        wave_lds_sync();
    }
}

// The order of seq[] as positions on the machines, -1 in the padding, in a coalesced pass: gathered by flat index through slot[],
// which is idle between a move's choice and the next backward pass.
__device__ __forceinline__ void write_positions(const Walker &w, int32_t *out, int jmax) {
    wave_lds_sync();                                                  // (lane 0's exchange in seq[])
#pragma unroll 1
    for (int i = w.lane; i < w.total; i += kWave) {
        const int e = w.seq[i];
        w.slot[e] = (uint16_t)(i - w.m_off[(w.opw[e] >> 16) & 63]);
    }
    wave_lds_sync();
    const int region = jmax * w.mmax;
#pragma unroll 1
    for (int e = w.lane; e < region; e += kWave) {
        const int j = e / w.mmax, k = e - j * w.mmax;
        out[e] = j < w.J && k < w.M ? (int)w.slot[e] : -1;
    }
}

__device__ __forceinline__ void refuse(const TabuParams &p, long long i, int lane, int code) {
    if (lane == 0) p.best_makespan[i] = code;
    if (p.info && lane < JSS_TABU_NI) p.info[i * JSS_TABU_NI + lane] = lane == 0 ? code : 0;
}

__global__ __launch_bounds__(256) void jss_tabu_kernel(TabuParams p) {
    HIP_DYNAMIC_SHARED(int32_t, lds)

    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    const long long i = (long long)blockIdx.x * p.waves_per_block + wv;
    if (i >= p.batch) return;                                         // (the whole wavefront, like every return below)
    const int jmax = p.jmax, mmax = p.mmax, region = jmax * mmax;
    const int32_t *ec = p.env_const + (size_t)i * JSS_NC;
    const int J = __builtin_amdgcn_readfirstlane(ec[JSS_C_JOBS]), M = __builtin_amdgcn_readfirstlane(ec[JSS_C_MACHINES]);
    const int tab = __builtin_amdgcn_readfirstlane(ec[JSS_C_TABLE]);
    const int tenure = __builtin_amdgcn_readfirstlane(p.tenure_of ? p.tenure_of[i] : p.tenure);
    // (J == 0: never reset.  The rest holds for every env a reset has written; it keeps the walks inside the rows)
    if (!(J >= 1 && J <= jmax && M >= 1 && M <= mmax && tab >= 0 && tab < p.n_tables) || tenure < 0 || tenure > 64)
        return refuse(p, i, lane, -1);
    const int32_t *rank = p.rank + (size_t)i * region;
    const int32_t *ops = p.ops + (size_t)tab * region;

    // this wavefront's LDS: two int32 rows and two uint16 rows over the entries, five blocks of one word per machine
    Walker w;
    w.val = lds + (size_t)wv * p.wave_lds_ints;
    w.opw = w.val + p.entries8;
    w.slot = reinterpret_cast<uint16_t *>(w.opw + p.entries8);
    w.seq = w.slot + p.entries8;
    w.m_off = reinterpret_cast<int32_t *>(w.seq + p.entries8);
    w.m_cnt = w.m_off + kWave;
    w.m_cur = w.m_cnt + kWave;
    w.m_rel = w.m_cur + kWave;
    w.m_crit = w.m_rel + kWave;
    w.lane = lane, w.J = J, w.M = M, w.mmax = mmax, w.total = J * M;
    const int total = w.total;

    // ---- once: op words, rank check, the machines' counts and offsets, the deal, the positions (jss_order_eval_kernel 1-3) ---
    w.m_cnt[lane] = 0, w.m_cur[lane] = 0;
    wave_lds_sync();
    bool bad = false;
#pragma unroll 1
    for (int e = lane; e < region; e += kWave) {
        const int j = e / mmax, k = e - j * mmax;
        const int r = rank[e], o = ops[e];
        if (j < J && k < M) {
            bad |= r < 0;
            w.opw[e] = o;
            atomicAdd(&w.m_cnt[(o >> 16) & 63], 1);
        }
    }
    if (__ballot(bad)) return refuse(p, i, lane, -1);
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
#pragma unroll 1
    for (int e = lane; e < region; e += kWave) {
        const int j = e / mmax, k = e - j * mmax;
        const int r = rank[e];
        if (j < J && k < M) {
            const int m = (w.opw[e] >> 16) & 63;
            const int at = w.m_off[m] + atomicAdd(&w.m_cur[m], 1);
            w.slot[at] = (uint16_t)e, w.val[at] = r;
        }
    }
    wave_lds_sync();
#pragma unroll 1
    for (int x0 = lane; x0 < total; x0 += kWave) {
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

    // ---- the start -----------------------------------------------------------------------------------------------------------
    int cur = forward_pass<true>(w);
    if (cur < 0) return refuse(p, i, lane, -2);
    int best = cur, moves = 0, best_move = 0, evaluations = 0, stop = 0;
    write_positions(w, p.best_rank + (size_t)i * region, jmax);
    const bool aims = p.target != nullptr;
    const int target = aims ? __builtin_amdgcn_readfirstlane(p.target[i]) : 0;
    int32_t *trace = p.trace ? p.trace + (size_t)i * p.iters : nullptr;
    int list_key = -1, list_move = 0;                                 // this lane's entry of the tabu list
    if (aims && best <= target) stop = 2;

    // ---- the walk ------------------------------------------------------------------------------------------------------------
#pragma unroll 1
    for (int t = 1; t <= p.iters && stop == 0; ++t) {
        if (t > 1) forward_pass<true>(w);                             // the starts of the order the last move left
        backward_marks(w, cur);
        // the marks, compacted in place into the pairs' positions: seq[] is already in the order the header lists pairs in
        // (entry `at` of the list is written at or below the mark it comes from, and behind the ballot that read its chunk)
        int found = 0;
#pragma unroll 1
        for (int x0 = 0; x0 < total; x0 += kWave) {
            const int x = x0 + lane;
            const bool marked = x < total && w.slot[x] != 0;
            const unsigned long long mask = __ballot(marked);
            if (marked) w.slot[found + lanes_below(mask)] = (uint16_t)x;
            found += __popcll(mask);
        }
        wave_lds_sync();
        evaluations += found;
        const int lo = imax(1, t - tenure);                           // the moves lo ... t - 1 are the last `tenure`
        int take = -1, take_mk = 0, forced = -1, forced_mk = 0, forced_age = 0;
#pragma unroll 1
        for (int k = 0; k < found; ++k) {
            const int at = __builtin_amdgcn_readfirstlane((int)w.slot[k]);
            const int uv = __builtin_amdgcn_readfirstlane((int)w.seq[at] << 16 | (int)w.seq[at + 1]);   // (lane 0's view: it wrote them last)
            const int u = uv >> 16, v = uv & 0xffff;
            if (lane == 0) w.seq[at] = (uint16_t)v, w.seq[at + 1] = (uint16_t)u;
            const int mk = forward_pass<false>(w);
            if (lane == 0) w.seq[at] = (uint16_t)u, w.seq[at + 1] = (uint16_t)v;
            if (mk < 0) continue;                                     // no schedule: not usable
            const int key = imin(u, v) << 16 | imax(u, v);
            const bool match = list_move >= lo && list_key == key;
            const bool is_tabu = __ballot(match) != 0;
            if (!is_tabu || mk < best) {                              // admissible: the lowest (makespan, k)
                if (take < 0 || mk < take_mk) take = at, take_mk = mk;
            } else {                                                  // the one whose most recent entry is the oldest
                const int recent = wave_max(match ? list_move : 0);
                if (forced < 0 || recent < forced_age) forced = at, forced_mk = mk, forced_age = recent;
            }
        }
        if (take < 0) take = forced, take_mk = forced_mk;
        if (take < 0) {                                               // no usable neighbour: no critical machine arc
            stop = 1;
            break;
        }
        const int uv = __builtin_amdgcn_readfirstlane((int)w.seq[take] << 16 | (int)w.seq[take + 1]);
        const int u = uv >> 16, v = uv & 0xffff;
        if (lane == 0) w.seq[take] = (uint16_t)v, w.seq[take + 1] = (uint16_t)u;
        if (lane == ((t - 1) & 63)) list_key = imin(u, v) << 16 | imax(u, v), list_move = t;
        cur = take_mk, moves = t;
        if (trace && lane == 0) trace[t - 1] = cur;
        if (cur < best) {
            best = cur, best_move = t;
            write_positions(w, p.best_rank + (size_t)i * region, jmax);
        }
        if (aims && best <= target) stop = 2;
    }

    // ---- the end -------------------------------------------------------------------------------------------------------------
    if (lane == 0) p.best_makespan[i] = best;
    if (p.info && lane < JSS_TABU_NI)
        p.info[i * JSS_TABU_NI + lane] = lane == 0 ? stop : lane == 1 ? moves : lane == 2 ? best_move : evaluations;
    if (p.last_rank) write_positions(w, p.last_rank + (size_t)i * region, jmax);
    if (trace)
        for (int x = moves + lane; x < p.iters; x += kWave) trace[x] = -1;
}

}  // namespace

extern "C" {

int jss_tabu_search(const JssDesc *desc, const JssState *state, const JssTabu *t, void *stream) {
    if (const int rc = jss_abi::check_tabu_search(desc, state, t)) return rc;
    if (desc->batch == 0) return 0;
    TabuParams p;
    p.env_const = state->env_const, p.ops = desc->ops, p.rank = t->rank, p.tenure_of = t->tenure_of, p.target = t->target;
    p.best_makespan = t->best_makespan, p.best_rank = t->best_rank, p.last_rank = t->last_rank, p.info = t->info, p.trace = t->trace;
    p.iters = t->iters, p.tenure = t->tenure, p.batch = desc->batch, p.jmax = desc->jmax, p.mmax = desc->mmax, p.n_tables = desc->n_tables;
    const long long bytes = jss_abi::tabu_lds_bytes(desc->jmax, desc->mmax);
    p.entries8 = (int32_t)jss_abi::order_entries8(desc->jmax, desc->mmax);
    p.wave_lds_ints = (int32_t)(bytes / 4);
    // wavefronts per workgroup: they only share the LDS allocation, and small allocations pack a CU's 160 KB better
    p.waves_per_block = 4 * bytes <= 32 * 1024 ? 4 : 2 * bytes <= 32 * 1024 ? 2 : 1;
    const size_t shmem = (size_t)bytes * p.waves_per_block;          // at most 64 KB (check_tabu_search): no function attribute to raise
    const long long blocks = ((long long)desc->batch + p.waves_per_block - 1) / p.waves_per_block;
    hipLaunchKernelGGL(jss_tabu_kernel, dim3((unsigned)blocks), dim3((unsigned)(kWave * p.waves_per_block)), shmem,
                       reinterpret_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

}  // extern "C"
