// jssenv_amd/csrc/jss_block.hip -- libjss_block_hip.so: jss_block_search (include/jss_block.h), a whole tabu walk over block
// insertions per env in one launch on the MI355X.  A library of its own: libjss_hip.so, libjss_beam_hip.so, libjss_bound_hip.so,
// libjss_order_hip.so, libjss_tabu_hip.so and their kernels are not touched by it (the device helpers it has in common with
// jss_tabu.hip are written out again here for that reason).  It shares jss_abi_checks.hpp (the argument checks and the LDS a
// walker needs) with the host-core twin, which carries the same entry point.
//
// jss_block_kernel: one wavefront per walker, walker i being env i; everything a branch or a loop around a cross-lane operation
// depends on is wave-uniform, so every way out of the kernel takes the whole wavefront.  Job j sits on lane j % 64, slot j / 64
// (two slots beyond 64 jobs).  No workgroup barrier is used: the wavefronts of a workgroup only share its LDS allocation, each
// with a region of its own (block_lds_bytes), and the host picks 4, 2 or 1 of them per workgroup by that size.  The semantics
// are the header's; the form:
//
//   once    as jss_tabu_kernel: the op words into LDS (with the operation's index in its job in the word's free top byte, which
//           spares the candidates every division) and the machines sorted by (rank, flat index) into seq[], machine-major and
//           position ascending.  seq[] stays in LDS for the whole walk; a move rotates one stretch of it.
//   a move  backward over the current order, whose starts the last forward pass left: the tails, stored, and the marks; the
//           marked positions compacted into cand[], which is the header's listing order.  Then 32 marks at a time, two lanes per
//           mark -- F on the even lane, B on the odd one: a lane walks along the marks to its block's end, applies the screen and
//           sweeps once along the stretch in its new order for the estimate, all out of LDS.  The choice is a wave minimum and
//           a ballot per chunk.  The stretch is rotated through slot[], and ONE forward pass re-times the new order exactly:
//           it is also the next move's forward pass, so a move costs two passes however many candidates it had.
//   tabu    the list lives in registers: lane l holds the pair (min << 16 | max of the two flat indices, both below 3568) of
//           the move s with (s - 1) % 64 == l; 64 entries cover the largest tenure.  A chunk's candidates are tested against
//           the last L entries by one lane read per entry.
//   out     best_rank is written to global memory in a coalesced pass whenever the best improves (the positions are gathered
//           through slot[], idle then), so the best order needs no LDS copy; last_rank once, at the end.  A move's only other
//           global traffic is its trace word and its two move_log words.
//
// Every loop is bounded: the rounds of a pass by the operation count (a round that fires nothing ends it early), a lane's walk
// and sweep by its machine's segment, the chunks by the operation count, the moves by iters.  Every index into LDS is a position
// below the operation count or the flat index of a real operation.  No scratch memory, no spilled registers, LDS only as dynamic
// allocation of at most 64 KB (tests/test_block.py reads the code object's notes); only vector stores; only what the tests' SIMT
// emulator provides is used, so the unmodified source runs there.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "jss_abi_checks.hpp"

namespace {

constexpr int kWave = 64;
constexpr int kDurMask = 0xffff;

// what the kernel reads of (desc, state, t): the members by value, so that the kernel's arguments stay few
struct BlockParams {
    const int32_t *env_const, *ops, *rank, *tenure_of, *target;
    int32_t *best_makespan, *best_rank, *last_rank, *info, *trace, *move_log;
    int32_t iters, tenure, reach, batch, jmax, mmax, n_tables;
    int32_t waves_per_block;
    int32_t wave_lds_ints;        // block_lds_bytes / 4
    int32_t entries8;             // order_entries8
};

// a walker's LDS and shape, as every pass sees them
struct Walker {
    int32_t *val;                 // sorting: ranks in segment order; then the starts of the current order, by flat index
    int32_t *opw;                 // the op words, by flat index: k << 24 | machine << 16 | duration
    int32_t *tl;                  // the tails of the current order, by flat index
    uint16_t *slot;               // sorting: flat indices as dealt; a move: the marks, then the stretch in rotation; output: positions
    uint16_t *seq;                // the order: flat indices, machine-major, position ascending
    uint16_t *cand;               // a move: the marked positions, ascending
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

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = imin(v, __shfl_xor(v, off));
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

// Backward over seq[] behind a forward pass that stored the starts: the tails go to tl[], and slot[at] = 1 where the entries at
// and at + 1 are a pair.  The operation behind on the machine was placed in an earlier round and has left, per machine, its start
// if it is critical.
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
            if (pair) {                                               // (its row's first entry, without a division)
                const int other = w.seq[at + 1];
                pair = other - (w.opw[other] >> 24) != j * mmax;
            }
            w.slot[at] = pair ? 1 : 0, w.tl[x] = tl;
            job_tail[s] = dur + tl;
            w.m_rel[m] = dur + tl, w.m_crit[m] = critical ? st : -1, w.m_cur[m] = at - 1;
            next_k[s] -= 1;
            if (next_k[s] >= 0) op_now[s] = w.opw[x - 1];
        }
        wave_lds_sync();
    }
}

// The order of seq[] as positions on the machines, -1 in the padding, in a coalesced pass: gathered by flat index through slot[],
// which is idle between a move's choice and the next backward pass.  (The last chunk's spare lanes repeat its last entry -- the
// same value to the same place -- so that no lane predicate has to live in registers through the walk.)
__device__ __forceinline__ void write_positions(const Walker &w, int32_t *out, int jmax) {
    wave_lds_sync();                                                  // (the rotation in seq[])
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

// The stretch [from, to] of seq[] rotated by one place through slot[], which is idle behind a move's choice: to the left (the
// entry at `from` goes to `to`: an F move) or, with `back`, to the right (the entry at `to` goes to `from`: a B move).
__device__ __forceinline__ void rotate(const Walker &w, int from, int to, bool back) {
#pragma unroll 1
    for (int q = from + w.lane; q <= to; q += kWave) w.slot[q] = w.seq[q];
    wave_lds_sync();
#pragma unroll 1
    for (int q = from + w.lane; q <= to; q += kWave) w.seq[q] = w.slot[back ? (q == from ? to : q - 1) : (q == to ? from : q + 1)];
    wave_lds_sync();
}

// (the lane index from the lane masks, here and at the kernel's end: the predicates are made where they are used and not
// carried in registers through everything in between)
__device__ __forceinline__ void refuse(const BlockParams &p, long long i, int code) {
    const int late = lanes_below(~0ull);
    if (late == 0) p.best_makespan[i] = code;
    if (p.info && late < JSS_BLOCK_NI) p.info[i * JSS_BLOCK_NI + late] = late == 0 ? code : 0;
}

__global__ __launch_bounds__(256) void jss_block_kernel(BlockParams p) {
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
        return refuse(p, i, -1);
    const int32_t *rank = p.rank + (size_t)i * region;
    const int32_t *ops = p.ops + (size_t)tab * region;

    // this wavefront's LDS: five blocks of one word per machine (at fixed offsets, which cost no register), then three int32 rows
    // and three uint16 rows over the entries
    Walker w;
    w.m_off = lds + (size_t)wv * p.wave_lds_ints;
    w.m_cnt = w.m_off + kWave;
    w.m_cur = w.m_cnt + kWave;
    w.m_rel = w.m_cur + kWave;
    w.m_crit = w.m_rel + kWave;
    w.val = w.m_crit + kWave;
    w.opw = w.val + p.entries8;
    w.tl = w.opw + p.entries8;
    w.slot = reinterpret_cast<uint16_t *>(w.tl + p.entries8);
    w.seq = w.slot + p.entries8;
    w.cand = w.seq + p.entries8;
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
    if (cur < 0) return refuse(p, i, -2);
    int best = cur, moves = 0, best_move = 0, evaluations = 0, screened = 0, far = 0, hits = 0, stop = 0;
    write_positions(w, p.best_rank + (size_t)i * region, jmax);
    const int target = p.target ? __builtin_amdgcn_readfirstlane(p.target[i]) : -1;   // (no makespan is below 0)
    const int reach = p.reach;
    int32_t *trace = p.trace ? p.trace + (size_t)i * p.iters : nullptr;
    int32_t *moved = p.move_log ? p.move_log + (size_t)i * p.iters * 2 : nullptr;
    int list_key = -1;                                                // this lane's entry of the tabu list
    if (best <= target) stop = 2;

    // ---- the walk ------------------------------------------------------------------------------------------------------------
#pragma unroll 1
    for (int t = 1; t <= p.iters && stop == 0; ++t) {
        backward_marks(w, cur);                                       // (val[] holds the starts of this order: the last forward pass)
        int found = 0;
#pragma unroll 1
        for (int x0 = 0; x0 < total; x0 += kWave) {
            const int x = x0 + lane;
            const bool marked = x < total && w.slot[x] != 0;
            const unsigned long long mask = __ballot(marked);
            if (marked) w.cand[found + lanes_below(mask)] = (uint16_t)x;
            found += __popcll(mask);
        }
        if (found == 0) {                                             // no critical machine arc
            stop = 1;
            break;
        }
        wave_lds_sync();
        const int lo = imax(1, t - tenure);                           // the moves lo ... t - 1 are the last `tenure`
        // the choice so far: the stretch as from | to << 12 | back << 24, and its estimate
        int take = -1, take_est = 0, forced = -1, forced_est = 0, forced_age = 0;
#pragma unroll 1
        for (int c0 = 0; c0 < found; c0 += kWave / 2) {
            // (no nest of branches: a lane without a candidate reads what a neighbour reads and sweeps over nothing)
            const bool back = (lane & 1) != 0;
            const int at = w.cand[imin(c0 + (lane >> 1), found - 1)];
            const int m = (w.opw[w.seq[at]] >> 16) & 63, m_lo = w.m_off[m], m_hi = m_lo + w.m_cnt[m];
            int edge = back ? at : at + 1;                            // along the marks to the block's end (a mark's partner is on the machine)
            while (back ? edge > m_lo && w.slot[edge - 1] != 0 : edge + 1 < m_hi && w.slot[edge] != 0) edge += back ? -1 : 1;
            const int from = back ? edge : at, to = back ? at + 1 : edge;
            bool exists = c0 + (lane >> 1) < found && !(reach > 0 && to - from > reach);
            if (back) exists = exists && (from < at || (at + 2 < m_hi && w.slot[at + 1] != 0));   // a block of two marks at least
            const int x = w.seq[back ? to : from], y = w.seq[back ? from : to];
            const int ox = w.opw[x], oy = w.opw[y], kx = ox >> 24, row_x = x - kx;
            const int before = w.seq[imax(from - 1, m_lo)], after = w.seq[imin(to + 1, m_hi - 1)];
            int head = from > m_lo ? w.val[before] + (w.opw[before] & kDurMask) : 0;
            const int behind = to + 1 < m_hi ? (w.opw[after] & kDurMask) + w.tl[after] : 0;
            bool same_job = false;
            int est = 0;
            const int n = exists ? to - from : -1;
#pragma unroll 1
            for (int s = 0; s <= n; ++s) {                            // the stretch in its new order
                const int e = back ? (s == 0 ? x : (int)w.seq[from + s - 1]) : (s == n ? x : (int)w.seq[from + s + 1]);
                const int oe = w.opw[e], ke = oe >> 24;
                const int up = e - (ke > 0 ? 1 : 0), down = e + (ke + 1 < M ? 1 : 0);
                const int job_head = ke > 0 ? w.val[up] + (w.opw[up] & kDurMask) : 0;
                const int job_tail = ke + 1 < M ? (w.opw[down] & kDurMask) + w.tl[down] : 0;
                same_job |= e != x && e - ke == row_x;
                head = imax(job_head, head) + (oe & kDurMask);
                est = imax(est, head + imax(job_tail, s == n ? behind : 0));
            }
            const bool blocked = back ? kx > 0 && !(w.val[y] + (oy & kDurMask) > w.val[x - (kx > 0 ? 1 : 0)])
                                      : kx + 1 < M && !((oy & kDurMask) + w.tl[y] > w.tl[x + (kx + 1 < M ? 1 : 0)]);
            const bool screen = exists && (same_job || blocked), listed = exists && !screen;
            const int key = imin(x, y) << 16 | imax(x, y), span = from | to << 12 | (back ? 1 << 24 : 0);
            const unsigned long long listed_mask = __ballot(listed);
            evaluations += __popcll(listed_mask), screened += __popcll(__ballot(screen));
            if (listed_mask == 0) continue;
            int recent = 0;                                           // the latest of the last `tenure` moves that made this pair, or 0
#pragma unroll 1
            for (int s = lo; s < t; ++s)
                if (__shfl(list_key, (s - 1) & 63) == key) recent = s;
            const bool admissible = listed && (recent == 0 || est < best);
            const bool rest = listed && !admissible;
            if (__ballot(admissible)) {                               // the lowest (estimate, listing order)
                const int low = __builtin_amdgcn_readfirstlane(wave_min(admissible ? est : 0x7fffffff));
                const int who = __ffsll(__ballot(admissible && est == low)) - 1;
                if (take < 0 || low < take_est) take = __shfl(span, who), take_est = low;
            }
            if (__ballot(rest)) {                                     // the one whose most recent entry is the oldest
                const int low = __builtin_amdgcn_readfirstlane(wave_min(rest ? recent : 0x7fffffff));
                const int who = __ffsll(__ballot(rest && recent == low)) - 1;
                if (forced < 0 || low < forced_age) forced = __shfl(span, who), forced_est = __shfl(est, who), forced_age = low;
            }
        }
        if (take < 0) take = forced, take_est = forced_est;
        take = __builtin_amdgcn_readfirstlane(take), take_est = __builtin_amdgcn_readfirstlane(take_est);
        if (take < 0) {                                               // marks, and every candidate screened
            stop = 3;
            break;
        }
        const int from = take & 0xfff, to = (take >> 12) & 0xfff;
        const bool back = (take >> 24) != 0;
        const int xy = __builtin_amdgcn_readfirstlane((int)w.seq[back ? to : from] << 16 | (int)w.seq[back ? from : to]);
        const int x = xy >> 16, y = xy & 0xffff;
        rotate(w, from, to, back);
        const int mk = __builtin_amdgcn_readfirstlane(forward_pass<true>(w));   // the exact re-timing, and the next move's starts
        if (mk < 0) {                                                 // (unreachable: the screen) the move undone
            rotate(w, from, to, !back);
            stop = 4;
            break;
        }
        far += to - from >= 2 ? 1 : 0, hits += take_est == mk ? 1 : 0;
        cur = mk, moves = t;
        if (lane == ((t - 1) & 63)) {                                 // the lane that keeps the move's list entry also writes its words
            list_key = imin(x, y) << 16 | imax(x, y);
            if (trace) trace[t - 1] = cur;
            if (moved) moved[2 * (t - 1)] = x, moved[2 * (t - 1) + 1] = y;
        }
        if (cur < best) {
            best = cur, best_move = t;
            write_positions(w, p.best_rank + (size_t)i * region, jmax);
        }
        if (best <= target) stop = 2;
    }

    // ---- the end -------------------------------------------------------------------------------------------------------------
    const int late = lanes_below(~0ull);
    if (late == 0) p.best_makespan[i] = best;
    if (p.info && late < JSS_BLOCK_NI)
        p.info[i * JSS_BLOCK_NI + late] = late == 0 ? stop : late == 1 ? moves : late == 2 ? best_move : late == 3 ? evaluations
                                        : late == 4 ? screened : late == 5 ? far : late == 6 ? hits : 0;
    if (p.last_rank) write_positions(w, p.last_rank + (size_t)i * region, jmax);
    if (trace)
        for (int x = moves + lane; x < p.iters; x += kWave) trace[x] = -1;
    if (moved)
        for (int x = 2 * moves + lane; x < 2 * p.iters; x += kWave) moved[x] = -1;
}

}  // namespace

extern "C" {

int jss_block_search(const JssDesc *desc, const JssState *state, const JssBlock *b, void *stream) {
    if (const int rc = jss_abi::check_block_search(desc, state, b)) return rc;
    if (desc->batch == 0) return 0;
    BlockParams p;
    p.env_const = state->env_const, p.ops = desc->ops, p.rank = b->rank, p.tenure_of = b->tenure_of, p.target = b->target;
    p.best_makespan = b->best_makespan, p.best_rank = b->best_rank, p.last_rank = b->last_rank, p.info = b->info, p.trace = b->trace;
    p.move_log = b->move_log;
    p.iters = b->iters, p.tenure = b->tenure, p.reach = b->reach;
    p.batch = desc->batch, p.jmax = desc->jmax, p.mmax = desc->mmax, p.n_tables = desc->n_tables;
    const long long bytes = jss_abi::block_lds_bytes(desc->jmax, desc->mmax);
    p.entries8 = (int32_t)jss_abi::order_entries8(desc->jmax, desc->mmax);
    p.wave_lds_ints = (int32_t)(bytes / 4);
    // wavefronts per workgroup: they only share the LDS allocation, and small allocations pack a CU's 160 KB better
    p.waves_per_block = 4 * bytes <= 32 * 1024 ? 4 : 2 * bytes <= 32 * 1024 ? 2 : 1;
    const size_t shmem = (size_t)bytes * p.waves_per_block;          // at most 64 KB (check_block_search): no function attribute to raise
    const long long blocks = ((long long)desc->batch + p.waves_per_block - 1) / p.waves_per_block;
    hipLaunchKernelGGL(jss_block_kernel, dim3((unsigned)blocks), dim3((unsigned)(kWave * p.waves_per_block)), shmem,
                       reinterpret_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

}  // extern "C"
