// jssenv_amd/csrc/jss_order.hip -- libjss_order_hip.so: jss_order_eval and jss_order_apply (include/jss_order.h), the exact
// schedule of a machine order and one descent step's bookkeeping on the MI355X.  A library of its own: libjss_hip.so,
// libjss_beam_hip.so, libjss_bound_hip.so and their kernels are not touched by it.  It shares jss_abi_checks.hpp (the argument
// checks and the LDS a candidate needs) with the host-core twin, which carries the same entry points.
//
// jss_order_eval_kernel: one wavefront per candidate, in the caller's order; the parent and the swap are read once and made
// wave-uniform, so every way out of the kernel takes the whole wavefront.  Job j sits on lane j % 64, slot j / 64 (two slots
// beyond 64 jobs).  No workgroup barrier is used: the wavefronts of a workgroup only share its LDS allocation, each with a
// region of its own (order_lds_bytes), and the host picks 4, 2 or 1 of them per workgroup by that size.  The semantics are the
// header's; the form:
//
//   1. a coalesced pass over the row: the op words into LDS, a negative rank of a real operation noted, the machines'
//      operation counts by atomicAdd; a wave scan turns the counts into the machines' offsets.
//   2. a second pass deals the operations into their machines' segments in arrival order, each with its rank -- the swap is made
//      here, in registers: the two entries take each other's rank on the way in.
//   3. every entry counts the entries of its segment with a smaller (rank, flat index), four at a time: that is its position,
//      and seq[] -- machine-major, position ascending -- holds the order.
//   4. forward, in rounds: a job whose next operation is the one at its machine's cursor starts it at max(job end, machine
//      release) and moves both on.  One operation per machine per round at most, so the writes do not collide; a round in which
//      nothing fired while operations remain is a cycle.
//   5. backward, the mirror image, for the tails.  The operation behind on the machine was placed in an earlier round and has
//      left, per machine, its start if it is critical: the operation in front knows then whether the two form a pair, and marks
//      its position.
//   6. the marks are listed with a ballot prefix count: seq[] is already in the order the header lists pairs in.
//
// start[] and tail[] are written from LDS in coalesced passes (padding -1).  No scratch memory, no spilled registers, LDS only
// as dynamic allocation of at most 64 KB (tests/test_order.py reads the code object's notes); only vector stores; only what the
// tests' SIMT emulator provides is used, so the unmodified source runs there.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "jss_abi_checks.hpp"

namespace {

constexpr int kWave = 64;
constexpr int kDurMask = 0xffff;
constexpr int kNone = 0x7fffffff;
constexpr int kApplyThreads = 256;
constexpr int kApplyWaves = kApplyThreads / kWave;

// what the kernel reads of (desc, state, o): the members by value, so that the kernel's arguments stay few
struct OrderParams {
    const int32_t *env_const, *ops, *rank, *parent, *swap_a, *swap_b;
    int32_t *makespan, *start, *tail, *pair_a, *pair_b, *n_pairs;
    int32_t n, pair_cap, batch, jmax, mmax, n_tables;
    int32_t waves_per_block;
    int32_t wave_lds_ints;        // order_lds_bytes / 4
    int32_t entries8;             // order_entries8
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

__global__ __launch_bounds__(256) void jss_order_eval_kernel(OrderParams p) {
    HIP_DYNAMIC_SHARED(int32_t, lds)

    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    const long long c = (long long)blockIdx.x * p.waves_per_block + wv;
    if (c >= p.n) return;                                           // (the whole wavefront, like every return below)
    const int parent = __builtin_amdgcn_readfirstlane(p.parent ? p.parent[c] : (int)c);
    const int swap_a = __builtin_amdgcn_readfirstlane(p.swap_a ? p.swap_a[c] : -1);
    const int swap_b = __builtin_amdgcn_readfirstlane(p.swap_b ? p.swap_b[c] : -1);
    const int jmax = p.jmax, mmax = p.mmax, region = jmax * mmax;

    bool ok = parent >= 0 && parent < p.batch;
    int J = 0, M = 0, tab = 0;
    if (ok) {
        const int32_t *ec = p.env_const + (size_t)parent * JSS_NC;
        J = ec[JSS_C_JOBS], M = ec[JSS_C_MACHINES], tab = ec[JSS_C_TABLE];
        // (J == 0: never reset.  The rest holds for every env a reset has written; it keeps the walks inside the rows)
        ok = J >= 1 && J <= jmax && M >= 1 && M <= mmax && tab >= 0 && tab < p.n_tables;
    }
    const bool swaps = swap_a != -1 || swap_b != -1;
    if (ok && swaps) {
        ok = swap_a >= 0 && swap_a < region && swap_b >= 0 && swap_b < region;
        if (ok) ok = swap_a / mmax < J && swap_a % mmax < M && swap_b / mmax < J && swap_b % mmax < M;
    }
    if (!ok) {
        if (lane == 0) p.makespan[c] = -1;
        return;
    }
    const int total = J * M;
    const int32_t *rank = p.rank + (size_t)parent * region;
    const int32_t *ops = p.ops + (size_t)tab * region;

    // this wavefront's LDS: two int32 rows and two uint16 rows over the entries, five blocks of one word per machine
    int32_t *mine = lds + (size_t)wv * p.wave_lds_ints;
    int32_t *val = mine;                                              // ranks in segment order -> start, by flat index -> tail
    int32_t *opw = val + p.entries8;                                  // the op words, by flat index
    uint16_t *slot = reinterpret_cast<uint16_t *>(opw + p.entries8);  // segment order: flat indices as dealt -> the pair marks
    uint16_t *seq = slot + p.entries8;                                // segment order: flat indices by position
    int32_t *m_off = reinterpret_cast<int32_t *>(seq + p.entries8);   // the machines' segments: first entry ...
    int32_t *m_cnt = m_off + kWave;                                   // ... and length
    int32_t *m_cur = m_cnt + kWave;                                   // dealing: entries taken; passes: the cursor into seq[]
    int32_t *m_rel = m_cur + kWave;                                   // forward: release time; backward: d + tail of the last one
    int32_t *m_crit = m_rel + kWave;                                  // backward: the last one's start if it is critical, else -1

    // ---- 1. op words, rank check, counts, offsets ---------------------------------------------------------------------
    m_cnt[lane] = 0, m_cur[lane] = 0;
    wave_lds_sync();
    bool bad = false;
#pragma unroll 1
    for (int e = lane; e < region; e += kWave) {
        const int j = e / mmax, k = e - j * mmax;
        const int r = rank[e], o = ops[e];
        if (j < J && k < M) {
            bad |= r < 0;
            opw[e] = o;
            atomicAdd(&m_cnt[(o >> 16) & 63], 1);
        }
    }
    if (__ballot(bad)) {
        if (lane == 0) p.makespan[c] = -1;
        return;
    }
    wave_lds_sync();
    {
        const int mine_cnt = m_cnt[lane];
        int incl = mine_cnt;
#pragma unroll
        for (int dlt = 1; dlt < kWave; dlt <<= 1) {
            const int below = __shfl(incl, (lane - dlt) & 63);
            if (lane >= dlt) incl += below;
        }
        m_off[lane] = incl - mine_cnt;
    }
    wave_lds_sync();
    // ---- 2. deal the operations into their machines' segments, the swap made on the way ------------------------------------
    int rank_a = 0, rank_b = 0;
    if (swaps) rank_a = rank[swap_a], rank_b = rank[swap_b];
#pragma unroll 1
    for (int e = lane; e < region; e += kWave) {
        const int j = e / mmax, k = e - j * mmax;
        int r = rank[e];
        if (swaps) r = e == swap_a ? rank_b : e == swap_b ? rank_a : r;
        if (j < J && k < M) {
            const int m = (opw[e] >> 16) & 63;
            const int at = m_off[m] + atomicAdd(&m_cur[m], 1);
            slot[at] = (uint16_t)e, val[at] = r;
        }
    }
    wave_lds_sync();
    // ---- 3. positions: the entries of the segment with a smaller (rank, flat index) -----------------------------------------
#pragma unroll 1
    for (int i = lane; i < total; i += kWave) {
        const int x = slot[i], r = val[i], m = (opw[x] >> 16) & 63;
        const int lo = m_off[m], hi = lo + m_cnt[m];
        int pos = 0;
#pragma unroll 1
        for (int t = lo; t < hi; t += 4) {
            int y[4], ry[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int at = imin(t + u, hi - 1);                   // (clamped, not branched around: the loads go out together)
                y[u] = slot[at], ry[u] = val[at];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) pos += (t + u < hi && (ry[u] < r || (ry[u] == r && y[u] < x))) ? 1 : 0;
        }
        seq[lo + pos] = (uint16_t)x;
    }
    wave_lds_sync();                                                  // (val[] and slot[] are free from here)

    // ---- 4. forward ---------------------------------------------------------------------------------------------------------
    m_cur[lane] = m_off[lane], m_rel[lane] = 0;
    wave_lds_sync();
    int next_k[2] = {0, 0}, job_end[2] = {0, 0}, op_now[2] = {0, 0};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int j = s * kWave + lane;
        if (j < J) op_now[s] = opw[j * mmax];
    }
    int left = total;
#pragma unroll 1
    while (left > 0) {
        bool ready[2] = {false, false};
        int fired = 0;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (s * kWave >= J) break;
            const int j = s * kWave + lane;
            if (j < J && next_k[s] < M) ready[s] = seq[m_cur[(op_now[s] >> 16) & 63]] == j * mmax + next_k[s];
            fired += __popcll(__ballot(ready[s]));                    // (all lanes have looked before any lane writes)
        }
        if (fired == 0) {                                             // operations remain and none can start: a cycle
            if (lane == 0) p.makespan[c] = -2;
            return;
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (!ready[s]) continue;
            const int j = s * kWave + lane, m = (op_now[s] >> 16) & 63, x = j * mmax + next_k[s];
            const int st = imax(job_end[s], m_rel[m]);
            val[x] = st;
            job_end[s] = st + (op_now[s] & kDurMask);
            m_rel[m] = job_end[s], m_cur[m] += 1;
            next_k[s] += 1;
            if (next_k[s] < M) op_now[s] = opw[x + 1];
        }
        left -= fired;
        wave_lds_sync();
    }
    const int makespan = wave_max(imax(job_end[0], job_end[1]));
    if (lane == 0) p.makespan[c] = makespan;
    if (p.start) {
        int32_t *out = p.start + (size_t)c * region;
    #pragma unroll 1
    for (int e = lane; e < region; e += kWave) {
            const int j = e / mmax, k = e - j * mmax;
            out[e] = j < J && k < M ? val[e] : -1;
        }
    }
    if (!p.tail && !p.pair_a) return;

    // ---- 5. backward: tails, critical operations, pair marks -----------------------------------------------------------------
    m_cur[lane] = m_off[lane] + m_cnt[lane] - 1, m_rel[lane] = 0, m_crit[lane] = -1;
    wave_lds_sync();
    int job_tail[2] = {0, 0};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int j = s * kWave + lane;
        next_k[s] = M - 1;
        if (j < J) op_now[s] = opw[j * mmax + M - 1];
    }
    left = total;
#pragma unroll 1
    while (left > 0) {
        bool ready[2] = {false, false};
        int fired = 0;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (s * kWave >= J) break;
            const int j = s * kWave + lane;
            if (j < J && next_k[s] >= 0) ready[s] = seq[m_cur[(op_now[s] >> 16) & 63]] == j * mmax + next_k[s];
            fired += __popcll(__ballot(ready[s]));
        }
        if (fired == 0) break;                                        // (cannot happen behind a forward pass that ended)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (!ready[s]) continue;
            const int j = s * kWave + lane, m = (op_now[s] >> 16) & 63, x = j * mmax + next_k[s];
            const int dur = op_now[s] & kDurMask, at = m_cur[m];
            const int st = val[x], tl = imax(job_tail[s], m_rel[m]);
            const bool critical = st + dur + tl == makespan;
            // the operation behind on the machine: critical and starting as this one ends -- then of another job?
            bool pair = critical && m_crit[m] == st + dur && at + 1 < m_off[m] + m_cnt[m];
            if (pair) pair = (int)seq[at + 1] / mmax != j;
            slot[at] = pair ? 1 : 0;
            val[x] = tl;
            job_tail[s] = dur + tl;
            m_rel[m] = dur + tl, m_crit[m] = critical ? st : -1, m_cur[m] = at - 1;
            next_k[s] -= 1;
            if (next_k[s] >= 0) op_now[s] = opw[x - 1];
        }
        left -= fired;
        wave_lds_sync();
    }
    if (p.tail) {
        int32_t *out = p.tail + (size_t)c * region;
    #pragma unroll 1
    for (int e = lane; e < region; e += kWave) {
            const int j = e / mmax, k = e - j * mmax;
            out[e] = j < J && k < M ? val[e] : -1;
        }
    }
    if (!p.pair_a) return;
    // ---- 6. the pairs, machine by machine and position by position: the order of seq[] -----------------------------------------
    const int cap = p.pair_cap;
    int32_t *pa = p.pair_a + (size_t)c * cap, *pb = p.pair_b + (size_t)c * cap;
    int found = 0;
#pragma unroll 1
    for (int i0 = 0; i0 < total; i0 += kWave) {
        const int i = i0 + lane;
        const bool marked = i < total && slot[i] != 0;
        const unsigned long long mask = __ballot(marked);
        const int at = found + lanes_below(mask);
        if (marked && at < cap) pa[at] = seq[i], pb[at] = seq[i + 1];   // (a mark has an entry of its segment behind it)
        found += __popcll(mask);
    }
    for (int i = found + lane; i < cap; i += kWave) pa[i] = -1, pb[i] = -1;
    if (lane == 0) p.n_pairs[c] = found;
}

// jss_order_apply: one wavefront per env; the lanes share out the candidates, two wave-wide minima give the lowest
// (makespan, index), lane 0 exchanges the two ranks.
__global__ __launch_bounds__(kApplyThreads) void jss_order_apply_kernel(JssOrderApply a) {
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    const long long i = (long long)blockIdx.x * kApplyWaves + wv;
    if (i >= a.batch) return;
    const int cap = a.pair_cap, region = a.jmax * a.mmax;
    const int32_t *mk = a.makespan + (size_t)i * cap, *pa = a.pair_a + (size_t)i * cap, *pb = a.pair_b + (size_t)i * cap;
    int best = kNone, best_at = kNone;
    for (int k = lane; k < cap; k += kWave) {
        const int v = mk[k], x = pa[k], y = pb[k];
        if (v >= 0 && x >= 0 && x < region && y >= 0 && y < region && v < best) best = v, best_at = k;   // (k ascends: ties keep the first)
    }
    const int low = wave_min(best);
    const int at = wave_min(best == low ? best_at : kNone);
    if (lane == 0) {
        int took = 0;
        if (low != kNone && low < a.cur[i]) {
            int32_t *row = a.rank + (size_t)i * region;
            const int x = pa[at], y = pb[at];
            const int rx = row[x], ry = row[y];
            row[x] = ry, row[y] = rx;
            a.cur[i] = low;
            took = 1;
        }
        a.improved[i] = took;
    }
}

}  // namespace

extern "C" {

int jss_order_eval(const JssDesc *desc, const JssState *state, const JssOrder *o, void *stream) {
    if (const int rc = jss_abi::check_order_eval(desc, state, o)) return rc;
    if (o->n == 0) return 0;
    OrderParams p;
    p.env_const = state->env_const, p.ops = desc->ops, p.rank = o->rank, p.parent = o->parent, p.swap_a = o->swap_a, p.swap_b = o->swap_b;
    p.makespan = o->makespan, p.start = o->start, p.tail = o->tail, p.pair_a = o->pair_a, p.pair_b = o->pair_b, p.n_pairs = o->n_pairs;
    p.n = o->n, p.pair_cap = o->pair_cap, p.batch = desc->batch, p.jmax = desc->jmax, p.mmax = desc->mmax, p.n_tables = desc->n_tables;
    const long long bytes = jss_abi::order_lds_bytes(desc->jmax, desc->mmax);
    p.entries8 = (int32_t)jss_abi::order_entries8(desc->jmax, desc->mmax);
    p.wave_lds_ints = (int32_t)(bytes / 4);
    // wavefronts per workgroup: they only share the LDS allocation, and small allocations pack a CU's 160 KB better
    p.waves_per_block = 4 * bytes <= 32 * 1024 ? 4 : 2 * bytes <= 32 * 1024 ? 2 : 1;
    const size_t shmem = (size_t)bytes * p.waves_per_block;          // at most 64 KB (check_order_eval): no function attribute to raise
    const long long blocks = ((long long)o->n + p.waves_per_block - 1) / p.waves_per_block;
    hipLaunchKernelGGL(jss_order_eval_kernel, dim3((unsigned)blocks), dim3((unsigned)(kWave * p.waves_per_block)), shmem,
                       reinterpret_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

int jss_order_apply(const JssOrderApply *a, void *stream) {
    if (const int rc = jss_abi::check_order_apply(a)) return rc;
    if (a->batch == 0) return 0;
    hipLaunchKernelGGL(jss_order_apply_kernel, dim3((unsigned)((a->batch + kApplyWaves - 1) / kApplyWaves)), dim3(kApplyThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), *a);
    return (int)hipGetLastError();
}

}  // extern "C"
