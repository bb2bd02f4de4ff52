// jssenv_amd/csrc/jss_beam.hip -- libjss_beam_hip.so: jss_beam_select (include/jss_beam.h), beam search's candidate selection
// on the MI355X.  A library of its own: libjss_hip.so and its kernels are not touched by it.  It shares jss_abi_checks.hpp
// (the argument check) with the host-core twin, which carries the same entry point.
//
// One 256-thread workgroup per group.  The semantics are the header's; the form:
//
//   1. one strided pass over the group's W * A candidates: the valid ones are appended to an LDS list as 64-bit keys
//      (makespan with its sign bit flipped, index within the group) -- ascending key order is the header's ORDER -- and the
//      running slots and the valid candidates are counted;
//   2. the list, padded to a power of two, is sorted in LDS (bitonic network, one barrier per stage);
//   3. each sorted entry's (steps, reward_num) is gathered next to it; an entry is a duplicate when an earlier entry of the
//      run of its makespan has the same pair -- the runs are short, every entry is tested on its own;
//   4. a workgroup prefix sum of the survivors ranks them: survivor r < W writes slot r, the slots left over are cleared and
//      next_parent follows.
//
// LDS capacity: the list holds kBeamCap = 2048 candidates (8 + 4 + 8 bytes each, 40 KB, 42 KB with the scan's words).  A beam
// of width 64 over 16 actions has 1024 candidates of which a few hundred are valid.  A group with MORE valid candidates than
// the list holds takes the rescanning path instead of 2. - 4.: one round per candidate in order, each round a pass over global
// memory for the smallest key above the last one taken and, with dedupe, a second one for a valid candidate of a lower
// index with an equal triple (the header's definition itself).  It is exact and slow (rounds x W * A / 256 loads per thread): it
// is there so that no shape the argument check admits is refused.
//
// No scratch memory, no spilled registers (tests/test_beam.py reads the code object's notes); only what the SIMT emulator of the
// tests provides is used (__shared__, __syncthreads, __shfl, atomicAdd on int), so the unmodified source runs there.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "jss_abi_checks.hpp"

namespace {

constexpr int kBeamThreads = 256;
constexpr int kBeamCap = 2048;
constexpr unsigned long long kNoKey = ~0ull;

__device__ __forceinline__ unsigned long long beam_key(int makespan, int c) {
    return ((unsigned long long)((unsigned)makespan ^ 0x80000000u) << 32) | (unsigned)c;
}
__device__ __forceinline__ int key_makespan(unsigned long long k) { return (int)((unsigned)(k >> 32) ^ 0x80000000u); }
__device__ __forceinline__ int key_cand(unsigned long long k) { return (int)(unsigned)k; }

// candidate (slot w of the group, action a): is it valid, and with which makespan (the header's table); *running: its slot is
__device__ __forceinline__ bool beam_valid(const JssBeam &b, int slot0, size_t cand0, int w, int a, int *makespan, bool *running) {
    const int s = slot0 + w;
    const int A = b.n_actions;
    *running = false;
    if (b.cand_parent[cand0 + (size_t)w * A] != s) return false;                 // a dead slot
    if (b.done[s]) {
        *makespan = b.env_makespan[s];
        return a == 0;
    }
    *running = true;
    *makespan = b.makespan[cand0 + (size_t)w * A + a];
    return *makespan >= 0;
}

// the triple's second and third member of candidate c of the group (valid, as beam_valid found it)
__device__ __forceinline__ void beam_pair(const JssBeam &b, int slot0, size_t cand0, int c, int *steps, long long *rnum) {
    const int w = c / b.n_actions;
    if (b.done[slot0 + w]) {
        *steps = 0;
        *rnum = 0;
    } else {
        *steps = b.steps[cand0 + c];
        *rnum = b.reward_num[cand0 + c];
    }
}

// smallest of the workgroup's keys, for every thread (two barriers; `red` holds kBeamThreads + 16 keys)
__device__ __forceinline__ unsigned long long beam_min(unsigned long long v, unsigned long long *red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    if (t < 16) {
        unsigned long long m = red[t * 16];
        for (int i = 1; i < 16; ++i) {
            const unsigned long long x = red[t * 16 + i];
            m = x < m ? x : m;
        }
        red[kBeamThreads + t] = m;
    }
    __syncthreads();
    unsigned long long m = red[kBeamThreads];
    for (int i = 1; i < 16; ++i) {
        const unsigned long long x = red[kBeamThreads + i];
        m = x < m ? x : m;
    }
    return m;
}

__global__ __launch_bounds__(kBeamThreads) void jss_beam_select_kernel(JssBeam b) {
    __shared__ unsigned long long key[kBeamCap];
    __shared__ long long pair_rnum[kBeamCap];
    __shared__ int pair_steps[kBeamCap];
    __shared__ unsigned long long red[kBeamThreads + 16];
    __shared__ int wave_sum[kBeamThreads / 64];
    __shared__ int n_list, n_running, n_dropped, dup_found;

    const int t = threadIdx.x, g = blockIdx.x;
    const int W = b.width, A = b.n_actions, n = W * A;                           // n <= 65536 (check_beam_select)
    const int slot0 = g * W;
    const size_t cand0 = (size_t)slot0 * A;
    const bool dedupe = (b.flags & JSS_BEAM_DEDUPE) != 0;
    const int step_w = kBeamThreads / A, step_a = kBeamThreads % A;              // a thread's walk over c = t, t + 256, ...

    if (t == 0) n_list = 0, n_running = 0, n_dropped = 0, dup_found = 0;
    __syncthreads();

    // ---- 1. the valid candidates, as keys ----------------------------------------------------------------------------
    {
        int w = t / A, a = t % A;
        for (int c = t; c < n; c += kBeamThreads) {
            int m;
            bool runs;
            const bool ok = beam_valid(b, slot0, cand0, w, a, &m, &runs);
            if (a == 0 && runs) atomicAdd(&n_running, 1);
            if (ok) {
                const int at = atomicAdd(&n_list, 1);
                if (at < kBeamCap) key[at] = beam_key(m, c);
            }
            w += step_w, a += step_a;
            if (a >= A) a -= A, ++w;
        }
    }
    __syncthreads();
    const int n_valid = n_list, running = n_running;

    if (running == 0) {                                                          // a finished group: left alone
        for (int c = t; c < n; c += kBeamThreads) b.next_parent[cand0 + c] = b.cand_parent[cand0 + c];
        for (int w = t; w < W; w += kBeamThreads) b.src[slot0 + w] = -1, b.action[slot0 + w] = JSS_ACTION_SKIP, b.score[slot0 + w] = -1;
        if (t < 4) b.counts[g * 4 + t] = 0;
        return;
    }

    int n_sel = 0;
    if (n_valid <= kBeamCap) {
        // ---- 2. sort ---------------------------------------------------------------------------------------------------
        int P = 2;
        while (P < n_valid) P <<= 1;
        for (int i = n_valid + t; i < P; i += kBeamThreads) key[i] = kNoKey;
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int q = t; q < (P >> 1); q += kBeamThreads) {
                    const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), p = i | j;
                    const unsigned long long x = key[i], y = key[p];
                    if ((x > y) == ((i & k) == 0)) key[i] = y, key[p] = x;
                }
                __syncthreads();
            }
        // ---- 3. the pairs, then the duplicates ----------------------------------------------------------------------------
        if (dedupe) {
            for (int i = t; i < n_valid; i += kBeamThreads) {
                int st;
                long long rn;
                beam_pair(b, slot0, cand0, key_cand(key[i]), &st, &rn);
                pair_steps[i] = st, pair_rnum[i] = rn;
            }
            __syncthreads();
        }
        // thread t owns the entries [t * L, t * L + L): a bit per entry that survives
        const int L = (n_valid + kBeamThreads - 1) / kBeamThreads;               // <= 8
        unsigned keep = 0;
        for (int q = 0; q < L; ++q) {
            const int i = t * L + q;
            if (i >= n_valid) break;
            bool dup = false;
            if (dedupe) {
                const unsigned hi = (unsigned)(key[i] >> 32);
                const int st = pair_steps[i];
                const long long rn = pair_rnum[i];
                for (int j = i - 1; j >= 0 && (unsigned)(key[j] >> 32) == hi; --j)
                    if (pair_steps[j] == st && pair_rnum[j] == rn) {
                        dup = true;
                        break;
                    }
            }
            keep |= (dup ? 0u : 1u) << q;
        }
        // ---- 4. rank the survivors, write the slots ----------------------------------------------------------------------
        const int mine = __popc(keep), lane = t & 63;
        int incl = mine;
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl(incl, (lane - d) & 63);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_sum[t >> 6] = incl;
        __syncthreads();
        int before = incl - mine, total = 0;
        for (int v = 0; v < kBeamThreads / 64; ++v) {
            if (v < (t >> 6)) before += wave_sum[v];
            total += wave_sum[v];
        }
        n_sel = total < W ? total : W;
        int rank = before, dropped = 0;
        for (int q = 0; q < L; ++q) {
            const int i = t * L + q;
            if (i >= n_valid) break;
            if ((keep >> q) & 1) {
                if (rank < W) {
                    const unsigned long long k = key[i];
                    const int c = key_cand(k), w = c / A, d = slot0 + rank;
                    b.src[d] = slot0 + w;
                    b.action[d] = b.done[slot0 + w] ? JSS_ACTION_SKIP : c - w * A;
                    b.score[d] = key_makespan(k);
                }
                ++rank;
            } else if (rank < W) {
                ++dropped;
            }
        }
        if (dropped) atomicAdd(&n_dropped, dropped);
        __syncthreads();
    } else {
        // ---- the rescanning path: one round per candidate in order ---------------------------------------------------------
        unsigned long long last = 0;
        bool first = true;
        int dropped = 0, dups_seen = 0;                                          // (dup_found only grows: no reset to order)
        while (n_sel < W) {
            unsigned long long best = kNoKey;
            int w = t / A, a = t % A;
            for (int c = t; c < n; c += kBeamThreads) {
                int m;
                bool runs;
                if (beam_valid(b, slot0, cand0, w, a, &m, &runs)) {
                    const unsigned long long k = beam_key(m, c);
                    if ((first || k > last) && k < best) best = k;
                }
                w += step_w, a += step_a;
                if (a >= A) a -= A, ++w;
            }
            best = beam_min(best, red);
            if (best == kNoKey) break;
            const int c_best = key_cand(best), m_best = key_makespan(best);
            bool dup = false;
            if (dedupe) {
                int st;
                long long rn;
                beam_pair(b, slot0, cand0, c_best, &st, &rn);
                bool found = false;
                w = t / A, a = t % A;
                for (int c = t; c < c_best; c += kBeamThreads) {
                    int m;
                    bool runs;
                    if (beam_valid(b, slot0, cand0, w, a, &m, &runs) && m == m_best) {
                        int st2;
                        long long rn2;
                        beam_pair(b, slot0, cand0, c, &st2, &rn2);
                        found = found || (st2 == st && rn2 == rn);
                    }
                    w += step_w, a += step_a;
                    if (a >= A) a -= A, ++w;
                }
                if (found) atomicAdd(&dup_found, 1);
                __syncthreads();
                const int seen = dup_found;
                dup = seen != dups_seen;
                dups_seen = seen;
            }
            if (dup) {
                ++dropped;
            } else {
                if (t == 0) {
                    const int ws = c_best / A, d = slot0 + n_sel;
                    b.src[d] = slot0 + ws;
                    b.action[d] = b.done[slot0 + ws] ? JSS_ACTION_SKIP : c_best - ws * A;
                    b.score[d] = m_best;
                }
                ++n_sel;
            }
            last = best, first = false;
        }
        if (t == 0) n_dropped = dropped;
        __syncthreads();
    }

    for (int w = n_sel + t; w < W; w += kBeamThreads) b.src[slot0 + w] = -1, b.action[slot0 + w] = JSS_ACTION_SKIP, b.score[slot0 + w] = -1;
    {
        int w = t / A, a = t % A;
        for (int c = t; c < n; c += kBeamThreads) {
            b.next_parent[cand0 + c] = w < n_sel ? slot0 + w : -1;
            w += step_w, a += step_a;
            if (a >= A) a -= A, ++w;
        }
    }
    if (t == 0) {
        b.counts[g * 4 + 0] = n_sel;
        b.counts[g * 4 + 1] = running;
        b.counts[g * 4 + 2] = n_dropped;
        b.counts[g * 4 + 3] = n_valid;
    }
}

}  // namespace

extern "C" {

int jss_beam_select(const JssBeam *b, void *stream) {
    if (const int rc = jss_abi::check_beam_select(b)) return rc;
    if (b->n_groups == 0) return 0;
    hipLaunchKernelGGL(jss_beam_select_kernel, dim3((unsigned)b->n_groups), dim3(kBeamThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), *b);
    return (int)hipGetLastError();
}

}  // extern "C"
