// jssenv_amd/csrc/jss_propagate.hip -- libjss_propagate_hip.so: jss_propagate (include/jss_propagate.h), constraint propagation on
// the operation windows of a partial selection under a trial makespan, one candidate per wavefront in one launch on the MI355X.
// A library of its own: the other HIP libraries and their kernels are not touched by it (the device helpers it has in common
// with jss_machine.hip -- setup, the sort of the fixed machines, the forward and backward passes -- are written out again here
// for that reason).  It shares jss_abi_checks.hpp (the argument checks and the LDS a candidate needs) with the host-core twin,
// which carries the same entry point.
//
// The kernel has jss_machine.hip's form: one wavefront per candidate; the parent, J, M and the fixed mask are wave-uniform, and
// everything a branch or a loop around a cross-lane operation depends on is wave-uniform, so every way out takes the whole
// wavefront.  No workgroup barrier: the wavefronts of a workgroup only share its LDS allocation, each with a region of its own
// (propagate_lds_bytes), and the host picks 4, 2 or 1 of them per workgroup by that size.  What is new:
//
//   a pass    a Jacobi step over two generations of est[] and lct[] in LDS: one lane per operation (the positions of the
//             machine-major sequences strided over the lanes) reads the old generation only and writes its own operation's entries
//             of the new one, so a pass needs no atomic and no order.  An operation of a fixed machine takes its machine
//             neighbours from the machine's rank-sorted segment; an operation of a free machine runs the pairwise rule over its
//             machine's segment and, for the task intervals, two sweeps per threshold: under every upper end lct(b) the segment by
//             descending est with the running P and max(est + P) -- every prefix is the W of a pair of thresholds, and what is no
//             counting pair of the header is dominated by one (the same deduction under a weaker condition) -- and over every
//             lower end est(a) the segment by ascending lct with the running min(lct - P).  O(n^2) per lane and O(n^3 / 64) per
//             machine and pass.  The overload test rides on the first sweep.  A sweep serves four ends at once: the segment is
//             read once for them, and four independent running sums hide the LDS latency that one wavefront per SIMD cannot.
//   LDS       jss_machine.hip's op row, rank row and two sequence rows; the heads and tails are made in generation 0 of est[] and
//             lct[] and turned into the windows in place; the segments of the free machines in seq[] hold them by descending est, a
//             third row by ascending lct, both re-sorted every pass by counting.
//
// Every loop is bounded (by the budget and the operation counts); every index into LDS is the flat index of an entry of the row, a
// position of a segment or a machine number below 64.  No scratch memory, no spilled registers, LDS only as dynamic allocation of
// at most 64 KB (tests/test_propagate.py reads the code object's notes); only vector stores; only what the tests' SIMT emulator
// provides is used, so the unmodified source runs there.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "jss_abi_checks.hpp"

namespace {

constexpr int kWave = 64;
constexpr int kDurMask = 0xffff;
constexpr int kNever = 0x7fffffff;
constexpr int kEnds = 4;            // the ends of task intervals one sweep over a segment serves

// what the kernel reads of (desc, state, pr): the members by value, so that the kernel's arguments stay few
struct PropagateParams {
    const int32_t *env_const, *ops, *parents, *rank, *ub, *est_in, *lct_in, *hyp_op, *hyp_est, *hyp_lct;
    const uint64_t *fixed;
    int32_t *status, *passes_used, *est, *lct;
    int32_t n, stride, win_stride, passes, batch, jmax, mmax, n_tables;
    int32_t waves_per_block;
    int32_t wave_lds_ints;        // propagate_lds_bytes / 4
    int32_t entries8;             // order_entries8
};

// one wavefront's LDS and the candidate's shape
struct Rows {
    int32_t *m_off, *m_cnt, *m_cur, *m_rel;      // one word per machine: segment start and length, cursor, release / tail
    int32_t *opw, *rk;                           // by flat index
    int32_t *head, *tail;                        // generation 0 of est[] and lct[]: the heads and tails until the start
    int32_t *est1, *lct1;                        // generation 1
    uint16_t *slot, *seq, *seql;                 // machine-major flat indices: by flat index; by (rank, flat index) on fixed
                                                 // machines and by descending est on free ones; by ascending lct on free ones
    int J, M, mmax, total, lane;
};

__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }

// LDS writes of one wave consumed by other lanes of the same wave
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// (every control reads a valid lane of the row, so bound_ctrl never takes effect; with it set the move folds into its consumer)
#define JSS_DPP(v, ctrl) __builtin_amdgcn_update_dpp((v), (v), (ctrl), 0xF, 0xF, true)

// max over the 64 lanes, wave-uniform: four DPP steps within the rows of 16, the four rows combined on the scalar unit
__device__ __forceinline__ int wave_max(int v) {
    v = imax(v, JSS_DPP(v, 0xB1));   // quad_perm [1,0,3,2]   lane ^ 1
    v = imax(v, JSS_DPP(v, 0x4E));   // quad_perm [2,3,0,1]   lane ^ 2
    v = imax(v, JSS_DPP(v, 0x141));  // row_half_mirror       (quads are uniform by now)
    v = imax(v, JSS_DPP(v, 0x140));  // row_mirror
    const int a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
    const int c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
    return imax(imax(a, b), imax(c, d));
}

__device__ __forceinline__ unsigned long long uniform64(unsigned long long v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return (unsigned long long)hi << 32 | lo;
}

__device__ __forceinline__ bool has(unsigned long long mask, int m) { return (mask >> (m & 63)) & 1ull; }

__device__ __forceinline__ bool in_range(int v) { return v >= 0 && v <= JSS_PROPAGATE_MAX_TIME; }

// The candidate's LDS and its shape; the op row and the rank row loaded, the segments made.  0, or -1: refused.  *used: the
// machines with operations.
__device__ __forceinline__ int setup(const PropagateParams &p, int32_t *lds, long long c, const int32_t *rank, unsigned long long fixed,
                                     Rows &w, unsigned long long *used) {
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    const int parent = __builtin_amdgcn_readfirstlane(p.parents ? p.parents[c] : (int)c);
    if (parent < 0 || parent >= p.batch) return -1;
    const int jmax = p.jmax, mmax = p.mmax, region = jmax * mmax;
    const int32_t *ec = p.env_const + (size_t)parent * JSS_NC;
    const int J = __builtin_amdgcn_readfirstlane(ec[JSS_C_JOBS]), M = __builtin_amdgcn_readfirstlane(ec[JSS_C_MACHINES]);
    const int tab = __builtin_amdgcn_readfirstlane(ec[JSS_C_TABLE]);
    // (J == 0: never reset.  The rest holds for every env a reset has written; it keeps the walks inside the rows)
    if (!(J >= 1 && J <= jmax && M >= 1 && M <= mmax && tab >= 0 && tab < p.n_tables)) return -1;
    if (M < 64 && (fixed >> M)) return -1;
    const int32_t *ops = p.ops + (size_t)tab * region;

    int32_t *mine = lds + (size_t)wv * p.wave_lds_ints;
    w.m_off = mine, w.m_cnt = mine + kWave, w.m_cur = mine + 2 * kWave, w.m_rel = mine + 3 * kWave;
    w.opw = mine + 4 * kWave, w.rk = w.opw + p.entries8, w.head = w.rk + p.entries8, w.tail = w.head + p.entries8;
    w.est1 = w.tail + p.entries8, w.lct1 = w.est1 + p.entries8;
    w.slot = reinterpret_cast<uint16_t *>(w.lct1 + p.entries8), w.seq = w.slot + p.entries8, w.seql = w.seq + p.entries8;
    w.J = J, w.M = M, w.mmax = mmax, w.total = J * M, w.lane = lane;

    w.m_cnt[lane] = 0, w.m_cur[lane] = 0;
    wave_lds_sync();
    bool bad = false;
#pragma unroll 1
    for (int e = lane; e < region; e += kWave) {
        const int j = e / mmax, k = e - j * mmax;
        const int r = rank ? rank[e] : 0, o = ops[e];
        w.rk[e] = r;
        if (j < J && k < M) {
            const int m = (o >> 16) & 63;
            bad |= r < 0 && has(fixed, m);
            w.opw[e] = o;
            atomicAdd(&w.m_cnt[m], 1);
        }
    }
    if (__ballot(bad)) return -1;
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
        *used = __ballot(mine_cnt > 0 && lane < mmax);
    }
    wave_lds_sync();
    // dealt in arrival order into seq[], then placed by flat index into slot[]
#pragma unroll 1
    for (int e = lane; e < region; e += kWave) {
        const int j = e / mmax, k = e - j * mmax;
        if (j < J && k < M) {
            const int m = (w.opw[e] >> 16) & 63;
            w.seq[w.m_off[m] + atomicAdd(&w.m_cur[m], 1)] = (uint16_t)e;
        }
    }
    wave_lds_sync();
#pragma unroll 1
    for (int i = lane; i < w.total; i += kWave) {
        const int x = w.seq[i], m = (w.opw[x] >> 16) & 63;
        const int lo = w.m_off[m], hi = lo + w.m_cnt[m];
        int pos = 0;
#pragma unroll 1
        for (int t = lo; t < hi; ++t) pos += (int)w.seq[t] < x ? 1 : 0;
        w.slot[lo + pos] = (uint16_t)x;
    }
    wave_lds_sync();
    return 0;
}

// seq[] of the machines in `need`: their segments by (rank, flat index)
__device__ __forceinline__ void sort_machines(const Rows &w, unsigned long long need) {
#pragma unroll 1
    while (need) {
        const int m = __ffsll(need) - 1;
        need &= need - 1;
        const int lo = __builtin_amdgcn_readfirstlane(w.m_off[m]), n = __builtin_amdgcn_readfirstlane(w.m_cnt[m]);
#pragma unroll 1
        for (int i = w.lane; i < n; i += kWave) {
            const int x = w.slot[lo + i], r = w.rk[x];
            int pos = 0;
#pragma unroll 1
            for (int t = 0; t < n; ++t) {
                const int y = w.slot[lo + t], ry = w.rk[y];
                pos += (ry < r || (ry == r && y < x)) ? 1 : 0;
            }
            w.seq[lo + pos] = (uint16_t)x;
        }
    }
    wave_lds_sync();
}

// the heads of (rk, fixed) into head[]; returns the length, or -2: cyclic
__device__ __forceinline__ int forward(const Rows &w, unsigned long long fixed) {
    const int lane = w.lane, J = w.J, M = w.M, mmax = w.mmax;
    w.m_cur[lane] = w.m_off[lane], w.m_rel[lane] = 0;
    wave_lds_sync();
    int next_k[2] = {0, 0}, job_end[2] = {0, 0}, op_now[2] = {0, 0};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int j = s * kWave + lane;
        if (j < J) op_now[s] = w.opw[j * mmax];
    }
    int left = w.total;
#pragma unroll 1
    while (left > 0) {
        bool ready[2] = {false, false};
        int fired = 0;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (s * kWave >= J) break;
            const int j = s * kWave + lane;
            if (j < J && next_k[s] < M) {
                const int m = (op_now[s] >> 16) & 63;
                ready[s] = !has(fixed, m) || (int)w.seq[w.m_cur[m]] == j * mmax + next_k[s];
            }
            fired += __popcll(__ballot(ready[s]));                    // (all lanes have looked before any lane writes)
        }
        if (fired == 0) return -2;                                    // operations remain and none can start: a cycle
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (!ready[s]) continue;
            const int j = s * kWave + lane, m = (op_now[s] >> 16) & 63, x = j * mmax + next_k[s];
            const bool tied = has(fixed, m);
            const int st = tied ? imax(job_end[s], w.m_rel[m]) : job_end[s];
            w.head[x] = st;
            job_end[s] = st + (op_now[s] & kDurMask);
            if (tied) w.m_rel[m] = job_end[s], w.m_cur[m] += 1;
            next_k[s] += 1;
            if (next_k[s] < M) op_now[s] = w.opw[x + 1];
        }
        left -= fired;
        wave_lds_sync();
    }
    return wave_max(imax(job_end[0], job_end[1]));
}

// the tails of (rk, fixed) into tail[], behind a forward pass of the same selection that found no cycle
__device__ __forceinline__ void backward(const Rows &w, unsigned long long fixed) {
    const int lane = w.lane, J = w.J, M = w.M, mmax = w.mmax;
    w.m_cur[lane] = w.m_off[lane] + w.m_cnt[lane] - 1, w.m_rel[lane] = 0;
    wave_lds_sync();
    int next_k[2] = {M - 1, M - 1}, job_tail[2] = {0, 0}, op_now[2] = {0, 0};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int j = s * kWave + lane;
        if (j < J) op_now[s] = w.opw[j * mmax + M - 1];
    }
    int left = w.total;
#pragma unroll 1
    while (left > 0) {
        bool ready[2] = {false, false};
        int fired = 0;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (s * kWave >= J) break;
            const int j = s * kWave + lane;
            if (j < J && next_k[s] >= 0) {
                const int m = (op_now[s] >> 16) & 63;
                ready[s] = !has(fixed, m) || (int)w.seq[w.m_cur[m]] == j * mmax + next_k[s];
            }
            fired += __popcll(__ballot(ready[s]));
        }
        if (fired == 0) break;                                        // (cannot happen behind a forward pass that ended)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (!ready[s]) continue;
            const int j = s * kWave + lane, m = (op_now[s] >> 16) & 63, x = j * mmax + next_k[s];
            const bool tied = has(fixed, m);
            const int tl = tied ? imax(job_tail[s], w.m_rel[m]) : job_tail[s];
            w.tail[x] = tl;
            job_tail[s] = (op_now[s] & kDurMask) + tl;
            if (tied) w.m_rel[m] = job_tail[s], w.m_cur[m] -= 1;
            next_k[s] -= 1;
            if (next_k[s] >= 0) op_now[s] = w.opw[x - 1];
        }
        left -= fired;
        wave_lds_sync();
    }
}

// a [jmax][mmax] row of the outputs from a row of LDS, -1 in the padding
__device__ __forceinline__ void write_row(const Rows &w, int32_t *out, const int32_t *of, int region) {
#pragma unroll 1
    for (int e = w.lane; e < region; e += kWave) {
        const int j = e / w.mmax, k = e - j * w.mmax;
        out[e] = j < w.J && k < w.M ? of[e] : -1;
    }
}

// the free machines' segments of seq[] by descending est and of seql[] by ascending lct (the flat index breaks ties: any order
// of equal values gives the same pass), one lane per position, by counting
__device__ __forceinline__ void sort_windows(const Rows &w, unsigned long long fixed, const int32_t *est, const int32_t *lct) {
#pragma unroll 1
    for (int i = w.lane; i < w.total; i += kWave) {
        const int x = w.slot[i], m = (w.opw[x] >> 16) & 63;
        if (has(fixed, m)) continue;
        const int lo = w.m_off[m], hi = lo + w.m_cnt[m], ex = est[x], lx = lct[x];
        int above = 0, below = 0;
#pragma unroll 1
        for (int t = lo; t < hi; ++t) {
            const int y = w.slot[t], ey = est[y], ly = lct[y];
            above += (ey > ex || (ey == ex && y < x)) ? 1 : 0;
            below += (ly < lx || (ly == lx && y < x)) ? 1 : 0;
        }
        w.seq[lo + above] = (uint16_t)x, w.seql[lo + below] = (uint16_t)x;
    }
    wave_lds_sync();
}

// One pass of include/jss_propagate.h from (est, lct) into (est_new, lct_new): bit 0 of the result is set when a task interval
// is overloaded or a window closed, bit 1 when a window moved.  Wave-uniform.
__device__ __forceinline__ int one_pass(const Rows &w, unsigned long long fixed, const int32_t *est, const int32_t *lct, int32_t *est_new,
                                        int32_t *lct_new) {
    const int M = w.M, mmax = w.mmax;
    bool dead = false, moved = false;
#pragma unroll 1
    for (int i = w.lane; i < w.total; i += kWave) {
        const int at = w.slot[i], m = (w.opw[at] >> 16) & 63;
        const int lo = w.m_off[m], hi = lo + w.m_cnt[m];
        const bool tied = has(fixed, m);
        const int x = tied ? (int)w.seq[i] : at;
        const int ex = est[x], lx = lct[x], dx = w.opw[x] & kDurMask;
        int ne = ex, nl = lx;
        if (tied) {                                                   // 2. the machine's order
            if (i > lo) {
                const int u = w.seq[i - 1];
                ne = imax(ne, est[u] + (w.opw[u] & kDurMask));
            }
            if (i + 1 < hi) {
                const int v = w.seq[i + 1];
                nl = imin(nl, lct[v] - (w.opw[v] & kDurMask));
            }
        } else if (dx > 0) {
#pragma unroll 1
            for (int t = lo; t < hi; ++t) {                           // 3. pairs
                const int y = w.slot[t], dy = w.opw[y] & kDurMask;
                if (y == x || dy == 0) continue;
                const int ey = est[y], ly = lct[y];
                if (ex + dx + dy > ly) ne = imax(ne, ey + dy);
                if (ey + dy + dx > lx) nl = imin(nl, ly - dy);
            }
#pragma unroll 1
            for (int b = lo; b < hi; b += kEnds) {                    // 4. under every upper end, by descending est
                int L[kEnds], P[kEnds], E[kEnds];
#pragma unroll
                for (int u = 0; u < kEnds; ++u) {                     // (an end past the segment or of duration 0 holds no operation)
                    const int ob = w.slot[imin(b + u, hi - 1)];
                    L[u] = b + u < hi && (w.opw[ob] & kDurMask) != 0 ? lct[ob] : -kNever;
                    P[u] = 0, E[u] = -kNever;
                }
#pragma unroll 2
                for (int t = lo; t < hi; ++t) {
                    const int y = w.seq[t], dy = w.opw[y] & kDurMask, e = est[y], ly = lct[y];
                    if (dy == 0) continue;
#pragma unroll
                    for (int u = 0; u < kEnds; ++u) {
                        if (ly <= L[u]) P[u] += dy, E[u] = imax(E[u], e + P[u]);
                        if (P[u] == 0) continue;
                        dead |= e + P[u] > L[u];
                        if ((ex < e || lx > L[u]) && imin(e, ex) + P[u] + dx > L[u]) ne = imax(ne, E[u]);
                    }
                }
            }
#pragma unroll 1
            for (int a = lo; a < hi; a += kEnds) {                    //    over every lower end, by ascending lct
                int A[kEnds], P[kEnds], F[kEnds];
#pragma unroll
                for (int u = 0; u < kEnds; ++u) {
                    const int oa = w.slot[imin(a + u, hi - 1)];
                    A[u] = a + u < hi && (w.opw[oa] & kDurMask) != 0 ? est[oa] : kNever;
                    P[u] = 0, F[u] = kNever;
                }
#pragma unroll 2
                for (int t = lo; t < hi; ++t) {
                    const int y = w.seql[t], dy = w.opw[y] & kDurMask, ey = est[y], L = lct[y];
                    if (dy == 0) continue;
#pragma unroll
                    for (int u = 0; u < kEnds; ++u) {
                        if (ey >= A[u]) P[u] += dy, F[u] = imin(F[u], L - P[u]);
                        if (P[u] == 0) continue;
                        if ((ex < A[u] || lx > L) && A[u] + P[u] + dx > imax(L, lx)) nl = imin(nl, F[u]);
                    }
                }
            }
        }
        const int k = x % mmax;                                       // 1. the job
        if (k > 0) ne = imax(ne, est[x - 1] + (w.opw[x - 1] & kDurMask));
        if (k + 1 < M) nl = imin(nl, lct[x + 1] - (w.opw[x + 1] & kDurMask));
        est_new[x] = ne, lct_new[x] = nl;
        moved |= ne != ex || nl != lx;
        dead |= ne + dx > nl;
    }
    const int result = (__ballot(dead) ? 1 : 0) | (__ballot(moved) ? 2 : 0);
    wave_lds_sync();
    return result;
}

__global__ __launch_bounds__(256) void jss_propagate_kernel(PropagateParams p) {
    HIP_DYNAMIC_SHARED(int32_t, lds)

    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    const long long c = (long long)blockIdx.x * p.waves_per_block + wv;
    if (c >= p.n) return;                                             // (the whole wavefront, like every return below)
    const unsigned long long fixed = p.fixed ? uniform64(p.fixed[c]) : 0ull;
    const int region = p.jmax * p.mmax;
    Rows w;
    unsigned long long used = 0;
    int refused = setup(p, lds, c, p.rank ? p.rank + (size_t)c * p.stride : nullptr, fixed, w, &used);
    const int ub = __builtin_amdgcn_readfirstlane(p.ub[c]);
    const int hyp = p.hyp_op ? __builtin_amdgcn_readfirstlane(p.hyp_op[c]) : -1;
    int hyp_est = 0, hyp_lct = kNever;
    const int32_t *est_in = p.est_in ? p.est_in + (size_t)c * p.win_stride : nullptr;
    const int32_t *lct_in = p.lct_in ? p.lct_in + (size_t)c * p.win_stride : nullptr;
    if (refused == 0) {
        bool bad = !in_range(ub);
        if (hyp >= 0) {
            hyp_est = __builtin_amdgcn_readfirstlane(p.hyp_est[c]), hyp_lct = __builtin_amdgcn_readfirstlane(p.hyp_lct[c]);
            bad |= hyp >= region || hyp / p.mmax >= w.J || hyp % p.mmax >= w.M || !in_range(hyp_est) || !in_range(hyp_lct);
        }
        if (est_in) {
#pragma unroll 1
            for (int e = lane; e < region; e += kWave) {
                const int j = e / p.mmax, k = e - j * p.mmax;
                if (j < w.J && k < w.M) bad |= !in_range(est_in[e]) || !in_range(lct_in[e]);
            }
        }
        if (__ballot(bad)) refused = -1;
    }
    if (refused < 0) {
        if (lane == 0) p.status[c] = -1;
        return;
    }
    sort_machines(w, fixed & used);
    if (forward(w, fixed) < 0) {
        if (lane == 0) p.status[c] = -2;
        return;
    }
    backward(w, fixed);
    // the start: the windows in place of the heads and tails
    bool closed = false;
#pragma unroll 1
    for (int e = lane; e < region; e += kWave) {
        const int j = e / p.mmax, k = e - j * p.mmax;
        if (j < w.J && k < w.M) {
            int est = w.head[e], lct = ub - w.tail[e];
            if (est_in) est = imax(est, est_in[e]), lct = imin(lct, lct_in[e]);
            if (e == hyp) est = imax(est, hyp_est), lct = imin(lct, hyp_lct);
            w.head[e] = est, w.tail[e] = lct;
            closed |= est + (w.opw[e] & kDurMask) > lct;
        }
    }
    wave_lds_sync();
    int status = __ballot(closed) ? JSS_PROPAGATE_REFUTED : JSS_PROPAGATE_BUDGET, pass = 0;
    int32_t *est = w.head, *lct = w.tail, *est_new = w.est1, *lct_new = w.lct1;
#pragma unroll 1
    while (status == JSS_PROPAGATE_BUDGET && pass < p.passes) {
        pass += 1;
        sort_windows(w, fixed, est, lct);
        const int result = one_pass(w, fixed, est, lct, est_new, lct_new);
        int32_t *t = est;
        est = est_new, est_new = t;
        t = lct, lct = lct_new, lct_new = t;
        status = (result & 1) ? JSS_PROPAGATE_REFUTED : (result & 2) ? JSS_PROPAGATE_BUDGET : JSS_PROPAGATE_FIXPOINT;
    }
    if (lane == 0) {
        p.status[c] = status;
        if (p.passes_used) p.passes_used[c] = pass;
    }
    if (status == JSS_PROPAGATE_REFUTED) return;
    if (p.est) write_row(w, p.est + (size_t)c * region, est, region);
    if (p.lct) write_row(w, p.lct + (size_t)c * region, lct, region);
}

}  // namespace

extern "C" {

int jss_propagate(const JssDesc *desc, const JssState *state, const JssPropagate *pr, void *stream) {
    if (const int rc = jss_abi::propagate_check(desc, state, pr)) return rc;
    if (pr->n == 0) return 0;
    PropagateParams p = {};
    p.env_const = state->env_const, p.parents = pr->parents, p.rank = pr->rank, p.fixed = pr->fixed, p.ub = pr->ub;
    p.est_in = pr->est_in, p.lct_in = pr->lct_in, p.hyp_op = pr->hyp_op, p.hyp_est = pr->hyp_est, p.hyp_lct = pr->hyp_lct;
    p.status = pr->status, p.passes_used = pr->passes_used, p.est = pr->est, p.lct = pr->lct;
    p.n = pr->n, p.stride = pr->stride, p.win_stride = pr->win_stride, p.passes = pr->passes;
    const long long bytes = jss_abi::propagate_lds_bytes(desc->jmax, desc->mmax);
    p.batch = desc->batch, p.jmax = desc->jmax, p.mmax = desc->mmax, p.n_tables = desc->n_tables, p.ops = desc->ops;
    p.entries8 = (int32_t)jss_abi::order_entries8(desc->jmax, desc->mmax);
    p.wave_lds_ints = (int32_t)(bytes / 4);
    // wavefronts per workgroup: they only share the LDS allocation, and small allocations pack a CU's 160 KB better
    p.waves_per_block = 4 * bytes <= 32 * 1024 ? 4 : 2 * bytes <= 32 * 1024 ? 2 : 1;
    const size_t shmem = (size_t)bytes * p.waves_per_block;          // at most 64 KB (the checks): no function attribute to raise
    const long long blocks = ((long long)p.n + p.waves_per_block - 1) / p.waves_per_block;
    hipLaunchKernelGGL(jss_propagate_kernel, dim3((unsigned)blocks), dim3((unsigned)(kWave * p.waves_per_block)), shmem,
                       reinterpret_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

}  // extern "C"
