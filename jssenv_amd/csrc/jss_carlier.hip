// jssenv_amd/csrc/jss_carlier.hip -- libjss_carlier_hip.so: jss_machine_solve and jss_bottleneck_exact (include/jss_carlier.h),
// Carlier's branch and bound for the one-machine problems of a partial selection and a whole shifting bottleneck construction that
// sequences its machines with it, one candidate per wavefront in one launch on the MI355X.  A library of its own: the other HIP
// libraries and their kernels are not touched by it (the device helpers it has in common with jss_machine.hip -- setup, the sorts,
// the forward and backward passes, Jackson's and Schrage's schedules -- are written out again here for that reason).  It shares
// jss_abi_checks.hpp (the argument checks and the LDS a candidate needs) with the host-core twin, which carries the same entry
// points.
//
// Both kernels have jss_machine.hip's form: one wavefront per candidate; the parent, J, M and the fixed mask are wave-uniform, and
// everything a branch or a loop around a cross-lane operation depends on is wave-uniform, so every way out takes the whole
// wavefront.  No workgroup barrier: the wavefronts of a workgroup only share its LDS allocation, each with a region of its own
// (carlier_lds_bytes), and the host picks 4, 2 or 1 of them per workgroup by that size.  What is new:
//
//   the search   include/jss_carlier.h's node() without recursion: a state machine over NODE (count it, run Schrage's schedule,
//             find b, a, c and J, push a frame with the first child applied -- or set `open` where the budget or the depth is spent), EVAL (Jackson's preemptive value of the problem as
//             modified; enter the child, or set `open` where the budget forbids that) and ADVANCE (undo the top
//             frame's change; apply its second child, or pop).  The working r and q are the head[] and tail[] entries of the
//             machine's operations, raised by lane 0 and restored from the frame, so that when the search ends the rows hold the
//             relaxation again.  Every decision is a reduction result: b, a and the block's end fall out of Schrage's loop as
//             wave-uniform scalars, c, min r and min q of J are one strided pass and a reduction each, the sum of J's durations
//             is s[b] + p[b] - s[c+1] (the block has no idle time).
//   LDS       jss_machine.hip's rows; Schrage's starts of the current node go to tmp[] by position (free again when Jackson's
//             schedule runs on the children: by then c and J are scalars), its order to the machine's segment of seq[], which
//             only fixed machines use; the best starts have a row of their own, bst[]; the frames are three words each.
//
// Every loop is bounded (by the budget, the depth cap and the operation counts); every index into LDS is the flat index of an
// entry of the row, a position of a segment, a machine number below 64 or a frame below JSS_CARLIER_MAX_DEPTH.  No scratch memory,
// no spilled registers, LDS only as dynamic allocation of at most 64 KB (tests/test_carlier.py reads the code object's notes);
// only vector stores; only what the tests' SIMT emulator provides is used, so the unmodified source runs there.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "jss_abi_checks.hpp"

namespace {

constexpr int kWave = 64;
constexpr int kDurMask = 0xffff;
constexpr int kNever = 0x7fffffff;

constexpr int kDepth = JSS_CARLIER_MAX_DEPTH;

// what the kernels read of (desc, state, ms / be): the members by value, so that the kernels' arguments stay few.  The build
// writes its makespans through `length` and its orders through `rank_out`.
struct MachineParams {
    const int32_t *env_const, *ops, *parents, *rank, *bias;
    const uint64_t *fixed;
    int32_t *length, *lower_bound, *bottleneck, *opt, *low, *nodes_used, *head, *tail, *rank_out, *info, *order;
    uint64_t *proved;
    int32_t n, stride, reopt, nodes, batch, jmax, mmax, n_tables;
    int32_t waves_per_block;
    int32_t wave_lds_ints;        // carlier_lds_bytes / 4
    int32_t entries8;             // order_entries8
};

// one wavefront's LDS and the candidate's shape
struct Rows {
    int32_t *m_off, *m_cnt, *m_cur, *m_rel;      // one word per machine: segment start and length, cursor, release / tail
    int32_t *f_op, *f_old, *f_alt;               // one word per frame: operation | child << 16, the value it replaced, child 1's value
    int32_t *opw, *rk, *head, *tail;             // by flat index
    int32_t *tmp, *bst;                          // by position: remaining times, a node's starts, saved ranks; the best starts
    uint16_t *slot, *seq;                        // machine-major flat indices: by flat index, by (rank, flat index); of the
                                                 // machine being solved, seq[] holds the positions in Schrage's order
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

// min / max over the 64 lanes, wave-uniform: four DPP steps within the rows of 16, the four rows combined on the scalar unit
__device__ __forceinline__ int wave_min(int v) {
    v = imin(v, JSS_DPP(v, 0xB1));   // quad_perm [1,0,3,2]   lane ^ 1
    v = imin(v, JSS_DPP(v, 0x4E));   // quad_perm [2,3,0,1]   lane ^ 2
    v = imin(v, JSS_DPP(v, 0x141));  // row_half_mirror       (quads are uniform by now)
    v = imin(v, JSS_DPP(v, 0x140));  // row_mirror
    const int a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
    const int c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
    return imin(imin(a, b), imin(c, d));
}

__device__ __forceinline__ int wave_max(int v) {
    v = imax(v, JSS_DPP(v, 0xB1));
    v = imax(v, JSS_DPP(v, 0x4E));
    v = imax(v, JSS_DPP(v, 0x141));
    v = imax(v, JSS_DPP(v, 0x140));
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

// The candidate's LDS and its shape; the op row and the rank row loaded, the segments made.  0, or -1: refused.  *used: the
// machines with operations.
__device__ __forceinline__ int setup(const MachineParams &p, int32_t *lds, long long c, const int32_t *rank, unsigned long long fixed,
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
    w.f_op = mine + 4 * kWave, w.f_old = w.f_op + kDepth, w.f_alt = w.f_old + kDepth;
    w.opw = w.f_alt + kDepth, w.rk = w.opw + p.entries8, w.head = w.rk + p.entries8, w.tail = w.head + p.entries8;
    w.tmp = w.tail + p.entries8, w.bst = w.tmp + p.entries8;
    w.slot = reinterpret_cast<uint16_t *>(w.bst + p.entries8), w.seq = w.slot + p.entries8;
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

// the value of Jackson's preemptive schedule of machine m's operations, from head[] and tail[]; tmp[] holds the remaining times
// (-1: finished) by position
__device__ __forceinline__ int jackson(const Rows &w, int m) {
    const int lane = w.lane;
    const int lo = __builtin_amdgcn_readfirstlane(w.m_off[m]), n = __builtin_amdgcn_readfirstlane(w.m_cnt[m]);
    int first = kNever;
#pragma unroll 1
    for (int i = lane; i < n; i += kWave) {
        const int x = w.slot[lo + i];
        w.tmp[lo + i] = w.opw[x] & kDurMask;
        first = imin(first, w.head[x]);
    }
    int t = wave_min(first), left = n, value = 0;
    wave_lds_sync();
#pragma unroll 1
    for (int it = 0; it < 3 * n + 3 && left > 0; ++it) {             // (a decision finishes an operation or reaches a release)
        int q_high = -1, at = kNever, later = kNever;
#pragma unroll 1
        for (int i = lane; i < n; i += kWave) {
            if (w.tmp[lo + i] < 0) continue;
            const int x = w.slot[lo + i], r = w.head[x];
            if (r > t) {
                later = imin(later, r);
            } else if (w.tail[x] > q_high) {
                q_high = w.tail[x], at = i;
            }
        }
        const int q = wave_max(q_high), next = wave_min(later);
        if (q < 0) {                                                  // nothing released is unfinished: on to the next release
            if (next == kNever) break;
            t = next;
            continue;
        }
        const int pos = wave_min(q_high == q ? at : kNever);
        const int rem = __builtin_amdgcn_readfirstlane(w.tmp[lo + pos]);
        const int run = next == kNever ? rem : imin(rem, next - t);
        t += run;
        if (run == rem) left -= 1, value = imax(value, t + q);
        if (lane == 0) w.tmp[lo + pos] = run == rem ? -1 : rem - run;
        wave_lds_sync();
    }
    return value;
}

// Schrage's schedule of machine m's operations, from head[] and tail[]: the starts into rk[], the value returned
__device__ __forceinline__ int schrage(const Rows &w, int m) {
    const int lane = w.lane;
    const int lo = __builtin_amdgcn_readfirstlane(w.m_off[m]), n = __builtin_amdgcn_readfirstlane(w.m_cnt[m]);
    int first = kNever;
#pragma unroll 1
    for (int i = lane; i < n; i += kWave) first = imin(first, w.head[w.slot[lo + i]]);
    int t = wave_min(first), left = n, value = 0;
    unsigned long long done = 0;                                      // bit s: position lane + 64 * s is scheduled
#pragma unroll 1
    for (int it = 0; it < 2 * n + 2 && left > 0; ++it) {             // (a decision schedules an operation or reaches a release)
        int q_high = -1, at = kNever, later = kNever;
#pragma unroll 1
        for (int i = lane, s = 0; i < n; i += kWave, ++s) {
            if ((done >> s) & 1ull) continue;
            const int x = w.slot[lo + i], r = w.head[x];
            if (r > t) {
                later = imin(later, r);
            } else if (w.tail[x] > q_high) {
                q_high = w.tail[x], at = i;
            }
        }
        const int q = wave_max(q_high), next = wave_min(later);
        if (q < 0) {
            if (next == kNever) break;
            t = next;
            continue;
        }
        const int pos = wave_min(q_high == q ? at : kNever);
        const int x = __builtin_amdgcn_readfirstlane((int)w.slot[lo + pos]);
        const int d = __builtin_amdgcn_readfirstlane(w.opw[x]) & kDurMask;
        if (lane == (pos & 63)) done |= 1ull << (pos >> 6), w.rk[x] = t;
        value = imax(value, t + d + q);
        t += d, left -= 1;
    }
    wave_lds_sync();
    return value;
}

// a [jmax][mmax] row of the outputs from a row of LDS, -1 in the padding
__device__ __forceinline__ void write_row(const Rows &w, int32_t *out, const int32_t *of, int region) {
#pragma unroll 1
    for (int e = w.lane; e < region; e += kWave) {
        const int j = e / w.mmax, k = e - j * w.mmax;
        out[e] = j < w.J && k < w.M ? of[e] : -1;
    }
}


// What a node of the search reads off Schrage's schedule, all wave-uniform: the value; b, the lowest position that reaches it,
// with its start, duration and tail; a, the start of b's block without idle time.
struct Critical {
    int value, b, a, s_b, p_b, q_b;
};

// Schrage's schedule of machine m's operations as jss_machine.h defines it, from head[] and tail[]: the starts into tmp[] by
// position of the segment, the positions in the order they were scheduled into the machine's segment of seq[]
__device__ __forceinline__ Critical schrage_ordered(const Rows &w, int m) {
    const int lane = w.lane;
    const int lo = __builtin_amdgcn_readfirstlane(w.m_off[m]), n = __builtin_amdgcn_readfirstlane(w.m_cnt[m]);
    int first = kNever;
#pragma unroll 1
    for (int i = lane; i < n; i += kWave) first = imin(first, w.head[w.slot[lo + i]]);
    int t = wave_min(first), at_k = 0, block = 0;
    Critical cr = {-1, 0, 0, 0, 0, 0};
    unsigned long long done = 0;                                      // bit s: position lane + 64 * s is scheduled
#pragma unroll 1
    for (int it = 0; it < 2 * n + 2 && at_k < n; ++it) {             // (a decision schedules an operation or reaches a release)
        int q_high = -1, at = kNever, later = kNever;
#pragma unroll 1
        for (int i = lane, s = 0; i < n; i += kWave, ++s) {
            if ((done >> s) & 1ull) continue;
            const int x = w.slot[lo + i], r = w.head[x];
            if (r > t) {
                later = imin(later, r);
            } else if (w.tail[x] > q_high) {
                q_high = w.tail[x], at = i;
            }
        }
        const int q = wave_max(q_high), next = wave_min(later);
        if (q < 0) {                                                  // idle until the next release: a new block begins
            if (next == kNever) break;
            t = next, block = at_k;
            continue;
        }
        const int pos = wave_min(q_high == q ? at : kNever);
        const int x = __builtin_amdgcn_readfirstlane((int)w.slot[lo + pos]);
        const int d = __builtin_amdgcn_readfirstlane(w.opw[x]) & kDurMask;
        if (lane == (pos & 63)) done |= 1ull << (pos >> 6), w.tmp[lo + pos] = t, w.seq[lo + at_k] = (uint16_t)pos;
        if (t + d + q > cr.value) cr.value = t + d + q, cr.b = at_k, cr.a = block, cr.s_b = t, cr.p_b = d, cr.q_b = q;
        t += d, at_k += 1;
    }
    wave_lds_sync();
    return cr;
}

struct Solved {
    int best, count;
    bool open;
};

// include/jss_carlier.h's search on machine m, whose Jackson value of the relaxation the caller has: the best starts into bst[]
// by position.  head[] and tail[] of m's operations are raised and restored; tmp[] and m's segment of seq[] are overwritten.
__device__ __forceinline__ Solved carlier(const Rows &w, int m, int budget) {
    enum { kNode, kEval, kAdvance };
    const int lane = w.lane;
    const int lo = __builtin_amdgcn_readfirstlane(w.m_off[m]), n = __builtin_amdgcn_readfirstlane(w.m_cnt[m]);
    Solved sv = {kNever, 0, false};
    int state = kNode, sp = 0;                                        // sp frames: the node at hand lies at depth sp + 1
#pragma unroll 1
    for (int it = 0; it < 8 * budget + 4 * kDepth; ++it) {           // (a node costs one kNode, two kEval, three kAdvance at most)
        if (state == kNode) {
            sv.count += 1;
            const Critical cr = schrage_ordered(w, m);
            if (cr.value < sv.best) {
                sv.best = cr.value;
#pragma unroll 1
                for (int i = lane; i < n; i += kWave) w.bst[lo + i] = w.tmp[lo + i];
            }
            // c: the highest position in [a, b) with a tail below b's
            int c_high = -1;
#pragma unroll 1
            for (int k = cr.a + lane; k < cr.b; k += kWave)
                if (w.tail[w.slot[lo + w.seq[lo + k]]] < cr.q_b) c_high = k;
            const int c = wave_max(c_high);
            state = kAdvance;
            if (c < 0) continue;                                      // solved
            int r_low = kNever, q_low = kNever;
#pragma unroll 1
            for (int k = c + 1 + lane; k <= cr.b; k += kWave) {
                const int x = w.slot[lo + w.seq[lo + k]];
                r_low = imin(r_low, w.head[x]), q_low = imin(q_low, w.tail[x]);
            }
            const int rJ = wave_min(r_low), qJ = wave_min(q_low);
            const int i_c = __builtin_amdgcn_readfirstlane((int)w.seq[lo + c]), i_n = __builtin_amdgcn_readfirstlane((int)w.seq[lo + c + 1]);
            const int pJ = cr.s_b + cr.p_b - __builtin_amdgcn_readfirstlane(w.tmp[lo + i_n]);   // (no idle time between c + 1 and b)
            const int xc = __builtin_amdgcn_readfirstlane((int)w.slot[lo + i_c]);
            const int r_c = __builtin_amdgcn_readfirstlane(w.head[xc]), q_c = __builtin_amdgcn_readfirstlane(w.tail[xc]);
            const int p_c = __builtin_amdgcn_readfirstlane(w.opw[xc]) & kDurMask;
            if (imax(rJ + pJ + qJ, imin(rJ, r_c) + pJ + p_c + imin(qJ, q_c)) >= sv.best) continue;
            if (sv.count >= budget || sp + 1 >= kDepth) {             // no child of this node could be entered
                sv.open = true;
                continue;
            }
            // a frame with the first child applied: c before J
            wave_lds_sync();                                          // (every lane has read the tails before one is raised)
            if (lane == 0) w.f_op[sp] = xc, w.f_old[sp] = q_c, w.f_alt[sp] = rJ + pJ, w.tail[xc] = imax(q_c, pJ + qJ);
            sp += 1, state = kEval;
            wave_lds_sync();
        } else if (state == kEval) {
            state = kAdvance;
            if (jackson(w, m) < sv.best) {
                if (sv.count + 1 > budget) sv.open = true;
                else state = kNode;
            }
        } else {
            if (sp == 0) break;
            const int f = __builtin_amdgcn_readfirstlane(w.f_op[sp - 1]), old = __builtin_amdgcn_readfirstlane(w.f_old[sp - 1]);
            const int xc = f & 0xffff, child = f >> 16;
            wave_lds_sync();
            if (child == 0 && !sv.open) {                             // c after J
                const int r_c = __builtin_amdgcn_readfirstlane(w.head[xc]), alt = __builtin_amdgcn_readfirstlane(w.f_alt[sp - 1]);
                if (lane == 0) w.tail[xc] = old, w.f_op[sp - 1] = xc | 1 << 16, w.f_old[sp - 1] = r_c, w.head[xc] = imax(r_c, alt);
                state = kEval;
            } else {
                if (lane == 0) (child == 0 ? w.tail : w.head)[xc] = old;
                sp -= 1;
            }
            wave_lds_sync();
        }
    }
    wave_lds_sync();
    return sv;
}

// the best starts of machine m as its operations' ranks; the ranks they replace into tmp[] by position
__device__ __forceinline__ void take_best(const Rows &w, int m) {
    const int lo = __builtin_amdgcn_readfirstlane(w.m_off[m]), n = __builtin_amdgcn_readfirstlane(w.m_cnt[m]);
#pragma unroll 1
    for (int i = w.lane; i < n; i += kWave) {
        const int x = w.slot[lo + i];
        w.tmp[lo + i] = w.rk[x], w.rk[x] = w.bst[lo + i];
    }
    wave_lds_sync();
}

__global__ __launch_bounds__(256) void jss_machine_solve_kernel(MachineParams p) {
    HIP_DYNAMIC_SHARED(int32_t, lds)

    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    const long long c = (long long)blockIdx.x * p.waves_per_block + wv;
    if (c >= p.n) return;                                             // (the whole wavefront, like every return below)
    const unsigned long long fixed = p.fixed ? uniform64(p.fixed[c]) : 0ull;
    const int region = p.jmax * p.mmax;
    Rows w;
    unsigned long long used = 0;
    if (setup(p, lds, c, p.rank ? p.rank + (size_t)c * p.stride : nullptr, fixed, w, &used) < 0) {
        if (lane == 0) p.length[c] = -1;
        return;
    }
    sort_machines(w, fixed & used);
    const int length = forward(w, fixed);
    if (lane == 0) p.length[c] = length;
    if (length < 0) return;
    backward(w, fixed);
    int my_opt = -1, my_low = -1, my_nodes = -1, best = -1, neck = -1;
    unsigned long long open = used & ~fixed, proved = 0;
#pragma unroll 1
    while (open) {
        const int m = __ffsll(open) - 1;
        open &= open - 1;
        const int v = jackson(w, m);
        const Solved sv = carlier(w, m, p.nodes);
        const int low = sv.open ? v : sv.best;
        if (!sv.open) proved |= 1ull << m;
        if (p.rank_out) take_best(w, m);
        if (lane == m) my_opt = sv.best, my_low = low, my_nodes = sv.count;
        if (low > best) best = low, neck = m;
    }
    if (lane == 0) {
        if (p.lower_bound) p.lower_bound[c] = imax(length, best);
        if (p.bottleneck) p.bottleneck[c] = neck;
        if (p.proved) p.proved[c] = proved;
    }
    if (lane < p.mmax) {
        if (p.opt) p.opt[c * p.mmax + lane] = my_opt;
        if (p.low) p.low[c * p.mmax + lane] = my_low;
        if (p.nodes_used) p.nodes_used[c * p.mmax + lane] = my_nodes;
    }
    if (p.head) write_row(w, p.head + (size_t)c * region, w.head, region);
    if (p.tail) write_row(w, p.tail + (size_t)c * region, w.tail, region);
    if (p.rank_out) write_row(w, p.rank_out + (size_t)c * region, w.rk, region);
}

// what a build counts of its searches
struct Tally {
    int total, most, open, replaced;
};

// Machine k, free in the relaxation the rows hold (heads and tails of `fixed` without k's bit), sequenced by the search's best
// schedule, by Schrage's where that selection is cyclic: the length of the selection with k.  tmp[] keeps k's old ranks.
__device__ __forceinline__ int sequence(const Rows &w, int k, unsigned long long fixed, int budget, Tally &tally) {
    const unsigned long long k_bit = 1ull << k;
    const Solved sv = carlier(w, k, budget);
    tally.total += sv.count, tally.most = imax(tally.most, sv.count), tally.open += sv.open ? 1 : 0;
    take_best(w, k);
    sort_machines(w, k_bit);
    int length = forward(w, fixed);
    if (length == -2) {
        tally.replaced += 1;
        forward(w, fixed & ~k_bit);                                   // (the heads again; the tails were not touched)
        schrage(w, k);
        sort_machines(w, k_bit);
        length = forward(w, fixed);
    }
    return length;
}

__global__ __launch_bounds__(256) void jss_bottleneck_exact_kernel(MachineParams p) {
    HIP_DYNAMIC_SHARED(int32_t, lds)

    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    const long long c = (long long)blockIdx.x * p.waves_per_block + wv;
    if (c >= p.n) return;                                             // (the whole wavefront, like every return below)
    unsigned long long fixed = p.fixed ? uniform64(p.fixed[c]) : 0ull;
    const int region = p.jmax * p.mmax, reopt = p.reopt, budget = p.nodes;
    Rows w;
    unsigned long long used = 0;
    if (setup(p, lds, c, p.rank ? p.rank + (size_t)c * region : nullptr, fixed, w, &used) < 0) {
        if (lane == 0) p.length[c] = -1;
        return;
    }
    sort_machines(w, fixed & used);
    int length = forward(w, fixed);
    int first = length, n_fixed = 0, tried = 0, shorter = 0, my_order = -1;
    Tally tally = {0, 0, 0, 0};
    bool at_start = true;
#pragma unroll 1
    while (length >= 0 && (used & ~fixed)) {
        backward(w, fixed);
        // 1. the bottleneck: the greatest (jps + bias, then lowest machine)
        int star = -1;
        long long high = 0;
        unsigned long long open = used & ~fixed;
#pragma unroll 1
        while (open) {
            const int m = __ffsll(open) - 1;
            open &= open - 1;
            const int v = jackson(w, m);
            if (at_start && p.info) {                                 // (the first bound is the searches': they are not tallied)
                const Solved sv = carlier(w, m, budget);
                first = imax(first, sv.open ? v : sv.best);
            }
            const long long biased = (long long)v + (p.bias ? __builtin_amdgcn_readfirstlane(p.bias[c * p.mmax + m]) : 0);
            if (star < 0 || biased > high) star = m, high = biased;
        }
        at_start = false;
        // 2. - 4. its best starts as ranks, its bit, the length
        const unsigned long long star_bit = 1ull << star;
        fixed |= star_bit;
        if (lane == n_fixed) my_order = star;
        n_fixed += 1;
        int cur = length = sequence(w, star, fixed, budget, tally);
        if (cur < 0) break;
        // 5. the machines fixed before, one after the other: freed, sequenced anew, kept if the schedule is no longer
#pragma unroll 1
        for (int round = 0; round < reopt; ++round) {
            unsigned long long others = fixed & ~star_bit;
#pragma unroll 1
            while (others) {
                const int k = __ffsll(others) - 1;
                const unsigned long long k_bit = 1ull << k;
                others &= others - 1;
                tried += 1;
                if (!(used & k_bit)) continue;                        // (a fixed machine without operations: nothing changes)
                if (forward(w, fixed & ~k_bit) < 0) continue;         // (cannot happen: fewer arcs than an acyclic selection)
                backward(w, fixed & ~k_bit);
                const int now = sequence(w, k, fixed, budget, tally);
                if (now >= 0 && now <= cur) {
                    shorter += now < cur ? 1 : 0, cur = now;
                } else {
                    const int lo = __builtin_amdgcn_readfirstlane(w.m_off[k]), n = __builtin_amdgcn_readfirstlane(w.m_cnt[k]);
#pragma unroll 1
                    for (int i = lane; i < n; i += kWave) w.rk[w.slot[lo + i]] = w.tmp[lo + i];
                    wave_lds_sync();
                    sort_machines(w, k_bit);
                }
            }
        }
        if (reopt > 0) length = forward(w, fixed);                    // (the heads of the selection as it stands)
    }
    if (lane == 0) p.length[c] = length;
    if (length < 0) return;
    write_row(w, p.rank_out + (size_t)c * region, w.rk, region);
    if (p.info && lane < JSS_EXACT_NI) {
        const int row[JSS_EXACT_NI] = {n_fixed, tried, shorter, first, tally.total, tally.most, tally.open, tally.replaced};
        int mine = 0;
#pragma unroll
        for (int i = 0; i < JSS_EXACT_NI; ++i) mine = lane == i ? row[i] : mine;
        p.info[c * JSS_EXACT_NI + lane] = mine;
    }
    if (p.order && lane < p.mmax) p.order[c * p.mmax + lane] = my_order;
}

// the launch both entry points share
template <typename Kernel>
int launch(Kernel kernel, const JssDesc *desc, MachineParams &p, void *stream) {
    const long long bytes = jss_abi::carlier_lds_bytes(desc->jmax, desc->mmax);
    p.batch = desc->batch, p.jmax = desc->jmax, p.mmax = desc->mmax, p.n_tables = desc->n_tables, p.ops = desc->ops;
    p.entries8 = (int32_t)jss_abi::order_entries8(desc->jmax, desc->mmax);
    p.wave_lds_ints = (int32_t)(bytes / 4);
    // wavefronts per workgroup: they only share the LDS allocation, and small allocations pack a CU's 160 KB better
    p.waves_per_block = 4 * bytes <= 32 * 1024 ? 4 : 2 * bytes <= 32 * 1024 ? 2 : 1;
    const size_t shmem = (size_t)bytes * p.waves_per_block;          // at most 64 KB (the checks): no function attribute to raise
    const long long blocks = ((long long)p.n + p.waves_per_block - 1) / p.waves_per_block;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3((unsigned)(kWave * p.waves_per_block)), shmem,
                       reinterpret_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int jss_machine_solve(const JssDesc *desc, const JssState *state, const JssMachineSolve *ms, void *stream) {
    if (const int rc = jss_abi::machine_solve_check(desc, state, ms)) return rc;
    if (ms->n == 0) return 0;
    MachineParams p = {};
    p.env_const = state->env_const, p.parents = ms->parents, p.rank = ms->rank, p.fixed = ms->fixed;
    p.length = ms->length, p.lower_bound = ms->lower_bound, p.bottleneck = ms->bottleneck;
    p.opt = ms->opt, p.low = ms->low, p.nodes_used = ms->nodes_used, p.proved = ms->proved;
    p.head = ms->head, p.tail = ms->tail, p.rank_out = ms->rank_out;
    p.n = ms->n, p.stride = ms->stride, p.nodes = ms->nodes;
    return launch(jss_machine_solve_kernel, desc, p, stream);
}

int jss_bottleneck_exact(const JssDesc *desc, const JssState *state, const JssBottleneckExact *be, void *stream) {
    if (const int rc = jss_abi::bottleneck_exact_check(desc, state, be)) return rc;
    if (be->n == 0) return 0;
    MachineParams p = {};
    p.env_const = state->env_const, p.parents = be->parents, p.rank = be->rank_in, p.fixed = be->fixed_in, p.bias = be->bias;
    p.length = be->makespan, p.rank_out = be->rank, p.info = be->info, p.order = be->order;
    p.n = be->n, p.reopt = be->reopt, p.nodes = be->nodes;
    return launch(jss_bottleneck_exact_kernel, desc, p, stream);
}

}  // extern "C"
