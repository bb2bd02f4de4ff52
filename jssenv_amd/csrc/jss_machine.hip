// jssenv_amd/csrc/jss_machine.hip -- libjss_machine_hip.so: jss_machine_relax and jss_bottleneck_build (include/jss_machine.h), the
// one-machine relaxations of a partial selection and a whole shifting bottleneck construction, one candidate per wavefront in one
// launch on the MI355X.  A library of its own: the other HIP libraries and their kernels are not touched by it (the device helpers
// it has in common with them are written out again here for that reason).  It shares jss_abi_checks.hpp (the argument checks and
// the LDS a candidate needs) with the host-core twin, which carries the same entry points.
//
// Both kernels: one wavefront per candidate; the parent, J, M and the fixed mask are made wave-uniform, and everything a branch or
// a loop around a cross-lane operation depends on is wave-uniform, so every way out takes the whole wavefront.  No workgroup
// barrier is used: the wavefronts of a workgroup only share its LDS allocation, each with a region of its own
// (machine_lds_bytes), and the host picks 4, 2 or 1 of them per workgroup by that size.  The semantics are the header's; the form:
//
//   setup     the op row and the rank row into LDS, a lane per entry; the machines' operation counts by atomicAdd, a wave scan
//             turns them into the machines' segments; the operations are dealt into their segments and sorted there by flat index
//             (slot[]: machine-major, the same on every run, so the lowest position is the lowest flat index).
//   sort      a fixed machine's segment ordered by (rank, flat index) by counting, into seq[]; only the machines whose ranks
//             changed since their last sort.
//   forward   job j on lane j % 64, slot j / 64.  In rounds: a job whose next operation is on a free machine, or is the one at
//             its fixed machine's cursor, starts it at max(job end, machine release).  One operation per fixed machine per round
//             at most, so the writes do not collide; a round in which nothing fired while operations remain is a cycle.
//   backward  the mirror image, for the tails.
//   one machine  its operations sit on the lanes, position i of the segment on lane i % 64 (strided beyond 64: a machine that
//             repeats within jobs can hold every operation).  Every decision of Jackson's preemptive schedule and of Schrage's
//             schedule is a scan of the lane's own positions and then wave-wide reductions over the ready set -- the largest tail,
//             the lowest position that holds it, the next release -- never a serial scan by one lane.  Jackson's schedule keeps the
//             remaining times in a scratch row; Schrage's keeps the scheduled positions in a 64-bit mask per lane.
//
// Every loop is bounded (by the operations left, and by a count of its own where it waits for releases); every index into LDS is
// the flat index of an entry of the row, a position of a segment or a machine number below 64.  No scratch memory, no spilled
// registers, LDS only as dynamic allocation of at most 64 KB (tests/test_machine.py reads the code object's notes); only vector
// stores; only what the tests' SIMT emulator provides is used, so the unmodified source runs there.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "jss_abi_checks.hpp"

namespace {

constexpr int kWave = 64;
constexpr int kDurMask = 0xffff;
constexpr int kNever = 0x7fffffff;

// what the kernels read of (desc, state, mr / bb): the members by value, so that the kernels' arguments stay few.  The build
// writes its makespans through `length` and its orders through `rank_out`.
struct MachineParams {
    const int32_t *env_const, *ops, *parents, *rank, *bias;
    const uint64_t *fixed;
    int32_t *length, *lower_bound, *bottleneck, *jps, *schrage, *head, *tail, *rank_out, *info, *order;
    int32_t n, stride, reopt, batch, jmax, mmax, n_tables;
    int32_t waves_per_block;
    int32_t wave_lds_ints;        // machine_lds_bytes / 4
    int32_t entries8;             // order_entries8
};

// one wavefront's LDS and the candidate's shape
struct Rows {
    int32_t *m_off, *m_cnt, *m_cur, *m_rel;      // one word per machine: segment start and length, cursor, release / tail
    int32_t *opw, *rk, *head, *tail, *tmp;       // by flat index; tmp by position: remaining times, saved ranks
    uint16_t *slot, *seq;                        // machine-major flat indices: by flat index, by (rank, flat index)
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
    w.opw = mine + 4 * kWave, w.rk = w.opw + p.entries8, w.head = w.rk + p.entries8, w.tail = w.head + p.entries8;
    w.tmp = w.tail + p.entries8;
    w.slot = reinterpret_cast<uint16_t *>(w.tmp + p.entries8), w.seq = w.slot + p.entries8;
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

__global__ __launch_bounds__(256) void jss_machine_relax_kernel(MachineParams p) {
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
    int my_jps = -1, my_schrage = -1, best = -1, neck = -1;
    const bool starts = p.schrage || p.rank_out;
    unsigned long long open = used & ~fixed;
#pragma unroll 1
    while (open) {
        const int m = __ffsll(open) - 1;
        open &= open - 1;
        const int v = jackson(w, m), s = starts ? schrage(w, m) : -1;
        if (lane == m) my_jps = v, my_schrage = s;
        if (v > best) best = v, neck = m;
    }
    if (lane == 0) {
        if (p.lower_bound) p.lower_bound[c] = imax(length, best);
        if (p.bottleneck) p.bottleneck[c] = neck;
    }
    if (lane < p.mmax) {
        if (p.jps) p.jps[c * p.mmax + lane] = my_jps;
        if (p.schrage) p.schrage[c * p.mmax + lane] = my_schrage;
    }
    if (p.head) write_row(w, p.head + (size_t)c * region, w.head, region);
    if (p.tail) write_row(w, p.tail + (size_t)c * region, w.tail, region);
    if (p.rank_out) write_row(w, p.rank_out + (size_t)c * region, w.rk, region);
}

__global__ __launch_bounds__(256) void jss_bottleneck_kernel(MachineParams p) {
    HIP_DYNAMIC_SHARED(int32_t, lds)

    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    const long long c = (long long)blockIdx.x * p.waves_per_block + wv;
    if (c >= p.n) return;                                             // (the whole wavefront, like every return below)
    unsigned long long fixed = p.fixed ? uniform64(p.fixed[c]) : 0ull;
    const int region = p.jmax * p.mmax, reopt = p.reopt;
    Rows w;
    unsigned long long used = 0;
    if (setup(p, lds, c, p.rank ? p.rank + (size_t)c * region : nullptr, fixed, w, &used) < 0) {
        if (lane == 0) p.length[c] = -1;
        return;
    }
    sort_machines(w, fixed & used);
    int length = forward(w, fixed);
    int first = length, n_fixed = 0, tried = 0, shorter = 0, my_order = -1;
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
            if (at_start) first = imax(first, v);
            const long long biased = (long long)v + (p.bias ? __builtin_amdgcn_readfirstlane(p.bias[c * p.mmax + m]) : 0);
            if (star < 0 || biased > high) star = m, high = biased;
        }
        at_start = false;
        // 2. - 4. its Schrage starts as ranks, its bit, the length
        const unsigned long long star_bit = 1ull << star;
        schrage(w, star);
        fixed |= star_bit;
        if (lane == n_fixed) my_order = star;
        n_fixed += 1;
        sort_machines(w, star_bit);
        int cur = length = forward(w, fixed);
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
                const int lo = __builtin_amdgcn_readfirstlane(w.m_off[k]), n = __builtin_amdgcn_readfirstlane(w.m_cnt[k]);
#pragma unroll 1
                for (int i = lane; i < n; i += kWave) w.tmp[lo + i] = w.rk[w.slot[lo + i]];
                schrage(w, k);
                sort_machines(w, k_bit);
                const int now = forward(w, fixed);
                if (now >= 0 && now <= cur) {
                    shorter += now < cur ? 1 : 0, cur = now;
                } else {
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
    if (p.info && lane < JSS_BOTTLENECK_NI) p.info[c * JSS_BOTTLENECK_NI + lane] = lane == 0 ? n_fixed : lane == 1 ? tried : lane == 2 ? shorter : first;
    if (p.order && lane < p.mmax) p.order[c * p.mmax + lane] = my_order;
}

// the launch both entry points share
template <typename Kernel>
int launch(Kernel kernel, const JssDesc *desc, MachineParams &p, void *stream) {
    const long long bytes = jss_abi::machine_lds_bytes(desc->jmax, desc->mmax);
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

int jss_machine_relax(const JssDesc *desc, const JssState *state, const JssMachineRelax *mr, void *stream) {
    if (const int rc = jss_abi::machine_relax_check(desc, state, mr)) return rc;
    if (mr->n == 0) return 0;
    MachineParams p = {};
    p.env_const = state->env_const, p.parents = mr->parents, p.rank = mr->rank, p.fixed = mr->fixed;
    p.length = mr->length, p.lower_bound = mr->lower_bound, p.bottleneck = mr->bottleneck, p.jps = mr->jps, p.schrage = mr->schrage;
    p.head = mr->head, p.tail = mr->tail, p.rank_out = mr->rank_out;
    p.n = mr->n, p.stride = mr->stride;
    return launch(jss_machine_relax_kernel, desc, p, stream);
}

int jss_bottleneck_build(const JssDesc *desc, const JssState *state, const JssBottleneck *bb, void *stream) {
    if (const int rc = jss_abi::bottleneck_check(desc, state, bb)) return rc;
    if (bb->n == 0) return 0;
    MachineParams p = {};
    p.env_const = state->env_const, p.parents = bb->parents, p.rank = bb->rank_in, p.fixed = bb->fixed_in, p.bias = bb->bias;
    p.length = bb->makespan, p.rank_out = bb->rank, p.info = bb->info, p.order = bb->order;
    p.n = bb->n, p.reopt = bb->reopt;
    return launch(jss_bottleneck_kernel, desc, p, stream);
}

}  // extern "C"
