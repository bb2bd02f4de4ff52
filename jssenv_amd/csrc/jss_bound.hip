// jssenv_amd/csrc/jss_bound.hip -- libjss_bound_hip.so: jss_bound (include/jss_bound.h), makespan lower bounds of states and of
// candidate moves on the MI355X.  A library of its own: libjss_hip.so, libjss_beam_hip.so and their kernels are not touched by
// it.  It shares jss_abi_checks.hpp (the argument check) with the host-core twin, which carries the same entry point.
//
// One wavefront per candidate, four per 256-thread workgroup, in the caller's order.  The parent and the action are read once
// and made wave-uniform, so every way out of the kernel takes the whole wavefront.  Job j sits on lane j % 64, slot j / 64 (two
// slots beyond 64 jobs, one after the other); addresses are wave-uniform 64-bit bases plus 32-bit lane offsets.  The semantics
// are the header's; the form:
//
//   A. every lane walks its job's row of the solution and of the op table: s_j, jobend_j, and the scheduled ops' ends into
//      r[m], the machines' release times, a 64-word block of LDS per wavefront.  The walk stops behind the first chunk whose
//      last op no job has scheduled.
//   -  the candidate's job takes its next op at its head: r of that op's machine and the job's own end move, nothing is stored.
//   B. every lane walks its row again from the first chunk that holds an unscheduled op of any job: the heads are a dependent
//      chain of max / add per lane, and every unscheduled op goes into its machine's min h, sum d and min tail in LDS.
//   C. lane m puts machine m's three words together; two wave-wide maxima give job_bound and lower_bound.
//
// A row is walked in chunks of kChunk ops: a chunk's loads -- two per op, indices clamped rather than branched around -- and its
// LDS gathers are all issued before the chain over the chunk starts, so the chain never waits for memory one dword at a time.
// Maxima and minima into LDS are write-until-stable loops under a ballot (each lane reads its cells, writes where its value
// beats what it read, until no lane of the wavefront wrote): a cell ends at the extreme whichever lane wins a round -- a lane
// whose value was overwritten by a lesser one writes again, the lesser one does not -- and it needs no atomic min / max, which
// the tests' SIMT emulator does not have; the sums are atomicAdd on int.  est_start, when asked for, is the solution row
// copied in a coalesced pass (padding -1) plus the heads stored along walk B.
//
// No scratch memory, no spilled registers, 4 KB of LDS (tests/test_bound.py reads the code object's notes); only vector stores;
// only what the SIMT emulator provides is used, so the unmodified source runs there.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "jss_abi_checks.hpp"

namespace {

constexpr int kBoundThreads = 256;
constexpr int kWave = 64;
constexpr int kBoundWaves = kBoundThreads / kWave;
constexpr int kChunk = 8;                        // ops of a row in flight per lane
constexpr int kNone = 0x7fffffff;                // a minimum nothing has entered yet
constexpr int kDurMask = 0xffff;

struct BoundParams {
    JssDesc d;
    JssState s;
    JssBound b;
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

// cell[m[i]] = max(cell[m[i]], v[i]) for every lane's kChunk pairs (a pair that takes no part: v = -1, below every cell)
__device__ __forceinline__ void lds_raise(int *cell, const int (&m)[kChunk], const int (&v)[kChunk]) {
    for (;;) {
        bool wrote = false;
        int seen[kChunk];
#pragma unroll
        for (int i = 0; i < kChunk; ++i) seen[i] = cell[m[i]];           // (all reads in flight, one wait)
#pragma unroll
        for (int i = 0; i < kChunk; ++i)
            if (seen[i] < v[i]) cell[m[i]] = v[i], wrote = true;
        wave_lds_sync();
        if (!__ballot(wrote)) break;
    }
}

// lo_a[m[i]] = min(lo_a[m[i]], a[i]) and the same for lo_b / b (a pair that takes no part: kNone)
__device__ __forceinline__ void lds_lower2(int *lo_a, int *lo_b, const int (&m)[kChunk], const int (&a)[kChunk], const int (&b)[kChunk]) {
    for (;;) {
        bool wrote = false;
        int seen_a[kChunk], seen_b[kChunk];
#pragma unroll
        for (int i = 0; i < kChunk; ++i) seen_a[i] = lo_a[m[i]], seen_b[i] = lo_b[m[i]];
#pragma unroll
        for (int i = 0; i < kChunk; ++i) {
            if (seen_a[i] > a[i]) lo_a[m[i]] = a[i], wrote = true;
            if (seen_b[i] > b[i]) lo_b[m[i]] = b[i], wrote = true;
        }
        wave_lds_sync();
        if (!__ballot(wrote)) break;
    }
}

__global__ __launch_bounds__(kBoundThreads) void jss_bound_kernel(BoundParams p) {
    __shared__ int lds_release[kBoundWaves][kWave];   // r_m
    __shared__ int lds_min_head[kBoundWaves][kWave];  // min_{U_m} h
    __shared__ int lds_sum_dur[kBoundWaves][kWave];   // sum_{U_m} d
    __shared__ int lds_min_tail[kBoundWaves][kWave];  // min_{U_m} (rem - d)

    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    const long long c = (long long)blockIdx.x * kBoundWaves + wv;
    if (c >= p.b.n) return;                                           // (the whole wavefront, like every return below)
    const int parent = __builtin_amdgcn_readfirstlane(p.b.parent ? p.b.parent[c] : (int)c);
    const int action = __builtin_amdgcn_readfirstlane(p.b.action ? p.b.action[c] : JSS_ACTION_SKIP);
    const int jmax = p.d.jmax, mmax = p.d.mmax, region = jmax * mmax;

    bool ok = parent >= 0 && parent < p.d.batch;
    int J = 0, M = 0, tab = 0, now = 0;
    if (ok) {
        const int32_t *ec = p.s.env_const + (size_t)parent * JSS_NC;
        J = ec[JSS_C_JOBS], M = ec[JSS_C_MACHINES], tab = ec[JSS_C_TABLE];
        now = p.s.env[(size_t)parent * JSS_NH + JSS_H_CLOCK];
        // (J == 0: never reset.  The rest holds for every env a reset has written; it keeps the walks inside the rows)
        ok = J >= 1 && J <= jmax && M >= 1 && M <= mmax && tab >= 0 && tab < p.d.n_tables && action >= JSS_ACTION_SKIP && action <= J;
        if (ok && p.b.mask && action >= 0) ok = p.b.mask[(size_t)parent * (jmax + 1) + action] != 0;
    }
    const bool moves = ok && action >= 0 && action < J;               // a job takes its next op
    const int owner = action & 63, owner_slot = action >> 6;

    const int32_t *sol = p.s.solution + (size_t)(ok ? parent : 0) * region;
    const int32_t *ops = p.d.ops + (size_t)tab * region;
    const int32_t *rem = p.d.rem + (size_t)tab * region;
    int *release = lds_release[wv], *min_head = lds_min_head[wv], *sum_dur = lds_sum_dur[wv], *min_tail = lds_min_tail[wv];

    int n_sched[2] = {0, 0}, job_end[2] = {0, 0};                     // s_j and jobend_j of the lane's (up to) two jobs
    if (ok) {
        release[lane] = 0, min_head[lane] = kNone, sum_dur[lane] = 0, min_tail[lane] = kNone;
        wave_lds_sync();
        // ---- A. the scheduled prefixes: s_j, jobend_j, r_m -------------------------------------------------------------
#pragma unroll
        for (int slot = 0; slot < 2; ++slot) {
            if (slot * kWave >= J) break;
            const int j = slot * kWave + lane, row = j * mmax;
            const bool live = j < J;
            for (int k0 = 0; k0 < M; k0 += kChunk) {
                int start[kChunk], op[kChunk];
#pragma unroll
                for (int i = 0; i < kChunk; ++i) {
                    const bool in = live && k0 + i < M;
                    const int at = in ? row + k0 + i : 0;
                    const int sv = sol[at], ov = ops[at];
                    start[i] = in ? sv : -1, op[i] = ov;
                }
                int mach[kChunk], end[kChunk];
#pragma unroll
                for (int i = 0; i < kChunk; ++i) {
                    const bool sched = start[i] >= 0;
                    mach[i] = sched ? (op[i] >> 16) & 63 : 0;
                    end[i] = sched ? start[i] + (op[i] & kDurMask) : -1;
                    if (sched) n_sched[slot] = k0 + i + 1, job_end[slot] = end[i];
                }
                lds_raise(release, mach, end);
                if (!__ballot(start[kChunk - 1] >= 0)) break;         // (prefixes: no job has a scheduled op behind this chunk)
            }
        }
    }
    // ---- the candidate's move: its job's next op starts at its head -----------------------------------------------------
    int moved_at = -1, moved_head = 0;                                // owner lane: the op's index and start
    if (moves) {
        const int s_mine = owner_slot ? n_sched[1] : n_sched[0];
        const int s_a = __shfl(s_mine, owner);
        if (s_a >= M) ok = false;                                     // no operation left
        else {
            if (lane == owner) {
                const int op = ops[action * mmax + s_a], m = (op >> 16) & 63;
                const int e_mine = owner_slot ? job_end[1] : job_end[0];
                moved_at = s_a, moved_head = imax(imax(now, e_mine), release[m]);
                const int end = moved_head + (op & kDurMask);
                release[m] = imax(release[m], end);
                if (owner_slot) n_sched[1] = s_a + 1, job_end[1] = end;
                else n_sched[0] = s_a + 1, job_end[0] = end;
            }
            wave_lds_sync();
        }
    }
    if (!ok) {
        if (lane == 0) {
            p.b.lower_bound[c] = -1;
            if (p.b.job_bound) p.b.job_bound[c] = -1;
        }
        return;
    }

    int32_t *est = p.b.est_start ? p.b.est_start + (size_t)c * region : nullptr;
    if (est) {                                                        // scheduled starts and the padding, coalesced
        for (int e = lane; e < region; e += kWave) {
            const int j = e / mmax, k = e - j * mmax;
            const int sv = sol[e];
            if (j >= J || k >= M) est[e] = -1;
            else if (sv >= 0) est[e] = sv;
        }
        if (moved_at >= 0) est[action * mmax + moved_at] = moved_head;
    }

    // ---- B. the heads of the unscheduled ops; per machine min h, sum d, min tail ----------------------------------------
    int job_bound = 0;
#pragma unroll
    for (int slot = 0; slot < 2; ++slot) {
        if (slot * kWave >= J) break;
        const int j = slot * kWave + lane, row = j * mmax;
        const bool live = j < J;
        const int s_j = n_sched[slot];
        int ready = imax(now, job_end[slot]);                         // h(j,k-1) + d(j,k-1); before the first head: max(t, jobend_j)
        const int first = wave_min(live ? s_j : M);
        for (int k0 = first - first % kChunk; k0 < M; k0 += kChunk) {
            int op[kChunk], tail[kChunk], mach[kChunk], rel[kChunk];
#pragma unroll
            for (int i = 0; i < kChunk; ++i) {
                const bool in = live && k0 + i < M;
                const int at = in ? row + k0 + i : 0;
                op[i] = ops[at], tail[i] = rem[at];
            }
#pragma unroll
            for (int i = 0; i < kChunk; ++i) {
                mach[i] = (op[i] >> 16) & 63;
                rel[i] = release[mach[i]];
            }
            int head[kChunk];
#pragma unroll
            for (int i = 0; i < kChunk; ++i) {
                const int k = k0 + i, dur = op[i] & kDurMask;
                const bool open = live && k < M && k >= s_j;
                if (open) {
                    head[i] = imax(ready, rel[i]);
                    ready = head[i] + dur;
                    tail[i] -= dur;
                    atomicAdd(&sum_dur[mach[i]], dur);
                    if (est) est[row + k] = head[i];
                } else {
                    head[i] = kNone, tail[i] = kNone, mach[i] = 0;
                }
            }
            lds_lower2(min_head, min_tail, mach, head, tail);
        }
        if (live) job_bound = imax(job_bound, s_j >= M ? job_end[slot] : ready);
    }
    // ---- C. the bounds -------------------------------------------------------------------------------------------------------
    wave_lds_sync();
    const int machine_bound = min_head[lane] != kNone ? min_head[lane] + sum_dur[lane] + min_tail[lane] : -1;
    job_bound = wave_max(job_bound);
    const int lower = imax(job_bound, wave_max(machine_bound));
    if (lane == 0) {
        p.b.lower_bound[c] = lower;
        if (p.b.job_bound) p.b.job_bound[c] = job_bound;
    }
}

}  // namespace

extern "C" {

int jss_bound(const JssDesc *desc, const JssState *state, const JssBound *b, void *stream) {
    if (const int rc = jss_abi::check_bound(desc, state, b)) return rc;
    if (b->n == 0) return 0;
    BoundParams p;
    p.d = *desc, p.s = *state, p.b = *b;
    hipLaunchKernelGGL(jss_bound_kernel, dim3((unsigned)((b->n + kBoundWaves - 1) / kBoundWaves)), dim3(kBoundThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

}  // extern "C"
