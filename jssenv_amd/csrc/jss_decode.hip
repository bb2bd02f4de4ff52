// jssenv_amd/csrc/jss_decode.hip -- libjss_decode_hip.so: jss_decode_keys and jss_keys_evolve (include/jss_decode.h), key tables
// decoded into active schedules by Giffler and Thompson's procedure, one decode per candidate in one launch on the MI355X, and one
// generation of a biased random-key genetic algorithm.  A library of its own: libjss_hip.so, libjss_beam_hip.so,
// libjss_bound_hip.so, libjss_order_hip.so, libjss_tabu_hip.so, libjss_block_hip.so, libjss_relink_hip.so and their kernels are not
// touched by it (the device helpers it has in common with them are written out again here for that reason).  It shares
// jss_abi_checks.hpp (the argument checks and the LDS a candidate needs) with the host-core twin, which carries the same entry
// points.
//
// jss_decode_kernel: one wavefront per candidate; everything a branch or a loop around a cross-lane operation depends on is
// wave-uniform, so every way out of the kernel takes the whole wavefront.  Job j sits on lane j % 64, slot j / 64 (two slots
// beyond 64 jobs).  No workgroup barrier is used: the wavefronts of a workgroup only share its LDS allocation, each with a region
// of its own (decode_lds_bytes), and the host picks 4, 2 or 1 of them per workgroup by that size.  The semantics are the header's;
// the form:
//
//   once    the candidate's op row and key row into LDS, a lane per entry, and one word per machine, rel[], zeroed; where the
//           start times are asked for, the padding of the candidate's row gets its -1.  A lane keeps, per slot, its job's count,
//           end, current op word and current key in registers.
//   an iteration  est from rel[] (one LDS read per slot); the wave minimum of ect by DPP row steps and four lane reads, its
//           lowest job by a ballot (slot 0 holds the lower jobs); m* read from that lane; the wave minimum of est on m*; the
//           conflict lanes by the header's int64 comparison, whose right side is wave-uniform; the wave maximum of their keys and
//           the lowest job that holds it by a ballot -- the composite (key, -j) without an overflow, INT32_MIN included, because
//           the ballot only looks at conflict lanes.  The winning lane alone writes rel[m*] and its start (a plain store nobody
//           waits on) and reads its next op word and key from LDS.
//   out     the wave maximum of the jobs' ends; the counters are wave-uniform all along and leave through lanes 0 to 3.
//
// Idle lanes (j >= J, or a finished job) hold the neutral elements: INT32_MAX for the two minima, and no conflict bit.  Every
// loop is bounded (J * M iterations; the copies by the row's entries); every index into LDS is the flat index of an entry of the
// row or a machine number below 64.  No scratch memory, no spilled registers, LDS only as dynamic allocation of at most 64 KB
// (tests/test_decode.py reads the code object's notes); only vector stores; only what the tests' SIMT emulator provides is used,
// so the unmodified source runs there.
//
// jss_evolve_rank_kernel (one workgroup per group, the fitness in LDS, every individual's rank by counting) and
// jss_evolve_children_kernel (one thread per entry of keys_out) are small and not tuned: a generation is a few microseconds of a
// search whose time goes into the decodes.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "jss_abi_checks.hpp"

namespace {

constexpr int kWave = 64;
constexpr int kDurMask = 0xffff;
constexpr int kNever = 0x7fffffff;
constexpr int kLowest = -0x7fffffff - 1;
constexpr int kRankThreads = 256;
constexpr int kChildThreads = 256;

// what the kernel reads of (desc, state, dc): the members by value, so that the kernel's arguments stay few
struct DecodeParams {
    const int32_t *env_const, *ops, *parents, *keys, *delta_of;
    int32_t *makespan, *start, *info;
    int32_t n, stride, delta_q16, batch, jmax, mmax, n_tables;
    int32_t waves_per_block;
    int32_t wave_lds_ints;        // decode_lds_bytes / 4
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

// lanes below this one whose bit is set in `mask`
__device__ __forceinline__ int lanes_below(unsigned long long mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// the lowest job of two ballots, one per slot (slot 0 holds the jobs below 64); one of them is not empty
__device__ __forceinline__ int lowest_job(unsigned long long slot0, unsigned long long slot1) {
    return slot0 ? __ffsll(slot0) - 1 : kWave + __ffsll(slot1) - 1;
}

template <bool kTwoSlots>
__device__ __forceinline__ void decode(const DecodeParams &p, long long c, int J, int M, long long delta, const int32_t *opw,
                                       const int32_t *key_row, int32_t *rel, int32_t *start) {
    constexpr int kSlots = kTwoSlots ? 2 : 1;
    const int lane = lanes_below(~0ull), mmax = p.mmax, total = J * M;
    int done[kSlots], job_end[kSlots], op_now[kSlots], key_now[kSlots];
    bool live[kSlots];
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
        const int j = s * kWave + lane;
        live[s] = j < J;
        done[s] = 0, job_end[s] = 0;
        op_now[s] = live[s] ? opw[j * mmax] : 0;
        key_now[s] = live[s] ? key_row[j * mmax] : 0;
    }
    int conflicts = 0, widest = 0, delayed = 0;
#pragma unroll 1
    for (int it = 0; it < total; ++it) {
        // 1. est and ect of every unfinished job; 2. the lowest (ect, j)
        int est[kSlots], ect_low = kNever;
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            est[s] = imax(job_end[s], rel[(op_now[s] >> 16) & 63]);
            ect_low = imin(ect_low, live[s] ? est[s] + (op_now[s] & kDurMask) : kNever);
        }
        const int c_star = wave_min(ect_low);
        const unsigned long long first0 = __ballot(live[0] && est[0] + (op_now[0] & kDurMask) == c_star);
        const unsigned long long first1 = kTwoSlots && !first0 ? __ballot(live[kSlots - 1] && est[kSlots - 1] + (op_now[kSlots - 1] & kDurMask) == c_star) : 0ull;
        const int j_star = lowest_job(first0, first1);
        const int m_star = (__builtin_amdgcn_readlane(j_star < kWave ? op_now[0] : op_now[kSlots - 1], j_star & 63) >> 16) & 63;
        // 3. the earliest start on m*
        bool on[kSlots];
        int est_low = kNever;
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            on[s] = live[s] && ((op_now[s] >> 16) & 63) == m_star;
            est_low = imin(est_low, on[s] ? est[s] : kNever);
        }
        const int e0 = wave_min(est_low);
        // 4. the conflict set; 5. its largest key, the lowest job that holds it
        const long long bound = delta * (long long)(c_star - e0);         // (wave-uniform)
        bool conf[kSlots];
        int key_high = kLowest;
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            conf[s] = on[s] && (est[s] == e0 || (long long)(est[s] - e0) * 65536 < bound);
            key_high = imax(key_high, conf[s] ? key_now[s] : kLowest);
        }
        const int k_star = wave_max(key_high);
        const unsigned long long in0 = __ballot(conf[0]), in1 = kTwoSlots ? __ballot(conf[kSlots - 1]) : 0ull;
        const unsigned long long top0 = __ballot(conf[0] && key_now[0] == k_star);
        const unsigned long long top1 = kTwoSlots && !top0 ? __ballot(conf[kSlots - 1] && key_now[kSlots - 1] == k_star) : 0ull;
        const int pick = lowest_job(top0, top1);
        const int size = __popcll(in0) + __popcll(in1);
        const int s_pick = __builtin_amdgcn_readlane(pick < kWave ? est[0] : est[kSlots - 1], pick & 63);
        conflicts += size > 1 ? 1 : 0, widest = imax(widest, size), delayed += s_pick > e0 ? 1 : 0;
        // 6. the chosen job starts (every lane has read rel[]: the cross-lane operations lie between)
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            if (s * kWave + lane != pick) continue;
            const int x = pick * mmax + done[s];
            if (start) start[x] = est[s];
            job_end[s] = est[s] + (op_now[s] & kDurMask);
            rel[m_star] = job_end[s];
            done[s] += 1;
            live[s] = done[s] < M;
            if (live[s]) op_now[s] = opw[x + 1], key_now[s] = key_row[x + 1];
        }
        wave_lds_sync();
    }
    int end = job_end[0];
    if (kTwoSlots) end = imax(end, job_end[kSlots - 1]);
    const int makespan = wave_max(end);
    if (lane == 0) p.makespan[c] = makespan;
    if (p.info && lane < JSS_DECODE_NI) p.info[c * JSS_DECODE_NI + lane] = lane == 0 ? conflicts : lane == 1 ? widest : lane == 2 ? delayed : 0;
}

__global__ __launch_bounds__(256) void jss_decode_kernel(DecodeParams p) {
    HIP_DYNAMIC_SHARED(int32_t, lds)

    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    const long long c = (long long)blockIdx.x * p.waves_per_block + wv;
    if (c >= p.n) return;                                             // (the whole wavefront, like every return below)
    const int parent = __builtin_amdgcn_readfirstlane(p.parents ? p.parents[c] : (int)c);
    const int delta = __builtin_amdgcn_readfirstlane(p.delta_of ? p.delta_of[c] : p.delta_q16);
    if (parent < 0 || parent >= p.batch || delta < 0 || delta > 65536) {
        if (lane == 0) p.makespan[c] = -1;
        return;
    }
    const int jmax = p.jmax, mmax = p.mmax, region = jmax * mmax;
    const int32_t *ec = p.env_const + (size_t)parent * JSS_NC;
    const int J = __builtin_amdgcn_readfirstlane(ec[JSS_C_JOBS]), M = __builtin_amdgcn_readfirstlane(ec[JSS_C_MACHINES]);
    const int tab = __builtin_amdgcn_readfirstlane(ec[JSS_C_TABLE]);
    // (J == 0: never reset.  The rest holds for every env a reset has written; it keeps the decode inside the rows)
    if (!(J >= 1 && J <= jmax && M >= 1 && M <= mmax && tab >= 0 && tab < p.n_tables)) {
        if (lane == 0) p.makespan[c] = -1;
        return;
    }
    const int32_t *ops = p.ops + (size_t)tab * region, *keys = p.keys + (size_t)c * p.stride;
    int32_t *start = p.start ? p.start + (size_t)c * region : nullptr;

    // this wavefront's LDS: one word per machine, then the op row and the key row
    int32_t *rel = lds + (size_t)wv * p.wave_lds_ints;
    int32_t *opw = rel + kWave, *key_row = opw + p.entries8;
    rel[lane] = 0;
#pragma unroll 1
    for (int e = lane; e < region; e += kWave) {
        opw[e] = ops[e], key_row[e] = keys[e];
        if (start) {
            const int j = e / mmax, k = e - j * mmax;
            if (!(j < J && k < M)) start[e] = -1;                     // (the padding; every other entry gets its start below)
        }
    }
    wave_lds_sync();
    if (J > kWave)
        decode<true>(p, c, J, M, delta, opw, key_row, rel, start);
    else
        decode<false>(p, c, J, M, delta, opw, key_row, rel, start);
}

// ---- one BRKGA generation -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t fmix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}
// the counter RNG of jss_common.hpp (oracle/jss_oracle.c orc_rng_u32)
__device__ __forceinline__ uint32_t rng_u32(uint64_t seed, uint64_t env_id, uint32_t episode, uint32_t step) {
    const uint32_t a = (uint32_t)seed + (uint32_t)env_id * 0x9E3779B9u + episode * 0x85EBCA6Bu + step * 0xC2B2AE35u;
    const uint32_t b = (uint32_t)(seed >> 32) ^ ((uint32_t)(env_id >> 32) * 0x27D4EB2Fu);
    return fmix32(fmix32(a) ^ b);
}

// by_rank[g * P + r] = the individual with the r-th lowest (fitness < 0, fitness, p) of group g = blockIdx.x; without a
// fitness (an initial population) the individuals in their own order
__global__ __launch_bounds__(kRankThreads) void jss_evolve_rank_kernel(const int32_t *fitness, int32_t *by_rank, int pop) {
    __shared__ int32_t fit[JSS_EVOLVE_MAX_POP];
    const int tid = (int)threadIdx.x;
    const size_t base = (size_t)blockIdx.x * pop;
    if (!fitness) {
        for (int q = tid; q < pop; q += kRankThreads) by_rank[base + q] = q;
        return;
    }
    for (int q = tid; q < pop; q += kRankThreads) fit[q] = fitness[base + q];
    __syncthreads();
    for (int q = tid; q < pop; q += kRankThreads) {
        // (fitness < 0, fitness) as one unsigned word: a negative value keeps its top bit and sorts behind every other
        const unsigned mine = (unsigned)fit[q];
        int rank = 0;
        for (int o = 0; o < pop; ++o) {
            const unsigned other = (unsigned)fit[o];
            rank += other < mine || (other == mine && o < q) ? 1 : 0;
        }
        by_rank[base + rank] = q;
    }
}

struct ChildParams {
    const int32_t *keys_in, *by_rank;
    int32_t *keys_out;
    uint64_t seed;                // already keyed: seed ^ JSS_EVOLVE_SEED_XOR
    long long entries;            // groups * pop * region
    int32_t pop, region, n_elite, n_mutant, rho_q16, generation;
};

__global__ __launch_bounds__(kChildThreads) void jss_evolve_children_kernel(ChildParams p) {
    const long long x = (long long)blockIdx.x * kChildThreads + threadIdx.x;
    if (x >= p.entries) return;
    const long long i = x / p.region;
    const int e = (int)(x - i * p.region);
    const long long g = i / p.pop;
    const int c = (int)(i - g * p.pop);
    const long long first = g * p.pop;                                // the group's first row
    const uint32_t gen = (uint32_t)p.generation;
    if (c < p.n_elite) {
        p.keys_out[x] = p.keys_in[(first + p.by_rank[first + c]) * p.region + e];
        return;
    }
    const uint32_t r = rng_u32(p.seed, (uint64_t)i, gen, (uint32_t)e);
    if (c >= p.pop - p.n_mutant) {
        p.keys_out[x] = (int32_t)r;
        return;
    }
    const bool from_elite = (int)(r >> 16) < p.rho_q16;
    const int at = from_elite ? (int)(rng_u32(p.seed, (uint64_t)i, gen, (uint32_t)p.region) % (uint32_t)p.n_elite)
                              : p.n_elite + (int)(rng_u32(p.seed, (uint64_t)i, gen, (uint32_t)p.region + 1u) % (uint32_t)(p.pop - p.n_elite));
    p.keys_out[x] = p.keys_in[(first + p.by_rank[first + at]) * p.region + e];
}

// the children of one call; by_rank may be NULL for an initial population, which reads no ranking
int launch_children(const JssEvolve &ev, const int32_t *by_rank, hipStream_t s) {
    ChildParams p;
    p.keys_in = ev.keys_in, p.by_rank = by_rank, p.keys_out = ev.keys_out;
    p.seed = ev.seed ^ JSS_EVOLVE_SEED_XOR;
    p.entries = (long long)ev.groups * ev.pop * ev.region;
    p.pop = ev.pop, p.region = ev.region, p.n_elite = ev.n_elite, p.n_mutant = ev.n_mutant, p.rho_q16 = ev.rho_q16;
    p.generation = ev.generation;
    const long long blocks = (p.entries + kChildThreads - 1) / kChildThreads;
    hipLaunchKernelGGL(jss_evolve_children_kernel, dim3((unsigned)blocks), dim3(kChildThreads), 0, s, p);
    return (int)hipGetLastError();
}

// A ranking nobody asked for goes to device memory of the call's own.  hipFree waits for the device, so the kernels that read the
// ranking have ended when it goes; a caller that wants no such wait passes a by_rank.  (The SIMT emulator of the tests runs
// kernels on the host, synchronously.)
#if defined(__HIPCC__)
bool scratch_alloc(int32_t **ptr, size_t bytes) { return hipMalloc(reinterpret_cast<void **>(ptr), bytes) == hipSuccess; }
void scratch_free(int32_t *ptr) { (void)hipFree(ptr); }
#else
bool scratch_alloc(int32_t **ptr, size_t bytes) { return (*ptr = static_cast<int32_t *>(malloc(bytes))) != nullptr; }
void scratch_free(int32_t *ptr) { free(ptr); }
#endif

}  // namespace

extern "C" {

int jss_decode_keys(const JssDesc *desc, const JssState *state, const JssDecode *dc, void *stream) {
    if (const int rc = jss_abi::decode_check(desc, state, dc)) return rc;
    if (dc->n == 0) return 0;
    DecodeParams p;
    p.env_const = state->env_const, p.ops = desc->ops, p.parents = dc->parents, p.keys = dc->keys, p.delta_of = dc->delta_of;
    p.makespan = dc->makespan, p.start = dc->start, p.info = dc->info;
    p.n = dc->n, p.stride = dc->stride, p.delta_q16 = dc->delta_q16;
    p.batch = desc->batch, p.jmax = desc->jmax, p.mmax = desc->mmax, p.n_tables = desc->n_tables;
    const long long bytes = jss_abi::decode_lds_bytes(desc->jmax, desc->mmax);
    p.entries8 = (int32_t)jss_abi::order_entries8(desc->jmax, desc->mmax);
    p.wave_lds_ints = (int32_t)(bytes / 4);
    // wavefronts per workgroup: they only share the LDS allocation, and small allocations pack a CU's 160 KB better
    p.waves_per_block = 4 * bytes <= 32 * 1024 ? 4 : 2 * bytes <= 32 * 1024 ? 2 : 1;
    const size_t shmem = (size_t)bytes * p.waves_per_block;          // at most 64 KB (decode_check): no function attribute to raise
    const long long blocks = ((long long)dc->n + p.waves_per_block - 1) / p.waves_per_block;
    hipLaunchKernelGGL(jss_decode_kernel, dim3((unsigned)blocks), dim3((unsigned)(kWave * p.waves_per_block)), shmem,
                       reinterpret_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

int jss_keys_evolve(const JssEvolve *ev, void *stream) {
    if (const int rc = jss_abi::evolve_check(ev)) return rc;
    if (ev->groups == 0) return 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool fresh = ev->n_elite == 0 && ev->n_mutant == ev->pop;
    if (fresh && !ev->by_rank) return launch_children(*ev, nullptr, s);
    int32_t *scratch = nullptr;
    if (!ev->by_rank && !scratch_alloc(&scratch, (size_t)ev->groups * ev->pop * sizeof(int32_t))) return JSS_E_NULL;
    int32_t *by_rank = ev->by_rank ? ev->by_rank : scratch;
    hipLaunchKernelGGL(jss_evolve_rank_kernel, dim3((unsigned)ev->groups), dim3(kRankThreads), 0, s, fresh ? nullptr : ev->fitness,
                       by_rank, ev->pop);
    const int rc = launch_children(*ev, by_rank, s);
    if (scratch) scratch_free(scratch);
    return rc;
}

}  // extern "C"
