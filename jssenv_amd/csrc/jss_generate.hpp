// jssenv_amd/csrc/jss_generate.hpp -- jss_generate: Taillard (1993) instances drawn on the device, one J x M instance per
// flagged env, written into the env's own op / work / instance tables.  Interface and the draw: include/jss_hip.h.
//
//   * one wavefront reads the flags of `per_wave` consecutive envs (which / actions: one byte / dword per lane, one access),
//     ballots them and generates only the flagged envs, one after the other: a step's sparse `which = done` (about 1 env
//     in 225) costs one flag read per 64 envs.  Full generation (no flags) gives a wavefront fewer envs, for parallelism.
//   * inside an env, job j sits on lane j % 64 (slot j / 64).  Job j's draws start at index j * M of both Lehmer streams, so a
//     lane jumps there with x0 * a^(jM) mod (2^31 - 1) -- a^(jM) is the same for every env of the call and computed once
//     per lane -- and walks only its own M draws: the swap loop of the machine stream, then the time stream twice (the
//     durations and the job length, then the suffix sums), so that no duration has to be kept.
//   * the swap loop indexes the job's machine row dynamically: the row lives in LDS, one byte per machine, k-major
//     ([k][thread]: the lanes of a wave hit consecutive bytes), 64 bytes per lane -- never in a private array (scratch).
//   * max duration, max job length and sum_op are butterfly reductions over the wave; lanes 0-11 write the record.
#pragma once
#include "jss_common.hpp"

namespace jss {

struct GenParams {
    int32_t *ops, *rem, *inst;                   // JssGen's writable tables
    const int64_t *time_seed, *machine_seed;     // explicit seeds, or NULL (derived)
    const int32_t *actions;                      // JssGen.actions (may be NULL)
    const uint8_t *which;                        // may be NULL
    const int32_t *env;                          // JssState.env (derived seeds: the episode)
    const int64_t *env_ids;
    int64_t env_id_base;
    uint64_t seed;
    int32_t batch, jmax, mmax, jobs, machines, dur_low, dur_high;
    int32_t per_wave;                            // envs whose flags one wavefront reads (<= 64)
};

constexpr int kGenBlock = 256;
constexpr int kGenFullPerWave = 8;               // envs per wavefront when every env is generated
constexpr uint32_t kLcgM = 2147483647u;          // 2^31 - 1, a Mersenne prime
constexpr uint32_t kLcgA = 16807u;
constexpr uint64_t kGenSeedXor = JSS_GEN_SEED_XOR;

// x * y mod (2^31 - 1), x, y < 2^31: 2^31 = 1 (mod m), so the 62-bit product folds at bit 31 (twice: the first fold can
// carry into bit 31) and one conditional subtraction finishes it
__device__ __forceinline__ uint32_t lcg_mulmod(uint32_t x, uint32_t y) {
    const uint64_t p = (uint64_t)x * y;
    uint64_t r = (p & kLcgM) + (p >> 31);
    r = (r & kLcgM) + (r >> 31);
    return (uint32_t)(r >= kLcgM ? r - kLcgM : r);
}

// a^e mod (2^31 - 1) by square-and-multiply
__device__ __forceinline__ uint32_t lcg_pow(uint32_t e) {
    uint32_t r = 1, b = kLcgA;
    for (; e; e >>= 1) {
        if (e & 1) r = lcg_mulmod(r, b);
        b = lcg_mulmod(b, b);
    }
    return r;
}

// one Taillard draw: advance the stream, low + trunc(fl(fl(x / m) * n)) in IEEE double (the correctly rounded division:
// no reciprocal, and no addition that could be contracted)
__device__ __forceinline__ int lcg_unif(uint32_t &x, int low, int n) {
    x = lcg_mulmod(x, kLcgA);
    return low + (int)((double)x / 2147483647.0 * (double)n);
}

// job j of env e on this lane: its rows of the op and work tables (zeros behind M, all zeros for a padding row j >= J);
// returns the job length, raises maxd to the job's longest op
__device__ __forceinline__ int gen_job(const GenParams &g, size_t e, int j, uint32_t ts, uint32_t ms, uint32_t jump,
                                       uint8_t *row, int &maxd) {
    const int M = g.machines, mm = g.mmax;
    int32_t *op_row = g.ops + ((size_t)e * g.jmax + j) * mm;
    int32_t *rem_row = g.rem + ((size_t)e * g.jmax + j) * mm;
    int len = 0, k0 = 0;
    if (j < g.jobs) {
        for (int k = 0; k < M; ++k) row[k * kGenBlock] = (uint8_t)k;
        uint32_t x = lcg_mulmod(ms, jump);
        for (int k = 0; k < M; ++k) {              // machine order: swap row[k] with row[unif(k, M - 1)]
            const int s = lcg_unif(x, k, M - k);
            const uint8_t a = row[k * kGenBlock], b = row[s * kGenBlock];
            row[k * kGenBlock] = b;
            row[s * kGenBlock] = a;
        }
        const int low = g.dur_low, n = g.dur_high - g.dur_low + 1;
        x = lcg_mulmod(ts, jump);
        for (int k = 0; k < M; ++k) {              // durations
            const int d = lcg_unif(x, low, n);
            op_row[k] = ((int)row[k * kGenBlock] << 16) | d;
            len += d;
            maxd = imax(maxd, d);
        }
        x = lcg_mulmod(ts, jump);
        int left = len;
        for (int k = 0; k < M; ++k) {              // the same draws again: rem[k] = durations of ops k..M-1
            rem_row[k] = left;
            left -= lcg_unif(x, low, n);
        }
        k0 = M;
    }
    for (int k = k0; k < mm; ++k) {
        op_row[k] = 0;
        rem_row[k] = 0;
    }
    return len;
}

__global__ __launch_bounds__(kGenBlock) void jss_generate_kernel(GenParams g) {
    __shared__ uint8_t rows[JSS_MAX_MACHINES * kGenBlock];     // [k][thread]: the machine row of the lane's current job
    const int lane = (int)(threadIdx.x & 63);
    const long long base = ((long long)blockIdx.x * (kGenBlock / kWave) + (long long)(threadIdx.x >> 6)) * g.per_wave;
    if (base >= g.batch) return;                               // (the whole wavefront)
    const int n = (int)(g.batch - base < g.per_wave ? g.batch - base : g.per_wave);
    int flag = 0;
    if (lane < n) {
        const size_t e = (size_t)(base + lane);
        flag = (!g.which && !g.actions) || (g.which && g.which[e]) || (g.actions && g.actions[e] == JSS_ACTION_RESET);
    }
    unsigned long long todo = __ballot(flag);
    if (!todo) return;
    const int slots = g.jmax > 64 ? 2 : 1;
    // where the lane's jobs start in both streams: a^(j M)
    const uint32_t jump0 = lcg_pow((uint32_t)(lane * g.machines));
    const uint32_t jump1 = slots > 1 ? lcg_pow((uint32_t)((lane + 64) * g.machines)) : 0u;
    uint8_t *row = rows + threadIdx.x;
    while (todo) {
        const size_t e = (size_t)(base + (__ffsll(todo) - 1));
        todo &= todo - 1;
        uint32_t ts, ms;
        if (g.time_seed) {
            const int64_t a = g.time_seed[e], b = g.machine_seed[e];
            if (a < 1 || a >= (int64_t)kLcgM || b < 1 || b >= (int64_t)kLcgM) continue;   // documented: tables untouched
            ts = (uint32_t)a;
            ms = (uint32_t)b;
        } else {
            const uint64_t id = g.env_ids ? (uint64_t)g.env_ids[e] : (uint64_t)(g.env_id_base + (int64_t)e);
            const uint32_t episode = (uint32_t)g.env[e * JSS_NH + JSS_H_EPISODE] + 1u;
            ts = 1u + rng_u32(g.seed ^ kGenSeedXor, id, episode, 0) % (kLcgM - 1u);
            ms = 1u + rng_u32(g.seed ^ kGenSeedXor, id, episode, 1) % (kLcgM - 1u);
        }
        int maxd = 0, maxlen = 0, sum = 0;
        for (int s = 0; s < slots; ++s) {
            const int j = lane + 64 * s;
            if (j >= g.jmax) continue;
            const int len = gen_job(g, e, j, ts, ms, s ? jump1 : jump0, row, maxd);
            maxlen = imax(maxlen, len);
            sum += len;
        }
        for (int o = 32; o; o >>= 1) {             // (every lane: wave-uniform control flow)
            maxd = imax(maxd, __shfl_xor(maxd, o));
            maxlen = imax(maxlen, __shfl_xor(maxlen, o));
            sum += __shfl_xor(sum, o);
        }
        if (lane < JSS_NI) {
            // JSS_I_*: J, M, max_time_op, max_time_jobs, sum_op, the correctly rounded float32 reciprocals, zeros
            const int v = lane == JSS_I_JOBS ? g.jobs : lane == JSS_I_MACHINES ? g.machines : lane == JSS_I_MAX_TIME_OP ? maxd
                        : lane == JSS_I_MAX_TIME_JOBS ? maxlen : lane == JSS_I_SUM_OP ? sum : 0;
            const int of = lane == JSS_I_RCP_MAX_TIME_OP ? maxd : lane == JSS_I_RCP_MAX_TIME_JOBS ? maxlen
                         : lane == JSS_I_RCP_SUM_OP ? sum : lane == JSS_I_RCP_MACHINES ? g.machines : 0;
            g.inst[e * JSS_NI + lane] = of ? as_int(1.0f / (float)of) : v;
        }
    }
}

}  // namespace jss
