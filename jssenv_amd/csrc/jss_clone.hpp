// jssenv_amd/csrc/jss_clone.hpp -- jss_clone: env k of one batch becomes a byte-for-byte copy of env src_of_dst[k] of another
// (or the same) batch, every state and output row and the env's instance assignment.  Interface: include/jss_hip.h.
//
//   * one wavefront per destination env.  The source index is read once and made wave-uniform (readfirstlane), so a -1
//     ("leave k alone") or a bad index ends the whole wavefront at once.
//   * a segment is one env's row of one tensor, at env * row bytes in both batches.  The host decides per segment (from the
//     row length and the two base addresses) whether the rows move in dwordx4 -- both rows 16-byte aligned -- or in dwords /
//     bytes: the 900-byte solution row of ta01 starts 4-aligned in one env and 16-aligned in another, so it moves in dwords.
//   * lane i first loads element i of EVERY segment's row into registers and only then stores them (a register per
//     segment, indexed by unrolled constants: no private array in scratch), so one wavefront has all its rows in flight
//     at once instead of one round trip per segment; the elements from 64 on (the solution and observation rows of the
//     larger shapes) follow in a second loop.  No LDS.
//   * env_const's JSS_C_TABLE word is the env's table index.  With one table per env the clone moves env i's table into
//     table k, so the word is rewritten to k in the register before the store (what a reset of env k would write).
#pragma once
#include "jss_common.hpp"

namespace jss {

constexpr int kCloneBlock = 256;                 // four wavefronts, four destination envs
constexpr int kCloneMaxSegs = 13;               // 10 state / output rows, 3 table rows

// one tensor's per-env rows: destination and source base, bytes per row, element size (16, 4 or 1), elements per row
struct CloneSeg {
    char *dst;
    const char *src;
    int32_t bytes;
    int32_t unit;
    int32_t n;
    int32_t pad;
};

struct CloneParams {
    CloneSeg seg[kCloneMaxSegs];
    const int32_t *src_of_dst;
    int32_t *dst_env;                            // header (JSS_ERR_BAD_INDEX goes into its status word)
    int64_t batch_dst, batch_src;
    int32_t n_seg;
    int32_t own_tables;                          // one table per env: env_const's JSS_C_TABLE word names table k, not i
};

// element i of a row as a dwordx4 (unit 16), a dword (4) or a byte (1), in the low words of an int4
__device__ __forceinline__ int4 clone_load(const char *s, int unit, int i) {
    if (unit == 16) return reinterpret_cast<const int4 *>(s)[i];
    if (unit == 4) return make_int4(reinterpret_cast<const int32_t *>(s)[i], 0, 0, 0);
    return make_int4((int)reinterpret_cast<const uint8_t *>(s)[i], 0, 0, 0);
}

__device__ __forceinline__ void clone_store(char *d, int unit, int i, int4 v) {
    if (unit == 16) reinterpret_cast<int4 *>(d)[i] = v;
    else if (unit == 4) reinterpret_cast<int32_t *>(d)[i] = v.x;
    else reinterpret_cast<uint8_t *>(d)[i] = (uint8_t)v.x;
}

__global__ __launch_bounds__(kCloneBlock) void jss_clone_kernel(CloneParams p) {
    const int lane = (int)(threadIdx.x & 63);
    const long long k = (long long)blockIdx.x * (kCloneBlock / kWave) + (long long)(threadIdx.x >> 6);
    if (k >= p.batch_dst) return;                                    // (the whole wavefront)
    const int src = __builtin_amdgcn_readfirstlane(p.src_of_dst[k]);
    if (src == -1) return;
    if (src < -1 || src >= p.batch_src) {                            // documented: env k untouched but for this bit
        if (lane == 0) p.dst_env[k * JSS_NH + JSS_H_STATUS] |= JSS_ERR_BAD_INDEX;
        return;
    }
    int4 v[kCloneMaxSegs];
#pragma unroll
    for (int i = 0; i < kCloneMaxSegs; ++i) {                        // element `lane` of every row: all loads in flight
        if (i < p.n_seg && lane < p.seg[i].n)
            v[i] = clone_load(p.seg[i].src + (size_t)src * p.seg[i].bytes, p.seg[i].unit, lane);
        if (i == 1 && p.own_tables) {                                // segment 1 = env_const (12 words: one load per lane)
            if (p.seg[1].unit == 16 && lane == JSS_C_TABLE / 4) v[1].w = (int)k;
            if (p.seg[1].unit == 4 && lane == JSS_C_TABLE) v[1].x = (int)k;
        }
    }
#pragma unroll
    for (int i = 0; i < kCloneMaxSegs; ++i) {
        if (i < p.n_seg && lane < p.seg[i].n)
            clone_store(p.seg[i].dst + (size_t)k * p.seg[i].bytes, p.seg[i].unit, lane, v[i]);
    }
    for (int i = 0; i < p.n_seg; ++i) {                              // elements 64.. of the long rows
        const CloneSeg sg = p.seg[i];
        const int n = sg.n;
        const char *s = sg.src + (size_t)src * sg.bytes;
        char *d = sg.dst + (size_t)k * sg.bytes;
        for (int e = lane + kWave; e < n; e += kWave) clone_store(d, sg.unit, e, clone_load(s, sg.unit, e));
    }
}

}  // namespace jss
