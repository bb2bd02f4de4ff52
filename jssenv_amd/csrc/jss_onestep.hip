// jssenv_amd/csrc/jss_onestep.hip -- libjss_onestep_hip.so: the one-step rollout (policy + step fused, one launch per env
// step) of the flagship class, for the MI355X (gfx950 / CDNA4).  Interface, class and error codes: include/jss_onestep.h.
//
// The class is what the headline runs: the packed flavour (G = 16 or 32 lanes per env) on ONE shared instance whose op table is
// staged in LDS, compact 16-byte job records, mode kRollout1.  In libjss_hip.so that is jss_packed_kernel<G, kRollout1,
// kTabLdsC>, whose name and register count the resource tables of the test suite pin; the kernel here is the same body
// (packed_block, jss_packed_env.hpp) with ONE difference: every store of the call -- the state records and headers, the
// solution entries, reward / done / makespan, the mask and the observation -- is a write-through store (st_out<true>,
// wt_store16) instead of a plain or streaming one.  Plain and streaming stores stay dirty in the XCD's L2 until the launch
// ends, and the boundary to the dependent launch -- the next step of the same envs -- pays for writing them back: a half-batch
// launch of the headline leaves some 23 MB.  Written through, the lines leave while the kernel still computes.
//
// Measured on the headline (ta01 x 65 536 envs, random policy, us per step, median of 7 interleaved windows of 1000 steps;
// profiles/r26_onestep/ab.txt), against the control built from this file with plain stores, which times like libjss_hip.so's:
//                                       one launch per step    two half-batch launches    three parts
//   libjss_hip.so                            18.01                  13.62                    13.53
//   plain stores (control)                   17.94                  13.66                    13.45
//   write-through stores (this file)         17.25                  13.03                    12.84
//   two env sets per wavefront               19.98                  15.45                    15.14
//   ... with write-through stores            19.75                  15.14                    14.61
// The other idea tried here lost and is not in this file: a wavefront serving two env sets in turn (half the wavefronts, the
// table staged once for both, the second set's raw state requested before the first is stepped; 64 VGPRs, no scratch) is
// 11 % slower in every form -- a wavefront's two steps take longer than two wavefronts' one, as with the two-envs-per-wave form
// of the one-wavefront-per-env kernels below three resident rounds (jss_kernels.hip, JSS_TWO_PER_WAVE_MIN_BATCH).
#include <mutex>
#include <unordered_map>

#include "jss_common.hpp"
#include "jss_packed_env.hpp"
#include "jss_abi_checks.hpp"
#include "jss_env_rows.hpp"
#include "jss_onestep.h"

namespace jss {

// 8 wavefronts per SIMD (64 VGPRs), arguments by value: as the kernel it stands in for
template <int G>
__global__ __launch_bounds__(kBlock, 8) void jss_onestep_kernel(Params p_arg) {
    HIP_DYNAMIC_SHARED(int32_t, lds)
    JSS_PARAMS_OF(p, p_arg, false);
    packed_block<G, kRollout1, kTabLdsC, false, true>(p, (int)blockIdx.x, lds);
}

}  // namespace jss

namespace {
using namespace jss;
using namespace jss_abi;

// ---- the launcher: what jss_kernels.hip does for jss_rollout_steps, for the one class (the two libraries share no object
// code; the argument checks, the env rows and the device functions are the shared headers) ---------------------------------
constexpr size_t kMaxDynamicLds = 64 * 1024;

// events of JSS_ROLLOUT_FORK_JOIN: one set per main stream, created on first use, kept for the life of the process
struct ForkJoinEvents {
    hipEvent_t fork = nullptr;
    hipEvent_t join[16] = {};
};
std::mutex g_events_mutex;
std::unordered_map<void *, ForkJoinEvents> g_events;

int events_for(void *main_stream, ForkJoinEvents **out) {
    std::lock_guard<std::mutex> lock(g_events_mutex);
    ForkJoinEvents &ev = g_events[main_stream];
    if (!ev.fork) {
        if (hipEventCreateWithFlags(&ev.fork, hipEventDisableTiming) != hipSuccess) return (int)hipGetLastError();
        for (int i = 0; i < 16; ++i)
            if (hipEventCreateWithFlags(&ev.join[i], hipEventDisableTiming) != hipSuccess) return (int)hipGetLastError();
    }
    *out = &ev;
    return 0;
}

int fork_streams(const ForkJoinEvents &ev, void *const *streams, int n) {
    if (hipEventRecord(ev.fork, reinterpret_cast<hipStream_t>(streams[0])) != hipSuccess) return (int)hipGetLastError();
    for (int i = 1; i < n; ++i)
        if (hipStreamWaitEvent(reinterpret_cast<hipStream_t>(streams[i]), ev.fork, 0) != hipSuccess) return (int)hipGetLastError();
    return 0;
}
// (every stream is joined even if one of the calls fails: no side stream is left running free of the caller's stream)
int join_streams(const ForkJoinEvents &ev, void *const *streams, int n) {
    int rc = 0;
    for (int i = 1; i < n; ++i) {
        if (hipEventRecord(ev.join[i], reinterpret_cast<hipStream_t>(streams[i])) != hipSuccess ||
            hipStreamWaitEvent(reinterpret_cast<hipStream_t>(streams[0]), ev.join[i], 0) != hipSuccess) {
            const int e = (int)hipGetLastError();
            if (!rc) rc = e;
        }
    }
    return rc;
}

// what of the class the shared checks do not see (include/jss_onestep.h)
int check_class(const JssDesc *d) {
    if (d->n_tables != 1 || d->table_of_env) return JSS_E_SHAPE;
    if (d->record_ints != JSS_NFC) return JSS_E_SHAPE;
    if (d->jmax > 32 || d->mmax > 32) return JSS_E_SHAPE;
    if (d->kernel & JSS_KERNEL_WAVE) return JSS_E_KIND;
    return 0;
}

struct Plan {
    void (*fn)(Params);
    int envs_per_block;
    size_t shmem;
};

// the LDS layout of a packed shared-table launch (jss_kernels.hip lds_layout / plan): the table, one observation image and
// one move table per wavefront
int plan(Params &p, Plan &lp) {
    const int G = p.d.jmax <= 16 && p.d.mmax <= 16 ? 16 : 32;
    p.region_ints = p.d.jmax * p.d.mmax;
    p.table_lds_ints = (p.region_ints + 3) & ~3;
    p.obs_wave_floats = ((kWave / G) * p.d.jmax * 7 + 3) & ~3;
    p.mv_off_ints = p.table_lds_ints + kWavesPerBlock * p.obs_wave_floats;
    p.norm_off_ints = p.mv_off_ints + kBlock;
    lp.shmem = sizeof(int32_t) * (size_t)p.norm_off_ints;
    if (lp.shmem > kMaxDynamicLds) return JSS_E_LDS;
    lp.envs_per_block = (kWave / G) * kWavesPerBlock;
    lp.fn = G == 16 ? jss_onestep_kernel<16> : jss_onestep_kernel<32>;
    return 0;
}

int fire(const Params &p, const Plan &lp, void *stream) {
    if (p.d.batch == 0) return 0;
    const int blocks = (p.d.batch + lp.envs_per_block - 1) / lp.envs_per_block;
    hipLaunchKernelGGL(lp.fn, dim3(blocks), dim3(kBlock), lp.shmem, reinterpret_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

Params params_of(const JssDesc *desc, const JssState *state, const JssOut *out, int kind, uint64_t seed, uint32_t explore_q16,
                 int32_t flags) {
    Params p = {};
    p.d = *desc;
    p.s = *state;
    p.o = *out;
    p.kind = kind; p.seed = seed; p.explore_q16 = explore_q16;
    p.n_iter = 1; p.flags = flags & ~JSS_ROLLOUT_FORK_JOIN;
    return p;
}

// envs [start, start + count) of the batch `p` describes (jss_kernels.hip sub_batch): every per-env pointer moves, the one
// instance table stays
Params sub_batch(const Params &p, int start, int count) {
    Params q = p;
    const size_t s0 = (size_t)start;
    q.d.batch = count;
    if (p.d.env_ids) q.d.env_ids = p.d.env_ids + s0;
    q.d.env_id_base = p.d.env_id_base + start;
    for_each_env_row(p.d, q.s, q.o, [s0](auto *&rows, size_t bytes, bool) {
        if (rows) rows = reinterpret_cast<decltype(+rows)>(reinterpret_cast<char *>(rows) + s0 * bytes);
    });
    return q;
}

// at most n_sub contiguous parts, boundaries at multiples of 64 envs (jss_kernels.hip cut: the same parts)
struct Part {
    int start, count;
};
int cut(int batch, int n_sub, Part *parts) {
    const int chunk = (((batch + n_sub - 1) / n_sub) + 63) & ~63;
    int n = 0;
    for (int start = 0; n < n_sub && start < batch; start += chunk) parts[n++] = Part{start, batch - start < chunk ? batch - start : chunk};
    return n;
}

}  // namespace

extern "C" {

int jss_onestep_version(void) { return JSS_ONESTEP_VERSION; }

int jss_onestep_rollout(const JssDesc *desc, const JssState *state, const JssOut *out, int kind, uint64_t seed,
                        uint32_t explore_q16, int32_t n_iter, int32_t flags, void *stream) {
    int rc = check_rollout(desc, state, out, stock_selector(kind), n_iter);
    if (rc || (rc = check_class(desc))) return rc;
    if (n_iter != 1) return JSS_E_SHAPE;
    Params p = params_of(desc, state, out, kind, seed, explore_q16, flags);
    Plan lp;
    if ((rc = plan(p, lp))) return rc;
    return fire(p, lp, stream);
}

int jss_onestep_rollout_steps(const JssDesc *desc, const JssState *state, const JssOut *out, int kind, uint64_t seed,
                              uint32_t explore_q16, int32_t n_steps, int32_t flags, int32_t n_sub, void *const *streams) {
    int rc = check_rollout_steps(desc, state, out, kind, n_steps, n_sub, streams);
    if (rc || (rc = check_class(desc))) return rc;
    if (n_steps == 0) return 0;                       // (no step: nothing is launched, nothing is touched)
    Params p = params_of(desc, state, out, kind, seed, explore_q16, flags);
    Plan lp;
    if ((rc = plan(p, lp))) return rc;
    Part parts[16];
    Params sub[16];
    const int n = cut(desc->batch, n_sub, parts);
    for (int i = 0; i < n; ++i) sub[i] = sub_batch(p, parts[i].start, parts[i].count);
    // step s of a part depends only on its own step s - 1: part i on streams[i], step-major
    const bool fork_join = (flags & JSS_ROLLOUT_FORK_JOIN) != 0 && n > 1;
    ForkJoinEvents *ev = nullptr;
    if (fork_join && ((rc = events_for(streams[0], &ev)) || (rc = fork_streams(*ev, streams, n)))) return rc;
    for (int s = 0; s < n_steps && !rc; ++s)
        for (int i = 0; i < n && !rc; ++i) rc = fire(sub[i], lp, streams[i]);
    const int jrc = fork_join ? join_streams(*ev, streams, n) : 0;
    return rc ? rc : jrc;                             // (the launch error wins over the join error)
}

}  // extern "C"
