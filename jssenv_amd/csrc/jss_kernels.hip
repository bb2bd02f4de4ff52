// jssenv_amd/csrc/jss_kernels.hip -- MI355X (gfx950 / CDNA4) kernels + C ABI of the
// batched Job-Shop-Scheduling simulator.  Interface and layout: include/jss_hip.h.
//
//   jss_common.hpp      parameters, wave helpers, counter RNG
//   jss_wave_env.hpp    one wavefront per env        (any J <= 128, M <= 64)
//   jss_packed_env.hpp  64/G envs per wavefront      (J, M <= G, G = 16 or 32)
//   jss_generate.hpp    Taillard instances drawn into the envs' own tables (jss_generate)
//   jss_clone.hpp       env k <- a copy of env src_of_dst[k], state, outputs and instance assignment (jss_clone)
//   (jss_lookahead, include/jss_search.h: the kLookahead mode of the two env flavours above)
//   jss_abi_checks.hpp  the C ABI's argument checks, shared with the host-core twin (jss_cpu.cpp)
//   jss_env_rows.hpp    the per-env tensors of a batch and their row sizes, shared with the twin (sub_batch, jss_clone)
//
// No MFMA anywhere: the path is integer indexing, there is no dense contraction.
#include <mutex>
#include <unordered_map>

#include "jss_common.hpp"
#include "jss_packed_env.hpp"
#include "jss_wave_env.hpp"
#include "jss_generate.hpp"
#include "jss_clone.hpp"
#include "jss_abi_checks.hpp"
#include "jss_env_rows.hpp"

namespace {
using namespace jss;
using namespace jss_abi;

// ---------------------------------------------------------------------------------------
// host side of the C ABI
// ---------------------------------------------------------------------------------------
// Events of JSS_ROLLOUT_FORK_JOIN: one set per main stream (streams[0]), created on first use on the device that is
// current then -- the device the caller launches on -- and kept for the life of the process.  Two env objects on two
// devices, or two host threads driving two streams, never share an event; the registry itself is guarded by a mutex.
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
    *out = &ev;                        // (unordered_map never moves its elements)
    return 0;
}

// streams[1..n) start behind everything queued on streams[0] so far ...
int fork_streams(const ForkJoinEvents &ev, void *const *streams, int n) {
    if (hipEventRecord(ev.fork, reinterpret_cast<hipStream_t>(streams[0])) != hipSuccess) return (int)hipGetLastError();
    for (int i = 1; i < n; ++i)
        if (hipStreamWaitEvent(reinterpret_cast<hipStream_t>(streams[i]), ev.fork, 0) != hipSuccess) return (int)hipGetLastError();
    return 0;
}
// ... and streams[0] continues behind all of them (every stream is joined even if one of the calls fails: a launch
// error in the middle of a window must not leave side streams running free of the caller's stream)
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

#ifdef JSS_PROFILING
int g_ablate = 0;
int g_lds_pad = 0;
unsigned long long *g_stamps = nullptr;
#endif

// Kernel flavour for a batch shape: the packed kernel needs every env's jobs AND machines to fit
// a 16- or 32-lane group.
// by_class: the fused multi-set grid, which honours JssDesc.jclass / mclass (a shape class inside wider padded tensors)
int class_jobs(const JssDesc &d, bool by_class) { return by_class && d.jclass > 0 ? d.jclass : d.jmax; }
int class_machines(const JssDesc &d, bool by_class) { return by_class && d.mclass > 0 ? d.mclass : d.mmax; }
int packed_group(const JssDesc &d, bool by_class = false) {
    if (d.kernel & JSS_KERNEL_WAVE) return 0;
    const int j = class_jobs(d, by_class), m = class_machines(d, by_class);
    if (j <= 16 && m <= 16) return 16;
    if (j <= 32 && m <= 32) return 32;
    return 0;
}

using KernelFn = void (*)(Params);

// Jobs per lane of the one-wavefront-per-env flavour for a plain (single-set) launch: by the padded extent -- unless the call
// names a shape class inside wider rows (JssDesc.jclass: every env of the call has J <= jclass) that fits one job per lane.
// (64 jobs inside rows wider than 64 stay with two jobs per lane: the NOPE flag of such an env is byte 64 of its mask row.)
int wave_jpl(const JssDesc &d) {
    if (d.jmax <= kWave) return 1;
    return (d.jclass > 0 && d.jclass < kWave) ? 1 : 2;
}

// Two envs per wavefront, one after the other (jss_wave_env.hpp, wave_block2): the one-step modes of the one-wavefront-per-env
// flavour with one job per lane and per-env tables (full or medium records).  Measured (profiles/r06_misc/two_per_wave_ab.txt,
// wave_timeline_two_per_wave.txt): with half the wavefronts a launch of 8 192 envs is 15-18 % SLOWER (4 wavefronts per SIMD are
// latency-bound: a wavefront's two steps take 26.7 k cycles where one took 16.3 k), 16 384 envs 9-10 % slower, and only from
// about three rounds of resident wavefronts per launch on does the form come out ahead (65 536 envs in two or three
// sub-batches: +6-7 %) -- there the second env's state arrives under the first env's step instead of at the head of a new
// wavefront's life.  Hence the threshold; JssDesc.kernel's JSS_KERNEL_ONE / TWO_ENVS_PER_WAVE bits override it per call.
#ifndef JSS_TWO_PER_WAVE_MIN_BATCH
#define JSS_TWO_PER_WAVE_MIN_BATCH 20480
#endif
template <int MODE>
bool two_per_wave(const JssDesc &d, int G, int class_j) {
    if (MODE != kRollout1 && MODE != kStep) return false;
    if (G || class_j > kWave || d.n_tables == 1) return false;
    if (d.kernel & JSS_KERNEL_ONE_ENV_PER_WAVE) return false;
    return (d.kernel & JSS_KERNEL_TWO_ENVS_PER_WAVE) || d.batch >= JSS_TWO_PER_WAVE_MIN_BATCH;
}

template <int MODE, int TAB>
KernelFn pick_tab(int G, int jpl) {
    if (G == 16) return jss_packed_kernel<16, MODE, TAB>;
    if (G == 32) return jss_packed_kernel<32, MODE, TAB>;
    if (jpl == 1) return jss_kernel<1, MODE, TAB>;
    return jss_kernel<2, MODE, TAB>;
}
template <int MODE>
KernelFn pick(int G, int jpl, bool shared, int record_ints) {
    if (!shared) return record_ints == JSS_NFM ? pick_tab<MODE, kTabGlobalM>(G, jpl) : pick_tab<MODE, kTabGlobal>(G, jpl);
    return record_ints == JSS_NFC ? pick_tab<MODE, kTabLdsC>(G, jpl) : pick_tab<MODE, kTabLds>(G, jpl);
}

template <int MODE>
KernelFn pick_two(int record_ints) {       // (instantiated for the one-step modes only)
    if constexpr (MODE == kRollout1 || MODE == kStep)
        return record_ints == JSS_NFM ? jss_kernel_two<MODE, kTabGlobalM> : jss_kernel_two<MODE, kTabGlobal>;
    else return nullptr;
}

struct LaunchPlan {
    KernelFn fn;
    int envs_per_block;
    size_t shmem;
    bool two;               // one-wavefront-per-env flavour, two envs per wavefront
};

constexpr size_t kMaxDynamicLds = 64 * 1024;   // available to a workgroup without raising the function attribute

// The head of the LDS layout, which the plain launches (plan) and the step session (plan_session) share: the staged table
// of a shared-table batch, one observation image per wavefront and, for the packed flavour (G lanes per env), the move
// and normaliser areas behind them.  packed_obs_rows: job rows per env of the packed image -- the two plans size it
// differently, see their calls; with_obs == false: the mode writes no observation.
void lds_layout(Params &p, int G, int packed_obs_rows, bool with_obs) {
    p.region_ints = p.d.jmax * p.d.mmax;
    p.table_lds_ints = p.d.n_tables == 1 ? ((p.region_ints + 3) & ~3) : 0;
    if (G) {
        p.obs_wave_floats = with_obs ? ((kWave / G) * packed_obs_rows * 7 + 3) & ~3 : 0;
        p.mv_off_ints = p.table_lds_ints + kWavesPerBlock * p.obs_wave_floats;
        p.norm_off_ints = p.mv_off_ints + kBlock;                       // one int per lane (six used per group), kTabGlobal
    } else {
        p.obs_wave_floats = with_obs ? (p.d.jmax * 7 + 3 + 3) & ~3 : 0;   // + up to 3 floats of alignment shift (store_obs)
        if (p.obs_wave_floats < kWave) p.obs_wave_floats = kWave;      // unpack_env borrows it: one int per machine
        p.mv_off_ints = p.norm_off_ints = 0;
    }
}

// Fills the launch-derived fields of `p` (LDS layout) from the whole batch's description.
template <int MODE>
int plan(Params &p, LaunchPlan &lp, bool by_class = false) {
    const bool shared = p.d.n_tables == 1;
    const int G = packed_group(p.d, by_class);
    // (kLookahead writes no observation; packed image: min(jmax, G) rows -- jmax > G is a class inside padded rows)
    lds_layout(p, G, p.d.jmax < G ? p.d.jmax : G, MODE != kLookahead);
    lp.two = false;
    if (G) {
        lp.envs_per_block = (kWave / G) * kWavesPerBlock;
        lp.shmem = sizeof(int32_t) * ((size_t)p.norm_off_ints + (shared ? 0 : kBlock));
    } else {
        lp.two = !by_class && two_per_wave<MODE>(p.d, G, p.d.jmax);      // (the fused grid keeps one env per wavefront: its classes are parts of a batch)
        lp.envs_per_block = kWavesPerBlock * (lp.two ? 2 : 1);
        lp.shmem = sizeof(int32_t) * ((size_t)p.table_lds_ints + kWavesPerBlock * p.obs_wave_floats);
    }
#ifdef JSS_PROFILING
    p.ablate = g_ablate;
    p.stamps = g_stamps;
    lp.shmem += g_lds_pad;
#endif
    // (the shared-table packed rollout / lookahead kernels keep the rule of a jss_rule_* call in static LDS on top: rule_source)
    const size_t static_lds = G && rule_source(MODE, shared ? kTabLds : kTabGlobal) == kRwLds ? kRuleLdsBytes : 0;
    if (lp.shmem + static_lds > kMaxDynamicLds) return JSS_E_LDS;
    lp.fn = by_class ? nullptr : lp.two ? pick_two<MODE>(p.d.record_ints) : pick<MODE>(G, wave_jpl(p.d), shared, p.d.record_ints);   // (the grid has its own kernel)
    return 0;
}

// ---- step session ---------------------------------------------------------------------------------------
template <int TAB>
KernelFn pick_session_tab(int G, int jpl) {
    if (G == 16) return jss_packed_session_kernel<16, TAB>;
    if (G == 32) return jss_packed_session_kernel<32, TAB>;
    if (jpl == 1) return jss_session_kernel<1, TAB>;
    return jss_session_kernel<2, TAB>;
}
KernelFn pick_session(int G, int jpl, bool shared, int record_ints) {
    if (!shared) return record_ints == JSS_NFM ? pick_session_tab<kTabGlobalM>(G, jpl) : pick_session_tab<kTabGlobal>(G, jpl);
    return record_ints == JSS_NFC ? pick_session_tab<kTabLdsC>(G, jpl) : pick_session_tab<kTabLds>(G, jpl);
}

struct SessionInfo {          // what jss_session_wait needs to know about an open session (keyed by its progress pointer)
    int active_waves;         // wavefronts that own at least one env set: the progress words the waiter sweeps
    int slots;
    long long timeout_ticks;
};
std::mutex g_sessions_mutex;
std::unordered_map<const void *, SessionInfo> g_sessions;

constexpr size_t kMaxSessionLds = 96 * 1024;       // per workgroup
constexpr size_t kSessionLdsPerCu = 96 * 1024;     // of a CU's 160 KB, all resident workgroups of the session together
constexpr long long kTicksPerMs = 100000;        // the wall clock of the device counts at 100 MHz

// LDS layout, grid and residency of a session over the batch `p` describes with `slots` env sets per wavefront.
// Fits = every workgroup is resident at once AND the chip keeps room for the caller's own kernels (post, wait, the
// policy network): see the two budgets at the end.
int plan_session(Params &p, LaunchPlan &lp, int slots, int *blocks_out, int *active_out) {
    const bool shared = p.d.n_tables == 1, compact = p.d.record_ints == JSS_NFC;
    const int G = packed_group(p.d);
    // A session knows no shape classes: jobs per lane go by jmax alone where plan honours JssDesc.jclass (wave_jpl), and
    // the packed observation image has jmax rows where plan's has min(jmax, G) -- the same for every batch a session takes
    const int jpl = p.d.jmax <= kWave ? 1 : 2;
    lds_layout(p, G, p.d.jmax, true);
    p.slots = slots;
    int envs_per_wave, park4;                        // park4: int4 per parked env set of one wavefront
    if (G) {
        envs_per_wave = kWave / G;
        p.norm_slot_ints = shared ? 0 : kBlock;
        p.park_off_ints = p.norm_off_ints + (shared ? 0 : slots * kBlock);
        park4 = (compact ? 1 : p.d.record_ints == JSS_NFM ? 2 : 3) * kWave + 8;
    } else {
        envs_per_wave = 1;
        p.norm_slot_ints = 0;
        p.park_off_ints = p.table_lds_ints + kWavesPerBlock * p.obs_wave_floats;
        park4 = (compact ? jpl : 2 * jpl) * kWave + kWave / 4 + 1;   // (medium records: lo + hi rows like full ones)
    }
    lp.shmem = sizeof(int32_t) * ((size_t)p.park_off_ints + (slots > 1 ? (size_t)kWavesPerBlock * slots * park4 * 4 : 0));
    if (lp.shmem > kMaxSessionLds) return JSS_E_RESIDENT;
    lp.fn = pick_session(G, jpl, shared, p.d.record_ints);
    lp.envs_per_block = envs_per_wave * kWavesPerBlock * slots;
    const int sets = (p.d.batch + envs_per_wave - 1) / envs_per_wave;
    const int waves = (sets + slots - 1) / slots;
    const int blocks = (waves + kWavesPerBlock - 1) / kWavesPerBlock;
    if (lp.shmem > kMaxDynamicLds &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(lp.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lp.shmem) != hipSuccess) {
        (void)hipGetLastError();
        return JSS_E_LDS;
    }
    int dev = 0, n_cu = 0, occ = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, reinterpret_cast<const void *>(lp.fn), kBlock, 0) != hipSuccess)
        return (int)hipGetLastError();
    // Registers / wave slots: the occupancy query overstates what the hardware admits when a kernel uses more than 80
    // SGPRs (these do: 6 workgroups per CU at most, MI355X_MICROARCH.md "Residency"); two workgroup slots per CU stay
    // free.  LDS: the session takes at most kSessionLdsPerCu of a CU's 160 KB, so that a kernel of the caller that
    // asks for up to 64 KB always finds room next to it.
    if (occ > 6) occ = 6;
    int usable = occ - 2;
    const int by_lds = (int)(kSessionLdsPerCu / (lp.shmem ? lp.shmem : 1));
    if (by_lds < usable) usable = by_lds;
    if (usable < 1 || blocks > usable * n_cu) return JSS_E_RESIDENT;
    *blocks_out = blocks;
    *active_out = blocks * kWavesPerBlock < sets ? blocks * kWavesPerBlock : sets;
    return 0;
}

// mail[(step % depth) * B + i] = (step + 1) << 32 | action, steps [first, first + n): one thread per env
__global__ void jss_session_post_kernel(unsigned long long *mail, const int32_t *actions, int batch, int depth, int first, int n) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= batch) return;
    for (int k = 0; k < n; ++k) {
        const int step = first + k;
        const int a = actions ? actions[(size_t)k * batch + i] : JSS_ACTION_CLOSE;
        wt_store(mail + (size_t)(step % depth) * batch + i, ((unsigned long long)(unsigned)(step + 1) << 32) | (unsigned)a);
    }
}

// returns once every active wavefront has published `steps_done` steps (one workgroup sweeps the progress words);
// bounded: gives up -- status[1] += 1 -- after the session's timeout or as soon as a wavefront of the session has
__device__ __forceinline__ void session_wait(const int32_t *progress, int32_t *status, int active, int steps_done, long long timeout_ticks) {
    __shared__ int behind;     // 1: somebody has not published `steps_done` yet; 2: give up (decided by thread 0 for the workgroup)
    long long t0 = 0;
    for (unsigned spins = 0;; ++spins) {
        if (threadIdx.x == 0) behind = 0;
        __syncthreads();
        int mine = 0;
        for (int i = (int)threadIdx.x; i < active; i += (int)blockDim.x) mine |= fresh_load(progress + i) < steps_done ? 1 : 0;
        if (mine) behind = 1;
        __syncthreads();
        if (threadIdx.x == 0 && behind) {
            // ONE thread reads the status word and the clock and decides for everybody: wavefronts that looked for themselves
            // (each at its own instant, with its own t0) could disagree, and one of them would leave the others at the barrier
            bool give_up = fresh_load(status + 0) != 0;                      // a wavefront of the session timed out: it is dead
            if ((spins & 63u) == 63u) {
                const long long now = wall_clock64();
                if (t0 == 0) t0 = now;
                else if (now - t0 > timeout_ticks) give_up = true;
            }
            if (give_up) {
                atomicAdd(status + 1, 1);
                behind = 2;
            }
        }
        __syncthreads();
        const int b = behind;
        __syncthreads();                                                     // (everybody has read it before thread 0 clears it)
        if (b != 1) return;
        __builtin_amdgcn_s_sleep(1);
    }
}
__global__ void jss_session_wait_kernel(const int32_t *progress, int32_t *status, int active, int steps_done, long long timeout_ticks) {
    session_wait(progress, status, active, steps_done, timeout_ticks);
}
// post of one step, and the first workgroup waits for it
__global__ void jss_session_step_kernel(unsigned long long *mail, const int32_t *actions, int batch, int depth, int step,
                                        const int32_t *progress, int32_t *status, int active, long long timeout_ticks) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < batch)
        wt_store(mail + (size_t)(step % depth) * batch + i, ((unsigned long long)(unsigned)(step + 1) << 32) | (unsigned)actions[i]);
    if (blockIdx.x == 0) session_wait(progress, status, active, step + 1, timeout_ticks);
}

int fire(const Params &p, const LaunchPlan &lp, void *stream) {
    if (p.d.batch == 0) return 0;
    const int blocks = (p.d.batch + lp.envs_per_block - 1) / lp.envs_per_block;
    hipLaunchKernelGGL(lp.fn, dim3(blocks), dim3(kBlock), lp.shmem, reinterpret_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

template <int MODE>
int launch(Params &p, void *stream) {
    LaunchPlan lp;
    const int rc = plan<MODE>(p, lp);
    return rc ? rc : fire(p, lp, stream);
}

Params params_of(const JssDesc *desc, const JssState *state, const JssOut *out) {     // out == NULL: the call writes none
    Params p = {};
    p.d = *desc;
    p.s = *state;
    if (out) p.o = *out;
    return p;
}

// ps[i] = params_of(set i), then each(ps[i], i) for what the sets of a jss_multi_* call differ in
template <class Each>
void params_of_sets(Params *ps, int n, const JssDesc *const *descs, const JssState *const *states, const JssOut *const *outs,
                    Each &&each) {
    for (int i = 0; i < n; ++i) {
        ps[i] = params_of(descs[i], states[i], outs ? outs[i] : nullptr);
        each(ps[i], i);
    }
}

// The description of envs [start, start + count) of the batch `p` describes, for the step-type modes: every per-env
// pointer moves (jss_env_rows.hpp, and the three below that are no state or output rows); the instance tables stay (an
// env's header names its table by its index in the WHOLE batch's tables, so n_tables keeps describing those).  Not a
// description a reset may be launched with -- except the whole batch, sub_batch(p, 0, batch), which is `p` itself.
Params sub_batch(const Params &p, int start, int count) {
    Params q = p;
    const size_t s0 = (size_t)start;
    q.d.batch = count;
    if (p.d.table_of_env) q.d.table_of_env = p.d.table_of_env + s0;
    if (p.d.env_ids) q.d.env_ids = p.d.env_ids + s0;
    q.d.env_id_base = p.d.env_id_base + start;
    for_each_env_row(p.d, q.s, q.o, [s0](auto *&rows, size_t bytes, bool) {
        if (rows) rows = reinterpret_cast<decltype(+rows)>(reinterpret_cast<char *>(rows) + s0 * bytes);
    });
    return q;
}

// How a batch is cut into at most n_sub contiguous parts: boundaries at multiples of 64 envs (whole workgroups, 16-byte
// aligned rows); a part that would start behind the batch is dropped, the last part is shorter.  Returns the number of parts.
struct Part {
    int start, count;
};
int cut(int batch, int n_sub, Part *parts) {
    const int chunk = (((batch + n_sub - 1) / n_sub) + 63) & ~63;
    int n = 0;
    for (int start = 0; n < n_sub && start < batch; start += chunk) parts[n++] = Part{start, batch - start < chunk ? batch - start : chunk};
    return n;
}

// A window of n_steps steps over n_parts parts, part i on streams[i]: step s of a part depends only on its own step
// s - 1, so one part's drain overlaps another's fill.  launch_part(i, streams[i]) launches ONE step of part i and returns
// its error.  fork_join (JSS_ROLLOUT_FORK_JOIN; only with more than one part): the side streams start behind streams[0]
// and streams[0] continues behind them all -- every stream is joined even when a launch failed (join_streams), and the
// launch error wins over the join error.
template <class LaunchPart>
int issue_window(int n_parts, void *const *streams, int n_steps, bool fork_join, LaunchPart &&launch_part) {
    fork_join = fork_join && n_parts > 1;
    ForkJoinEvents *ev = nullptr;
    int rc = 0;
    if (fork_join && ((rc = events_for(streams[0], &ev)) || (rc = fork_streams(*ev, streams, n_parts)))) return rc;
    for (int s = 0; s < n_steps && !rc; ++s)
        for (int i = 0; i < n_parts && !rc; ++i) rc = launch_part(i, streams[i]);
    const int jrc = fork_join ? join_streams(*ev, streams, n_parts) : 0;
    return rc ? rc : jrc;
}

// ---- several independent env sets in ONE grid (jss_multi_*) ------------------------------------------------------
// The shape classes of a ragged population (jssenv_amd.BucketedJssEnv: 16-lane groups, 32-lane groups, one wavefront per
// env, two jobs per lane) are compact batches of their own.  Launched one by one they need one launch per class and step
// and -- to overlap -- one stream each, at the mercy of how HIP deals streams onto hardware queues (round 4: 0.37-0.55 of
// the roofline for the same work, depending on the box).  Here ONE grid covers them all: a workgroup finds its env set by
// its index (block ranges, scalar compares on kernel arguments) and runs that set's body -- the same device functions
// the plain kernels are made of -- on its own Params.  The sets with the longest-lived wavefronts come first in the
// grid, so that the short ones fill the tail.  Per-env-table layouts only (an LDS-staged shared table would add four
// more bodies); other sets make the entry points fall back to one launch per set on the same stream.
constexpr int kMultiMaxSets = 6;
enum MultiFlavour { kMfW2G = 0, kMfW1G = 1, kMfP32G = 2, kMfP32M = 3, kMfP16G = 4, kMfP16M = 5, kMfNone = 6 };   // grid order
struct MultiParams {
    Params p[kMultiMaxSets];
    int32_t block_end[kMultiMaxSets];   // first workgroup index behind set i
    int32_t flavour[kMultiMaxSets];
    int32_t n_sets;
};

#ifndef JSS_MULTI_STEP_MIN_BLOCKS
#define JSS_MULTI_STEP_MIN_BLOCKS 5
#endif
// kLogits (jss_multi_step_logits): 5, like the grid's kStep -- 73 VGPRs, 6 wavefronts per SIMD as kStep's 74, no scratch
// (6 compiles to 74 VGPRs with more SGPRs parked in VGPR lanes; the default 8 would cap it at 64 VGPRs and spill)
#ifndef JSS_MULTI_LOGITS_MIN_BLOCKS
#define JSS_MULTI_LOGITS_MIN_BLOCKS 5
#endif
constexpr int multi_min_blocks(int mode) {
    return mode == kStep ? JSS_MULTI_STEP_MIN_BLOCKS : mode == kRollout1 ? 7 : mode == kReset ? 6
         : mode == kLogits ? JSS_MULTI_LOGITS_MIN_BLOCKS : 8;
}

template <int MODE>
__global__ __launch_bounds__(kBlock, multi_min_blocks(MODE)) void jss_multi_kernel(MultiParams mp) {
    HIP_DYNAMIC_SHARED(int32_t, lds)
    const int blk = (int)blockIdx.x;
    int k = 0;
#pragma unroll
    for (int i = 0; i + 1 < kMultiMaxSets; ++i)
        if (i + 1 < mp.n_sets && blk >= mp.block_end[i]) k = i + 1;
    const int block = blk - (k ? mp.block_end[k - 1] : 0);
    // The set's Params copied up front -- every field loaded in the entry block, behind the state loads, like a kernel that
    // takes them by value -- rather than read in place at their uses (-DJSS_MULTI_PARAMS_IN_PLACE: no spilled SGPRs instead of
    // 30, and 3 % slower: profiles/r05_misc/bucketed_grid_vs_streams.txt; the same trade as JSS_PARAMS_OF in jss_common.hpp)
#ifdef JSS_MULTI_PARAMS_IN_PLACE
    const Params &p = mp.p[k];
#else
    const Params p = mp.p[k];
#endif
#ifdef JSS_EXP_MULTI_ONLY
    switch (JSS_EXP_MULTI_ONLY) {
#else
    switch (mp.flavour[k]) {
#endif
    case kMfW2G: wave_block<2, MODE, kTabGlobal, false>(p, block, lds); break;   // (one body: 66 VGPRs, no spills at 7 waves / SIMD)
    case kMfW1G: wave_block<1, MODE, kTabGlobal>(p, block, lds); break;
    case kMfP32G: packed_block<32, MODE, kTabGlobal, true>(p, block, lds); break;   // (full records: also classes inside padded rows)
    case kMfP32M: packed_block<32, MODE, kTabGlobalM>(p, block, lds); break;
    case kMfP16G: packed_block<16, MODE, kTabGlobal, true>(p, block, lds); break;
    default: packed_block<16, MODE, kTabGlobalM>(p, block, lds); break;
    }
}

int multi_flavour(const JssDesc &d) {
    if (d.n_tables == 1) return kMfNone;                                  // shared table: LDS-staged bodies are not in the grid
    const int G = packed_group(d, true);
    const bool medium = d.record_ints == JSS_NFM;
    if (G && d.jmax > G && (medium || d.jclass > d.jmax || d.mclass > d.mmax)) return kMfNone;   // a class inside padded rows: full records
    if (d.jclass > d.jmax || d.mclass > d.mmax) return kMfNone;
    if (G == 16) return medium ? kMfP16M : kMfP16G;
    if (G == 32) return medium ? kMfP32M : kMfP32G;
    if (medium) return kMfNone;
    // one job per lane: J <= 64 -- but a 64-job env inside rows wider than 64 keeps its NOPE flag at byte 64 of the mask row,
    // which only the two-jobs-per-lane body writes
    return class_jobs(d, true) <= (d.jmax > kWave ? kWave - 1 : kWave) ? kMfW1G : kMfW2G;
}

// `ps[0..n)`: fully filled Params of the sets (everything but the launch-derived LDS fields).  One fused launch per step when
// every set has a body in the grid, otherwise one plain launch per set and step.  n_sub > 1: every set is cut into n_sub
// contiguous parts (cut) and part i of ALL sets is issued on streams[i] -- as one grid when fused, else one launch per set --
// by issue_window (what jss_rollout_steps does for one set).  Step-type modes only (sub_batch; the reset / policy modes come
// with n_sub == 1, whose one part is the whole set).
template <int MODE>
int launch_multi(Params *ps, int n, int n_steps, int n_sub, void *const *streams, bool fork_join) {
    // No fused body for a combination with a shared-table set, medium records on the one-wavefront-per-env shapes or more
    // than kMultiMaxSets sets: parts and streams are the same either way, so that a caller who asked for overlap gets it.
    bool fused = n >= 2 && n <= kMultiMaxSets;
    for (int i = 0; i < n && fused; ++i) fused = multi_flavour(ps[i].d) != kMfNone;
    constexpr int kMaxParts = 4;                                         // (16 in the single-set calls)
    if (n_sub > kMaxParts) n_sub = kMaxParts;
    int order[16];
    for (int i = 0; i < n; ++i) order[i] = i;
    for (int i = 1; fused && i < n; ++i)                                 // insertion sort by flavour (= grid order), stable
        for (int j = i; j > 0 && multi_flavour(ps[order[j]].d) < multi_flavour(ps[order[j - 1]].d); --j) {
            const int t = order[j]; order[j] = order[j - 1]; order[j - 1] = t;
        }
    // What the two forms plan differs, and stays so (which kernel a launch selects is measured behaviour): unfused, a set is
    // planned WHOLE and its parts launch with that plan (fire() sizes the grid); fused, every part is planned for itself,
    // class-aware, and every grid launches with the largest LDS size over ALL parts.
    LaunchPlan whole[16];
    for (int i = 0; i < n && !fused; ++i)
        if (const int rc = plan<MODE>(ps[i], whole[i])) return rc;
    struct Item { Params p; const LaunchPlan *lp; };
    struct PartWork {                                                    // one part: the grid's argument, or its launches
        MultiParams grid;
        int blocks;
        Item items[16];
        int n_items;
    };
    static PartWork work[kMaxParts];                                     // (10 KB each: not on the stack of every caller)
    static std::mutex work_mutex;
    std::lock_guard<std::mutex> lock(work_mutex);
    Part cuts[16][kMaxParts];
    int n_cuts[16];
    for (int i = 0; i < n; ++i) n_cuts[i] = cut(ps[i].d.batch, n_sub, cuts[i]);
    size_t grid_lds = 0;
    int parts = 0;
    for (int part = 0; part < n_sub; ++part) {
        PartWork &w = work[parts];
        int nb = 0, k = 0;
        for (int q = 0; q < n; ++q) {
            const int i = order[q];
            if (part >= n_cuts[i]) continue;
            Params p = sub_batch(ps[i], cuts[i][part].start, cuts[i][part].count);
            if (fused) {
                LaunchPlan lp;
                if (const int rc = plan<MODE>(p, lp, true)) return rc;   // (fills the LDS layout fields; sized for THIS part)
                nb += (p.d.batch + lp.envs_per_block - 1) / lp.envs_per_block;
                w.grid.p[k] = p;
                w.grid.block_end[k] = nb;
                w.grid.flavour[k] = multi_flavour(p.d);
                if (lp.shmem > grid_lds) grid_lds = lp.shmem;
            } else {
                w.items[k] = Item{p, &whole[i]};
            }
            ++k;
        }
        if (k == 0) continue;
        w.grid.n_sets = w.n_items = k;
        w.blocks = nb;
        ++parts;
    }
    if (parts == 0) return 0;
    return issue_window(parts, streams, n_steps, fork_join, [&](int part, void *stream) {
        const PartWork &w = work[part];
        int rc = 0;
        if (fused) {                                                     // (the arguments are copied at every launch)
            hipLaunchKernelGGL(jss_multi_kernel<MODE>, dim3(w.blocks), dim3(kBlock), grid_lds, reinterpret_cast<hipStream_t>(stream), w.grid);
            rc = (int)hipGetLastError();
        }
        for (int k = 0; !fused && k < w.n_items && !rc; ++k) rc = fire(w.items[k].p, *w.items[k].lp, stream);
        return rc;
    });
}

// kLookahead over the candidates p.la of the batch p describes (lookahead_call)
int launch_lookahead(Params &p, void *stream) {
    // (the widest per-env rows a packed kernel offsets: job records, <= jmax x 32 bytes, and the 48-byte constants record)
    if ((unsigned long long)p.d.batch * ((unsigned long long)p.d.jmax * JSS_NF * 4 + JSS_NC * 4) >= (1ull << 32))
        p.d.kernel |= JSS_KERNEL_WAVE;
    LaunchPlan lp;
    if (const int rc = plan<kLookahead>(p, lp)) return rc;
    const int blocks = (int)(((long long)p.la.n + lp.envs_per_block - 1) / lp.envs_per_block);
    hipLaunchKernelGGL(lp.fn, dim3(blocks), dim3(kBlock), lp.shmem, reinterpret_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

// ---- policy, rollout, lookahead: ONE path each for the stock rules (jss_*), the caller's weighted rules (jss_rule_*,
// include/jss_rules.h) and the caller's key tables (jss_key_*, include/jss_keys.h) ------------------------------------------
// The selector into Params: a stock rule's `kind` as it came; the caller's selectors as kinds of their own, which are no
// JSS_POLICY_* codes, with the rule or the keys in the 16-byte slot the two share.
void apply(Params &p, const SelectorArg &sel) {
    if (sel.which == SelectorArg::kRule) {
        p.kind = kKindWeighted; p.rule = *sel.rule;
    } else if (sel.which == SelectorArg::kKeys) {
        p.kind = kKindKeys; p.keys = *sel.keys;
    } else {
        p.kind = sel.kind;
    }
}

}  // namespace

extern "C" {

int jss_abi_version(void) { return JSS_ABI_VERSION; }

const char *jss_backend(void) { return "hip:gfx950"; }

#ifdef JSS_PROFILING
int jss_profiling_set(int option, int value) {
    if (option == JSS_PROF_LDS_PAD && value >= 0 && value <= 150000) {
        g_lds_pad = value;
        return 0;
    }
    if (option == JSS_PROF_ABLATE) {
        g_ablate = value;
        return 0;
    }
    return JSS_E_KIND;
}
int jss_profiling_stamps(void *device_buffer) {      // [B][16] uint64 (NULL: off)
    g_stamps = static_cast<unsigned long long *>(device_buffer);
    return 0;
}
#endif

const char *jss_error_string(int code) {
    const char *text = arg_error_string(code);
    return text ? text : code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
}

int jss_reset(const JssDesc *desc, const JssState *state, const JssOut *out, const uint8_t *which, void *stream) {
    if (const int rc = check_reset(desc, state, out)) return rc;
    Params p = params_of(desc, state, out);
    p.which = which;
    return launch<kReset>(p, stream);
}

int jss_step(const JssDesc *desc, const JssState *state, const int32_t *actions, const JssOut *out, void *stream) {
    if (const int rc = check_step(desc, state, actions, out)) return rc;
    Params p = params_of(desc, state, out);
    p.actions = actions;
    return launch<kStep>(p, stream);
}

int jss_step_autoreset(const JssDesc *desc, const JssState *state, const int32_t *actions, const JssOut *out, void *stream) {
    if (const int rc = check_step(desc, state, actions, out)) return rc;
    Params p = params_of(desc, state, out);
    p.actions = actions; p.flags = JSS_ROLLOUT_AUTORESET;
    return launch<kStep>(p, stream);
}

// jss_step + the masked categorical draw from the caller's logits in one launch (kLogits: every kernel family kStep has, one
// env per wavefront at a time -- two_per_wave stays off)
int jss_step_logits(const JssDesc *desc, const JssState *state, const JssLogits *lg, uint64_t seed, int32_t flags,
                    const JssOut *out, void *stream) {
    if (const int rc = check_step_logits(desc, state, lg, out)) return rc;
    Params p = params_of(desc, state, out);
    p.lg = *lg; p.seed = seed; p.flags = flags & JSS_ROLLOUT_AUTORESET;
    if (p.lg.row == 0) p.lg.row = desc->jmax + 1;
    return launch<kLogits>(p, stream);
}

int jss_advance(const JssDesc *desc, const JssState *state, const uint8_t *which, int32_t *hole, const JssOut *out,
                void *stream) {
    if (const int rc = check_reset(desc, state, out)) return rc;
    Params p = params_of(desc, state, out);
    p.which = which; p.hole = hole;
    return launch<kAdvance>(p, stream);
}

// The three call shapes.  (They stand here, not with `apply`: the kernel instantiations are emitted in the order in which this
// file first names them, and the code object is held byte for byte to the one that jss_policy and jss_rollout gave here.)
static int policy_call(const JssDesc *desc, const JssState *state, const SelectorArg &sel, uint64_t seed, uint32_t explore_q16,
                       int32_t *actions, void *stream) {
    if (const int rc = check_policy(desc, state, sel, actions)) return rc;
    Params p = params_of(desc, state, nullptr);
    apply(p, sel);
    p.actions_out = actions; p.seed = seed; p.explore_q16 = explore_q16;
    return launch<kPolicy>(p, stream);
}

static int rollout_call(const JssDesc *desc, const JssState *state, const JssOut *out, const SelectorArg &sel, uint64_t seed,
                        uint32_t explore_q16, int32_t n_iter, int32_t flags, void *stream) {
    if (const int rc = check_rollout(desc, state, out, sel, n_iter)) return rc;
    Params p = params_of(desc, state, out);
    apply(p, sel);
    p.seed = seed; p.explore_q16 = explore_q16; p.n_iter = n_iter; p.flags = flags;
    // One iteration of a stock rule runs on the one-step kernels.  The caller's selectors plan kRollout whatever n_iter is:
    // kRollout1 (and kStep) do not carry them.
    return n_iter == 1 && sel.which == SelectorArg::kStock ? launch<kRollout1>(p, stream) : launch<kRollout>(p, stream);
}

// Candidate moves scored by rule rollouts (include/jss_search.h): kLookahead, a group (packed) or a wavefront per candidate,
// the kernel flavour and table layout of the batch as for jss_rollout.  The packed kernels address a parent's rows by a 32-bit
// lane offset from the start of the batch's tensors; a batch too large for that runs on the one-wavefront-per-env kernels,
// which address an env by a wave-uniform 64-bit base.
static int lookahead_call(const JssDesc *desc, const JssState *state, const JssLookahead *la, const SelectorArg &sel,
                          uint64_t seed, uint32_t explore_q16, int32_t n_iter, void *stream) {
    if (const int rc = check_lookahead(desc, state, la, sel, n_iter)) return rc;
    if (la->n == 0) return 0;                         // no candidate: nothing is planned (no JSS_E_LDS), nothing is launched
    Params p = params_of(desc, state, nullptr);
    apply(p, sel);
    p.la = *la; p.seed = seed; p.explore_q16 = explore_q16; p.n_iter = n_iter;
    return launch_lookahead(p, stream);
}

int jss_policy(const JssDesc *desc, const JssState *state, int kind, uint64_t seed, uint32_t explore_q16,
               int32_t *actions, void *stream) {
    return policy_call(desc, state, stock_selector(kind), seed, explore_q16, actions, stream);
}

int jss_rollout(const JssDesc *desc, const JssState *state, const JssOut *out, int kind, uint64_t seed,
                uint32_t explore_q16, int32_t n_iter, int32_t flags, void *stream) {
    return rollout_call(desc, state, out, stock_selector(kind), seed, explore_q16, n_iter, flags, stream);
}

int jss_trajectory(const JssDesc *desc, const JssState *state, const JssOut *out, const JssTraj *traj, int kind,
                   uint64_t seed, uint32_t explore_q16, int32_t n_steps, int32_t flags, void *stream) {
    if (const int rc = check_trajectory(desc, state, out, traj, kind, n_steps)) return rc;
    Params p = params_of(desc, state, out);
    p.t = *traj; p.kind = kind; p.seed = seed; p.explore_q16 = explore_q16;
    p.n_iter = n_steps; p.flags = flags;
    return launch<kTraj>(p, stream);
}

int jss_steps(const JssDesc *desc, const JssState *state, const JssOut *out, const JssTraj *traj, const int32_t *actions,
              int32_t n_steps, void *stream) {
    const int rc = check_steps(desc, state, out, actions, n_steps);
    if (rc || n_steps == 0) return rc;                // (n_steps == 0: nothing to do)
    Params p = params_of(desc, state, out);
    p.actions = actions; p.n_iter = n_steps;
    if (traj) p.t = *traj;
    p.t.action = nullptr;
    return launch<kSteps>(p, stream);
}

int jss_session_open(const JssDesc *desc, const JssState *state, const JssOut *out, const JssSession *session, void *stream) {
    int rc = check_session_open(desc, state, out, session);
    if (rc) return rc;
    const int want = session->slots;
    Params p = params_of(desc, state, out);
    p.mail = reinterpret_cast<const unsigned long long *>(session->mail);
    p.progress = session->progress;
    p.status = session->status;
    p.depth = session->depth;
    p.timeout_ticks = (long long)(session->timeout_ms ? session->timeout_ms : 2000) * kTicksPerMs;
    LaunchPlan lp;
    int blocks = 0, active = 0;
    rc = JSS_E_RESIDENT;
    for (int slots = want ? want : 1; slots <= (want ? want : 8); slots *= 2) {
        rc = plan_session(p, lp, slots, &blocks, &active);
        if (rc != JSS_E_RESIDENT) break;
    }
    if (rc) return rc;
    hipLaunchKernelGGL(lp.fn, dim3(blocks), dim3(kBlock), lp.shmem, reinterpret_cast<hipStream_t>(stream), p);
    const int lrc = (int)hipGetLastError();
    if (lrc) return lrc;
    {   // registered only once the resident kernel is really on its way: wait / step of a session that never opened -> JSS_E_SESSION
        std::lock_guard<std::mutex> lock(g_sessions_mutex);
        g_sessions[session->progress] = SessionInfo{active, p.slots, p.timeout_ticks};
    }
    return 0;
}

int jss_session_post(const JssDesc *desc, const JssSession *session, const int32_t *actions, int32_t first_step,
                     int32_t n_steps, int32_t waited, void *stream) {
    if (const int rc = check_session_post(desc, session, actions, first_step, n_steps, waited)) return rc;
    hipLaunchKernelGGL(jss_session_post_kernel, dim3((desc->batch + kBlock - 1) / kBlock), dim3(kBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), reinterpret_cast<unsigned long long *>(session->mail), actions,
                       desc->batch, session->depth, first_step, n_steps);
    return (int)hipGetLastError();
}

int jss_session_wait(const JssDesc *desc, const JssSession *session, int32_t steps_done, void *stream) {
    if (const int rc = check_session_wait(desc, session, steps_done)) return rc;
    SessionInfo info;
    {
        std::lock_guard<std::mutex> lock(g_sessions_mutex);
        const auto it = g_sessions.find(session->progress);
        if (it == g_sessions.end()) return JSS_E_SESSION;                    // never opened
        info = it->second;
    }
    hipLaunchKernelGGL(jss_session_wait_kernel, dim3(1), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream),
                       session->progress, session->status, info.active_waves, steps_done, info.timeout_ticks);
    return (int)hipGetLastError();
}

int jss_session_step(const JssDesc *desc, const JssSession *session, const int32_t *actions, int32_t step, void *stream) {
    if (const int rc = check_session_step(desc, session, actions, step)) return rc;
    SessionInfo info;
    {
        std::lock_guard<std::mutex> lock(g_sessions_mutex);
        const auto it = g_sessions.find(session->progress);
        if (it == g_sessions.end()) return JSS_E_SESSION;
        info = it->second;
    }
    hipLaunchKernelGGL(jss_session_step_kernel, dim3((desc->batch + kBlock - 1) / kBlock), dim3(kBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), reinterpret_cast<unsigned long long *>(session->mail), actions,
                       desc->batch, session->depth, step, session->progress, session->status, info.active_waves, info.timeout_ticks);
    return (int)hipGetLastError();
}

int jss_session_close(const JssDesc *desc, const JssSession *session, int32_t next_step, void *stream) {
    if (const int rc = check_session_close(desc, session, next_step)) return rc;
    // (the caller has waited for every step it posted: the slot of next_step is free)
    {   // the session is over for the host: wait / step on it answer JSS_E_SESSION from here on (the progress / status buffers
        // may be freed by the caller once its stream has drained)
        std::lock_guard<std::mutex> lock(g_sessions_mutex);
        g_sessions.erase(session->progress);
    }
    hipLaunchKernelGGL(jss_session_post_kernel, dim3((desc->batch + kBlock - 1) / kBlock), dim3(kBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), reinterpret_cast<unsigned long long *>(session->mail),
                       static_cast<const int32_t *>(nullptr), desc->batch, session->depth, next_step, 1);
    return (int)hipGetLastError();
}

int jss_sync_check(void *stream) {
    const hipError_t rc = hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream));
    const hipError_t sticky = hipGetLastError();
    return (int)(rc != hipSuccess ? rc : sticky);
}

int jss_rollout_steps(const JssDesc *desc, const JssState *state, const JssOut *out, int kind, uint64_t seed,
                      uint32_t explore_q16, int32_t n_steps, int32_t flags, int32_t n_sub, void *const *streams) {
    int rc = check_rollout_steps(desc, state, out, kind, n_steps, n_sub, streams);
    if (rc || n_steps == 0) return rc;                // (no step: nothing is launched, nothing is touched)
    Params p = params_of(desc, state, out);
    p.kind = kind; p.seed = seed; p.explore_q16 = explore_q16;
    p.n_iter = 1; p.flags = flags & ~JSS_ROLLOUT_FORK_JOIN;
    LaunchPlan lp;
    if ((rc = plan<kRollout1>(p, lp))) return rc;
    Part parts[16];
    Params sub[16];
    const int n = cut(desc->batch, n_sub, parts);
    for (int i = 0; i < n; ++i) sub[i] = sub_batch(p, parts[i].start, parts[i].count);
    // the kernel form goes by the size of a LAUNCH (two_per_wave): with more than one part, by the first part's -- where
    // jss_multi_rollout's per-set launches keep the whole set's plan (launch_multi)
    if (n > 1 && (rc = plan<kRollout1>(sub[0], lp))) return rc;
    return issue_window(n, streams, n_steps, (flags & JSS_ROLLOUT_FORK_JOIN) != 0,
                        [&](int i, void *stream) { return fire(sub[i], lp, stream); });
}

int jss_policy_step_steps(const JssDesc *desc, const JssState *state, const JssOut *out, int kind, uint64_t seed,
                          uint32_t explore_q16, int32_t *actions, int32_t n_steps, int32_t flags, int32_t n_sub,
                          void *const *streams) {
    int rc = check_policy_step_steps(desc, state, out, kind, actions, n_steps, n_sub, streams);
    if (rc || n_steps == 0) return rc;
    Params pp = params_of(desc, state, nullptr), ps = params_of(desc, state, out);
    pp.actions_out = actions; pp.kind = kind; pp.seed = seed; pp.explore_q16 = explore_q16;
    ps.actions = actions; ps.flags = flags & JSS_ROLLOUT_AUTORESET;
    LaunchPlan lpp, lps;
    if ((rc = plan<kPolicy>(pp, lpp)) || (rc = plan<kStep>(ps, lps))) return rc;
    Part parts[16];
    Params subp[16], subs[16];
    const int n = cut(desc->batch, n_sub, parts);
    for (int i = 0; i < n; ++i) {
        subp[i] = sub_batch(pp, parts[i].start, parts[i].count);
        subp[i].actions_out = actions + parts[i].start;
        subs[i] = sub_batch(ps, parts[i].start, parts[i].count);
        subs[i].actions = actions + parts[i].start;
    }
    if (n > 1 && (rc = plan<kStep>(subs[0], lps))) return rc;           // the kernel form goes by the size of a LAUNCH (two_per_wave), as in jss_rollout_steps
    return issue_window(n, streams, n_steps, (flags & JSS_ROLLOUT_FORK_JOIN) != 0, [&](int i, void *stream) {
        const int prc = fire(subp[i], lpp, stream);
        return prc ? prc : fire(subs[i], lps, stream);
    });
}

int jss_multi_reset(int32_t n_sets, const JssDesc *const *descs, const JssState *const *states, const JssOut *const *outs,
                    const uint8_t *const *which, void *stream) {
    if (const int rc = check_multi_reset(n_sets, descs, states, outs)) return rc;
    Params ps[16];
    params_of_sets(ps, n_sets, descs, states, outs, [&](Params &p, int i) { p.which = which ? which[i] : nullptr; });
    return launch_multi<kReset>(ps, n_sets, 1, 1, &stream, false);
}

int jss_multi_step(int32_t n_sets, const JssDesc *const *descs, const JssState *const *states, const int32_t *const *actions,
                   const JssOut *const *outs, int32_t flags, void *stream) {
    if (const int rc = check_multi_step(n_sets, descs, states, actions, outs)) return rc;
    Params ps[16];
    params_of_sets(ps, n_sets, descs, states, outs, [&](Params &p, int i) {
        p.actions = actions[i];
        p.flags = flags & JSS_ROLLOUT_AUTORESET;
    });
    return launch_multi<kStep>(ps, n_sets, 1, 1, &stream, false);
}

// jss_step_logits over several sets: the fused grid's kLogits bodies (class-aware, as jss_multi_step), or one plain kLogits
// launch per set when the combination has no body in the grid
int jss_multi_step_logits(int32_t n_sets, const JssDesc *const *descs, const JssState *const *states,
                          const JssLogits *const *lgs, uint64_t seed, int32_t flags, const JssOut *const *outs, void *stream) {
    if (const int rc = check_multi_step_logits(n_sets, descs, states, lgs, outs)) return rc;
    Params ps[16];
    params_of_sets(ps, n_sets, descs, states, outs, [&](Params &p, int i) {
        p.lg = *lgs[i]; p.seed = seed; p.flags = flags & JSS_ROLLOUT_AUTORESET;
        if (p.lg.row == 0) p.lg.row = p.d.jmax + 1;
    });
    return launch_multi<kLogits>(ps, n_sets, 1, 1, &stream, false);
}

int jss_multi_policy(int32_t n_sets, const JssDesc *const *descs, const JssState *const *states, int kind, uint64_t seed,
                     uint32_t explore_q16, int32_t *const *actions, void *stream) {
    if (const int rc = check_multi_policy(n_sets, descs, states, kind, actions)) return rc;
    Params ps[16];
    params_of_sets(ps, n_sets, descs, states, nullptr, [&](Params &p, int i) {
        p.actions_out = actions[i]; p.kind = kind; p.seed = seed; p.explore_q16 = explore_q16;
    });
    return launch_multi<kPolicy>(ps, n_sets, 1, 1, &stream, false);
}

int jss_multi_rollout(int32_t n_sets, const JssDesc *const *descs, const JssState *const *states, const JssOut *const *outs,
                      int kind, uint64_t seed, uint32_t explore_q16, int32_t n_steps, int32_t flags, int32_t n_sub,
                      void *const *streams) {
    const int rc = check_multi_rollout(n_sets, descs, states, outs, kind, n_steps, n_sub, streams);
    if (rc || n_steps == 0) return rc;                // (no step: nothing is launched, nothing is touched)
    Params ps[16];
    params_of_sets(ps, n_sets, descs, states, outs, [&](Params &p, int) {
        p.kind = kind; p.seed = seed; p.explore_q16 = explore_q16; p.n_iter = 1; p.flags = flags & JSS_ROLLOUT_AUTORESET;
    });
    return launch_multi<kRollout1>(ps, n_sets, n_steps, n_sub, streams, (flags & JSS_ROLLOUT_FORK_JOIN) != 0);
}

int jss_rollout_steps_multi(int32_t n_sets, const JssDesc *const *descs, const JssState *const *states,
                            const JssOut *const *outs, int kind, uint64_t seed, uint32_t explore_q16, int32_t n_steps,
                            int32_t flags, void *const *streams) {
    int rc = check_rollout_steps_multi(n_sets, descs, states, outs, kind, n_steps, streams);
    if (rc) return rc;
    Params ps[16];
    LaunchPlan lps[16];
    params_of_sets(ps, n_sets, descs, states, outs, [&](Params &p, int i) {
        p.kind = kind; p.seed = seed; p.explore_q16 = explore_q16; p.n_iter = 1; p.flags = flags & ~JSS_ROLLOUT_FORK_JOIN;
        if (!rc) rc = plan<kRollout1>(p, lps[i]);
    });
    if (rc || n_steps == 0) return rc;                // (planned first: unlike the other windowed calls, JSS_E_LDS is still reported with no step)
    return issue_window(n_sets, streams, n_steps, (flags & JSS_ROLLOUT_FORK_JOIN) != 0,
                        [&](int i, void *stream) { return fire(ps[i], lps[i], stream); });
}

// Taillard instances into the envs' own tables (jss_generate.hpp): sparse flags -> 64 envs' flags per wavefront, only the
// flagged ones generated; no flags -> every env, kGenFullPerWave per wavefront
int jss_generate(const JssDesc *desc, const JssState *state, const JssGen *gen, const uint8_t *which, void *stream) {
    if (const int rc = check_generate(desc, state, gen)) return rc;
    if (desc->batch == 0) return 0;
    GenParams g = {};
    g.ops = gen->ops; g.rem = gen->rem; g.inst = gen->inst;
    g.time_seed = gen->time_seed; g.machine_seed = gen->machine_seed; g.actions = gen->actions; g.which = which;
    g.env = gen->time_seed ? nullptr : state->env;
    g.env_ids = desc->env_ids; g.env_id_base = desc->env_id_base; g.seed = gen->seed;
    g.batch = desc->batch; g.jmax = desc->jmax; g.mmax = desc->mmax;
    g.jobs = gen->jobs; g.machines = gen->machines; g.dur_low = gen->dur_low; g.dur_high = gen->dur_high;
    g.per_wave = (which || gen->actions) ? kWave : kGenFullPerWave;
    const long long waves = ((long long)desc->batch + g.per_wave - 1) / g.per_wave;
    const int blocks = (int)((waves + kGenBlock / kWave - 1) / (kGenBlock / kWave));
    hipLaunchKernelGGL(jss_generate_kernel, dim3(blocks), dim3(kGenBlock), 0, reinterpret_cast<hipStream_t>(stream), g);
    return (int)hipGetLastError();
}

// env k <- env src_of_dst[k] (jss_clone.hpp): one wavefront per destination env, one kernel argument per copied tensor
int jss_clone(const JssDesc *dst_desc, const JssState *dst, const JssOut *dst_out, const JssCloneDst *dst_tables,
              const JssDesc *src_desc, const JssState *src, const JssOut *src_out, const int32_t *src_of_dst, void *stream) {
    int mode = 0;
    if (const int rc = check_clone(dst_desc, dst, dst_out, dst_tables, src_desc, src, src_out, src_of_dst, &mode)) return rc;
    if (dst_desc->batch == 0) return 0;
    const long long J = dst_desc->jmax, M = dst_desc->mmax;
    CloneParams p = {};
    // dwordx4 where both rows of every env are 16-byte aligned (row length and both bases), else dwords, else bytes
    auto add = [&](void *d, const void *s, long long bytes) {
        CloneSeg &g = p.seg[p.n_seg++];
        const uintptr_t a = (uintptr_t)d | (uintptr_t)s | (uintptr_t)bytes;
        g.dst = static_cast<char *>(d);
        g.src = static_cast<const char *>(s);
        g.bytes = (int32_t)bytes;
        g.unit = a % 16 == 0 ? 16 : a % 4 == 0 ? 4 : 1;
        g.n = (int32_t)(bytes / g.unit);
    };
    EnvRow to[kMaxEnvRows], from[kMaxEnvRows];       // (one shape, check_clone: the same rows on both sides)
    const int n_rows = cloned_rows(*dst_desc, *dst, *dst_out, to);
    cloned_rows(*src_desc, *src, *src_out, from);
    for (int i = 0; i < n_rows; ++i) add(to[i].base, from[i].base, (long long)to[i].bytes);
    if (mode == 1) add(dst_tables->table_of_env, src_desc->table_of_env, 4);
    if (mode == 2) {
        add(dst_tables->ops, src_desc->ops, J * M * 4);
        add(dst_tables->rem, src_desc->rem, J * M * 4);
        add(dst_tables->inst, src_desc->inst, JSS_NI * 4);
    }
    p.own_tables = mode == 2;
    p.src_of_dst = src_of_dst;
    p.dst_env = dst->env;
    p.batch_dst = dst_desc->batch;
    p.batch_src = src_desc->batch;
    const int per_block = kCloneBlock / kWave;
    const int blocks = (int)(((long long)dst_desc->batch + per_block - 1) / per_block);
    hipLaunchKernelGGL(jss_clone_kernel, dim3(blocks), dim3(kCloneBlock), 0, reinterpret_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

// include/jss_search.h, include/jss_rules.h, include/jss_keys.h: the companions of jss_policy and jss_rollout above
int jss_lookahead(const JssDesc *desc, const JssState *state, const JssLookahead *la, int kind, uint64_t seed,
                  uint32_t explore_q16, int32_t n_iter, void *stream) {
    return lookahead_call(desc, state, la, stock_selector(kind), seed, explore_q16, n_iter, stream);
}

int jss_rule_policy(const JssDesc *desc, const JssState *state, const JssRule *rule, uint64_t seed, uint32_t explore_q16,
                    int32_t *actions, void *stream) {
    return policy_call(desc, state, rule_selector(rule), seed, explore_q16, actions, stream);
}

int jss_rule_rollout(const JssDesc *desc, const JssState *state, const JssOut *out, const JssRule *rule, uint64_t seed,
                     uint32_t explore_q16, int32_t n_iter, int32_t flags, void *stream) {
    return rollout_call(desc, state, out, rule_selector(rule), seed, explore_q16, n_iter, flags, stream);
}

int jss_rule_lookahead(const JssDesc *desc, const JssState *state, const JssLookahead *la, const JssRule *rule,
                       uint64_t seed, uint32_t explore_q16, int32_t n_iter, void *stream) {
    return lookahead_call(desc, state, la, rule_selector(rule), seed, explore_q16, n_iter, stream);
}

int jss_key_policy(const JssDesc *desc, const JssState *state, const JssKeys *keys, uint64_t seed, uint32_t explore_q16,
                   int32_t *actions, void *stream) {
    return policy_call(desc, state, keys_selector(keys), seed, explore_q16, actions, stream);
}

int jss_key_rollout(const JssDesc *desc, const JssState *state, const JssOut *out, const JssKeys *keys, uint64_t seed,
                    uint32_t explore_q16, int32_t n_iter, int32_t flags, void *stream) {
    return rollout_call(desc, state, out, keys_selector(keys), seed, explore_q16, n_iter, flags, stream);
}

int jss_key_lookahead(const JssDesc *desc, const JssState *state, const JssLookahead *la, const JssKeys *keys,
                      uint64_t seed, uint32_t explore_q16, int32_t n_iter, void *stream) {
    return lookahead_call(desc, state, la, keys_selector(keys), seed, explore_q16, n_iter, stream);
}

}  // extern "C"
