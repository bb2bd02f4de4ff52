// jssenv_amd/csrc/jss_env_rows.hpp -- which tensors make up one env, and how many bytes one env's row of each is: the ONE
// table of it, shared by libjss_hip.so (sub_batch and jss_clone in jss_kernels.hip) and the host-core twin (jss_clone in
// jss_cpu.cpp).  A tensor added to JssState / JssOut is added here, and every user moves, copies or skips it with the
// rest.  What is not a state or output row -- table_of_env, env_ids, the instance tables a clone may copy -- stays with
// its user.  Plain C++17, no HIP.
#pragma once

#include <cstddef>

#include "jss_abi_checks.hpp"

namespace jss_abi {

// f(pointer member, bytes of one env's row, whether a clone copies it) for every per-env tensor of a batch that passed
// check_args, in the order jss_clone's kernel takes its segments.  `state` / `out` may be const (the pointers are
// read) or not (sub_batch moves them); a member may be NULL where the ABI lets it (counters).
template <class State, class Out, class F>
inline void for_each_env_row(const JssDesc &d, State &state, Out &out, F &&f) {
    const size_t J = (size_t)d.jmax, M = (size_t)d.mmax, R = (size_t)record_ints_of(d);
    f(state.env, JSS_NH * 4, true);
    f(state.env_const, JSS_NC * 4, true);
    f(state.job, J * R * 4, true);
    if (R == JSS_NF) f(state.machine, M * 4, true);       // compact and medium records keep no machine clocks
    f(state.solution, J * M * 4, true);
    f(state.counters, 4 * 8, false);                      // statistics of the env object, not state of the env
    f(out.real_obs, J * 7 * 4, true);
    f(out.action_mask, J + 1, true);
    f(out.reward, 4, true);
    f(out.done, 1, true);
    f(out.makespan, 4, true);
}

// The rows a clone copies as a list: base address and bytes per env.  Two batches of one shape (check_clone) give lists
// of one length with equal sizes, entry by entry.
struct EnvRow {
    char *base;
    size_t bytes;
};
constexpr int kMaxEnvRows = 11;
inline int cloned_rows(const JssDesc &d, const JssState &state, const JssOut &out, EnvRow *rows) {
    int n = 0;
    for_each_env_row(d, state, out, [&](auto *base, size_t bytes, bool cloned) {
        if (cloned) rows[n++] = EnvRow{reinterpret_cast<char *>(base), bytes};
    });
    return n;
}

}  // namespace jss_abi
