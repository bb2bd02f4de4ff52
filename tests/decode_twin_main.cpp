// tests/decode_twin_main.cpp -- a stand-alone driver of the host-core twin's jss_decode_keys and jss_keys_evolve
// (include/jss_decode.h): the "hand" and "zeros" cases of tests/decode_cases.py and two generations on plain arrays.
// tests/test_decode.py compiles it together with jssenv_amd/csrc/jss_cpu.cpp under AddressSanitizer and
// UndefinedBehaviorSanitizer, runs it as a child process and compares the printed lines with the NumPy mirrors.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "jss_decode.h"

namespace {

struct Batch {
    int J, M, B;
    std::vector<int32_t> ops, inst, env, env_const, job, machine, solution;
    JssDesc desc;
    JssState state;
    // B envs of one J x M instance, the last one never reset; the rows a decode does not read are there and zero
    Batch(int J_, int M_, int B_, const int *mach, const int *dur) : J(J_), M(M_), B(B_) {
        ops.assign((size_t)J * M, 0);
        for (int e = 0; e < J * M; ++e) ops[e] = mach[e] << 16 | dur[e];
        inst.assign(64, 0), env.assign((size_t)B * 64, 0), env_const.assign((size_t)B * JSS_NC, 0);
        job.assign((size_t)B * J * 64, 0), machine.assign((size_t)B * M, 0), solution.assign((size_t)B * J * M, 0);
        for (int i = 0; i + 1 < B; ++i) env_const[i * JSS_NC + JSS_C_JOBS] = J, env_const[i * JSS_NC + JSS_C_MACHINES] = M;
        desc = JssDesc();
        desc.batch = B, desc.jmax = J, desc.mmax = M, desc.n_tables = 1, desc.threads = 2;
        desc.ops = ops.data(), desc.inst = inst.data();
        state = JssState();
        state.env = env.data(), state.env_const = env_const.data(), state.job = job.data(), state.machine = machine.data();
        state.solution = solution.data();
    }
};

int decode_case(const char *name, Batch &b, const int *keys) {
    const int region = b.J * b.M;
    std::vector<int32_t> table(keys, keys + region);
    const int deltas[3] = {65536, 32768, 0};
    for (int delta : deltas) {
        std::vector<int32_t> makespan(b.B, -7), start((size_t)b.B * region, -7), info((size_t)b.B * JSS_DECODE_NI, -7);
        JssDecode dc = JssDecode();
        dc.n = b.B, dc.stride = 0, dc.delta_q16 = delta, dc.keys = table.data();
        dc.makespan = makespan.data(), dc.start = start.data(), dc.info = info.data();
        const int rc = jss_decode_keys(&b.desc, &b.state, &dc, nullptr);
        if (rc) return printf("%s: rc %d\n", name, rc), 1;
        if (makespan[b.B - 1] != -1 || start[(size_t)(b.B - 1) * region] != -7) return printf("%s: the env never reset\n", name), 1;
        printf("%s %d makespan %d info %d %d %d %d start", name, delta, makespan[0], info[0], info[1], info[2], info[3]);
        for (int e = 0; e < region; ++e) printf(" %d", start[e]);
        printf("\n");
    }
    // per-candidate tables and deltas through parents, a refused candidate among them
    const int parents[4] = {0, 5, 0, 1}, delta_of[4] = {0, 0, 65537, 65536};
    std::vector<int32_t> tables;
    for (int c = 0; c < 4; ++c) tables.insert(tables.end(), table.begin(), table.end());
    std::vector<int32_t> makespan(4, -7);
    JssDecode dc = JssDecode();
    dc.n = 4, dc.stride = region, dc.parents = parents, dc.delta_of = delta_of, dc.keys = tables.data(), dc.makespan = makespan.data();
    if (jss_decode_keys(&b.desc, &b.state, &dc, nullptr)) return 1;
    printf("%s candidates %d %d %d %d\n", name, makespan[0], makespan[1], makespan[2], makespan[3]);
    return 0;
}

int evolve_case() {
    const int G = 3, P = 8, region = 12;
    std::vector<int32_t> keys_in((size_t)G * P * region), keys_out(keys_in.size(), -7), fitness(G * P), by_rank(G * P, -7);
    for (size_t x = 0; x < keys_in.size(); ++x) keys_in[x] = (int32_t)(x * 2654435761u);
    for (int i = 0; i < G * P; ++i) fitness[i] = i % 5 == 3 ? -1 : (i * 7) % 4;
    JssEvolve ev = JssEvolve();
    ev.groups = G, ev.pop = P, ev.region = region, ev.n_elite = 2, ev.n_mutant = 2, ev.rho_q16 = 45875, ev.generation = 4;
    ev.seed = 0x0123456789ABCDEFULL;
    ev.fitness = fitness.data(), ev.keys_in = keys_in.data(), ev.keys_out = keys_out.data(), ev.by_rank = by_rank.data();
    if (jss_keys_evolve(&ev, nullptr)) return 1;
    uint32_t sum = 0;
    for (size_t x = 0; x < keys_out.size(); ++x) sum = sum * 31u + (uint32_t)keys_out[x];
    printf("evolve checksum %u by_rank", sum);
    for (int i = 0; i < G * P; ++i) printf(" %d", by_rank[i]);
    printf("\n");
    // an initial population: nothing is read
    ev.n_elite = 0, ev.n_mutant = P, ev.fitness = nullptr, ev.keys_in = nullptr, ev.by_rank = nullptr, ev.generation = 0;
    if (jss_keys_evolve(&ev, nullptr)) return 1;
    sum = 0;
    for (size_t x = 0; x < keys_out.size(); ++x) sum = sum * 31u + (uint32_t)keys_out[x];
    printf("fresh checksum %u\n", sum);
    ev.keys_in = keys_out.data();
    ev.n_elite = 1, ev.n_mutant = 1;
    if (jss_keys_evolve(&ev, nullptr) != JSS_E_NULL) return 1;           // (no fitness, and keys_out == keys_in)
    return 0;
}

}  // namespace

int main() {
    const int hand_machine[9] = {1, 0, 2, 2, 0, 1, 2, 1, 0}, hand_duration[9] = {5, 2, 3, 1, 3, 3, 3, 3, 1};
    const int hand_keys[9] = {3, 8, 4, 5, 1, 3, 9, 5, 0};
    const int zeros_machine[12] = {0, 1, 2, 1, 0, 2, 2, 2, 0, 0, 2, 1}, zeros_duration[12] = {0, 3, 0, 2, 0, 0, 0, 0, 0, 4, 0, 1};
    const int zeros_keys[12] = {1, 5, 2, 7, 7, 0, 3, 3, 9, 1, 2, 8};
    Batch hand(3, 3, 3, hand_machine, hand_duration), zeros(4, 3, 3, zeros_machine, zeros_duration);
    if (decode_case("hand", hand, hand_keys) || decode_case("zeros", zeros, zeros_keys) || evolve_case()) return 1;
    printf("DECODE-TWIN-OK\n");
    return 0;
}
