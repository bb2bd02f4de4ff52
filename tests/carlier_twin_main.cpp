// tests/carlier_twin_main.cpp -- a stand-alone driver of the host-core twin's jss_machine_solve and jss_bottleneck_exact
// (include/jss_carlier.h): the header's textbook case and the "hand" and "repeats" cases of tests/machine_cases.py, solved under
// two masks and built, at budgets of 1, 2 and 100 nodes.  tests/test_carlier.py compiles it together with
// jssenv_amd/csrc/jss_cpu.cpp under AddressSanitizer and UndefinedBehaviorSanitizer, runs it as a child process and compares the
// printed lines with the NumPy mirrors.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "jss_carlier.h"

namespace {

struct Batch {
    int J, M, B;
    std::vector<int32_t> ops, inst, env, env_const, job, machine, solution;
    JssDesc desc;
    JssState state;
    // B envs of one J x M instance, the last one never reset; the rows a relaxation does not read are there and zero
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

void print_row(const char *label, const std::vector<int32_t> &row, size_t count) {
    printf(" %s", label);
    for (size_t e = 0; e < count; ++e) printf(" %d", row[e]);
}

int carlier_case(const char *name, Batch &b) {
    const int region = b.J * b.M, B = b.B;
    std::vector<int32_t> base((size_t)region);
    for (int j = 0; j < b.J; ++j)
        for (int k = 0; k < b.M; ++k) base[j * b.M + k] = k * b.J + j;         // acyclic for every subset of machines
    const int budgets[3] = {1, 2, 100};
    for (int nodes : budgets) {
        const uint64_t masks[2] = {0, 1};
        for (uint64_t mask : masks) {
            std::vector<uint64_t> fixed((size_t)B, mask), proved((size_t)B, 77);
            std::vector<int32_t> length(B, -7), bound(B, -7), neck(B, -7), opt((size_t)B * b.M, -7), low((size_t)B * b.M, -7), used((size_t)B * b.M, -7);
            std::vector<int32_t> head((size_t)B * region, -7), tail((size_t)B * region, -7), rank_out((size_t)B * region, -7);
            JssMachineSolve ms = JssMachineSolve();
            ms.n = B, ms.stride = 0, ms.nodes = nodes, ms.rank = base.data(), ms.fixed = fixed.data();
            ms.length = length.data(), ms.lower_bound = bound.data(), ms.bottleneck = neck.data();
            ms.opt = opt.data(), ms.low = low.data(), ms.nodes_used = used.data(), ms.proved = proved.data();
            ms.head = head.data(), ms.tail = tail.data(), ms.rank_out = rank_out.data();
            const int rc = jss_machine_solve(&b.desc, &b.state, &ms, nullptr);
            if (rc) return printf("%s: rc %d\n", name, rc), 1;
            if (length[B - 1] != -1 || head[(size_t)(B - 1) * region] != -7 || proved[B - 1] != 77) return printf("%s: the env never reset\n", name), 1;
            printf("%s solve %d %llu length %d bound %d neck %d", name, nodes, (unsigned long long)mask, length[0], bound[0], neck[0]);
            print_row("opt", opt, b.M), print_row("low", low, b.M), print_row("nodes", used, b.M);
            printf(" proved %llu", (unsigned long long)proved[0]);
            print_row("head", head, region), print_row("tail", tail, region), print_row("rank", rank_out, region);
            printf("\n");
            ms.rank_out = const_cast<int32_t *>(ms.rank);
            if (jss_machine_solve(&b.desc, &b.state, &ms, nullptr) != JSS_E_NULL) return 1;      // (rank_out aliases rank)
        }
        const int reopts[2] = {0, 2};
        for (int reopt : reopts) {
            std::vector<int32_t> makespan(B, -7), rank((size_t)B * region, -7), info((size_t)B * JSS_EXACT_NI, -7), order((size_t)B * b.M, -7);
            JssBottleneckExact be = JssBottleneckExact();
            be.n = B, be.reopt = reopt, be.nodes = nodes, be.makespan = makespan.data(), be.rank = rank.data(), be.info = info.data(), be.order = order.data();
            const int rc = jss_bottleneck_exact(&b.desc, &b.state, &be, nullptr);
            if (rc) return printf("%s: rc %d\n", name, rc), 1;
            if (makespan[B - 1] != -1 || rank[(size_t)(B - 1) * region] != -7) return printf("%s: the env never reset\n", name), 1;
            printf("%s build %d %d makespan %d", name, nodes, reopt, makespan[0]);
            print_row("info", info, JSS_EXACT_NI), print_row("order", order, b.M), print_row("rank", rank, region);
            printf("\n");
        }
    }
    // candidates through parents, two refused among them, without the optional outputs
    const int parents[4] = {0, 7, 0, -1};
    std::vector<int32_t> makespan(4, -7), rank((size_t)4 * region, -7);
    JssBottleneckExact be = JssBottleneckExact();
    be.n = 4, be.reopt = 1, be.nodes = 3, be.parents = parents, be.makespan = makespan.data(), be.rank = rank.data();
    if (jss_bottleneck_exact(&b.desc, &b.state, &be, nullptr)) return 1;
    printf("%s candidates %d %d %d %d\n", name, makespan[0], makespan[1], makespan[2], makespan[3]);
    be.nodes = 0;
    if (jss_bottleneck_exact(&b.desc, &b.state, &be, nullptr) != JSS_E_SHAPE) return 1;
    be.nodes = JSS_CARLIER_MAX_NODES + 1;
    return jss_bottleneck_exact(&b.desc, &b.state, &be, nullptr) != JSS_E_SHAPE;
}

}  // namespace

int main() {
    const int text_machine[21] = {1, 0, 2, 1, 0, 2, 1, 0, 2, 1, 0, 2, 1, 0, 2, 1, 0, 2, 1, 0, 2};
    const int text_duration[21] = {11, 5, 8, 14, 6, 27, 12, 7, 25, 21, 4, 22, 31, 3, 9, 1, 6, 18, 31, 2, 1};
    const int hand_machine[9] = {1, 0, 2, 2, 0, 1, 2, 1, 0}, hand_duration[9] = {5, 2, 3, 1, 3, 3, 3, 3, 1};
    const int rep_machine[12] = {0, 0, 1, 3, 1, 0, 0, 1, 3, 1, 1, 0}, rep_duration[12] = {3, 5, 2, 4, 6, 1, 1, 7, 2, 2, 9, 3};
    Batch textbook(7, 3, 2, text_machine, text_duration), hand(3, 3, 3, hand_machine, hand_duration), repeats(3, 4, 4, rep_machine, rep_duration);
    if (carlier_case("textbook", textbook) || carlier_case("hand", hand) || carlier_case("repeats", repeats)) return 1;
    printf("CARLIER-TWIN-OK\n");
    return 0;
}
