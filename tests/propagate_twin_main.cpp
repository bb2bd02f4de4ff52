// tests/propagate_twin_main.cpp -- a stand-alone driver of the host-core twin's jss_propagate (include/jss_propagate.h): ft06 and
// the "hand" and "repeats" cases of tests/machine_cases.py, propagated under two masks, several trial makespans and budgets, with
// and without a hypothesis, and once more from the windows the call returned.  tests/test_propagate.py compiles it together with
// jssenv_amd/csrc/jss_cpu.cpp under AddressSanitizer and UndefinedBehaviorSanitizer, runs it as a child process and compares the
// printed lines with the NumPy mirror.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "jss_propagate.h"

namespace {

struct Batch {
    int J, M, B;
    std::vector<int32_t> ops, inst, env, env_const, job, machine, solution;
    JssDesc desc;
    JssState state;
    // B envs of one J x M instance, the last one never reset; the rows a propagation does not read are there and zero
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

int propagate_case(const char *name, Batch &b, const int *ubs, int n_ubs) {
    const int region = b.J * b.M, B = b.B;
    std::vector<int32_t> base((size_t)region);
    for (int j = 0; j < b.J; ++j)
        for (int k = 0; k < b.M; ++k) base[j * b.M + k] = k * b.J + j;         // acyclic for every subset of machines
    const int budgets[3] = {1, 2, 256};
    const uint64_t masks[2] = {0, 1};
    for (int passes : budgets)
        for (uint64_t mask : masks)
            for (int u = 0; u < n_ubs; ++u)
                for (int with_hyp = 0; with_hyp < 2; ++with_hyp) {
                    std::vector<uint64_t> fixed((size_t)B, mask);
                    std::vector<int32_t> ub((size_t)B, ubs[u]), hyp_op((size_t)B, 1), hyp_est((size_t)B, 2), hyp_lct((size_t)B, ubs[u] - 1);
                    std::vector<int32_t> status(B, -7), used(B, -7), est((size_t)B * region, -7), lct((size_t)B * region, -7);
                    JssPropagate pr = JssPropagate();
                    pr.n = B, pr.passes = passes, pr.rank = base.data(), pr.fixed = fixed.data(), pr.ub = ub.data();
                    if (with_hyp) pr.hyp_op = hyp_op.data(), pr.hyp_est = hyp_est.data(), pr.hyp_lct = hyp_lct.data();
                    pr.status = status.data(), pr.passes_used = used.data(), pr.est = est.data(), pr.lct = lct.data();
                    int rc = jss_propagate(&b.desc, &b.state, &pr, nullptr);
                    if (rc) return printf("%s: rc %d\n", name, rc), 1;
                    if (status[B - 1] != -1 || used[B - 1] != -7 || est[(size_t)(B - 1) * region] != -7) return printf("%s: the env never reset\n", name), 1;
                    printf("%s prop %d %llu %d %d status %d used %d", name, passes, (unsigned long long)mask, ubs[u], with_hyp, status[0], used[0]);
                    if (status[0] == JSS_PROPAGATE_REFUTED) {
                        if (est[0] != -7 || lct[0] != -7) return printf("%s: a refuted candidate's rows were written\n", name), 1;
                        printf("\n");
                        continue;
                    }
                    print_row("est", est, region), print_row("lct", lct, region);
                    // once more from these windows, as one shared table and without the hypothesis
                    std::vector<int32_t> est_in(est.begin(), est.begin() + region), lct_in(lct.begin(), lct.begin() + region);
                    pr.est_in = est_in.data(), pr.lct_in = lct_in.data(), pr.win_stride = 0, pr.hyp_op = pr.hyp_est = pr.hyp_lct = nullptr;
                    est.assign(est.size(), -1), lct.assign(lct.size(), -1);
                    rc = jss_propagate(&b.desc, &b.state, &pr, nullptr);
                    if (rc) return printf("%s: rc %d\n", name, rc), 1;
                    printf(" again %d %d", status[0], used[0]);
                    print_row("est", est, region), print_row("lct", lct, region);
                    printf("\n");
                    pr.est = const_cast<int32_t *>(pr.est_in);
                    if (jss_propagate(&b.desc, &b.state, &pr, nullptr) != JSS_E_NULL) return 1;         // (est aliases est_in)
                }
    // candidates through parents, two refused among them, without the optional outputs
    const int parents[4] = {0, 7, 0, -1}, ub[4] = {ubs[0], ubs[0], ubs[n_ubs - 1], ubs[0]};
    std::vector<int32_t> status(4, -7);
    JssPropagate pr = JssPropagate();
    pr.n = 4, pr.passes = 3, pr.parents = parents, pr.ub = ub, pr.status = status.data();
    if (jss_propagate(&b.desc, &b.state, &pr, nullptr)) return 1;
    printf("%s candidates %d %d %d %d\n", name, status[0], status[1], status[2], status[3]);
    pr.passes = 0;
    if (jss_propagate(&b.desc, &b.state, &pr, nullptr) != JSS_E_SHAPE) return 1;
    pr.passes = JSS_PROPAGATE_MAX_PASSES + 1;
    return jss_propagate(&b.desc, &b.state, &pr, nullptr) != JSS_E_SHAPE;
}

}  // namespace

int main() {
    const int ft_machine[36] = {2, 0, 1, 3, 5, 4, 1, 2, 4, 5, 0, 3, 2, 3, 5, 0, 1, 4, 1, 0, 2, 3, 4, 5, 2, 1, 4, 5, 0, 3, 1, 3, 5, 0, 4, 2};
    const int ft_duration[36] = {1, 3, 6, 7, 3, 6, 8, 5, 10, 10, 10, 4, 5, 4, 8, 9, 1, 7, 5, 5, 5, 3, 8, 9, 9, 3, 5, 4, 3, 1, 3, 3, 9, 10, 4, 1};
    const int hand_machine[9] = {1, 0, 2, 2, 0, 1, 2, 1, 0}, hand_duration[9] = {5, 2, 3, 1, 3, 3, 3, 3, 1};
    const int rep_machine[12] = {0, 0, 1, 3, 1, 0, 0, 1, 3, 1, 1, 0}, rep_duration[12] = {3, 5, 2, 4, 6, 1, 1, 7, 2, 2, 9, 3};
    const int ft_ubs[5] = {50, 53, 54, 55, 70}, hand_ubs[4] = {10, 11, 12, 20}, rep_ubs[5] = {20, 26, 30, 34, 60};
    Batch ft06(6, 6, 2, ft_machine, ft_duration), hand(3, 3, 3, hand_machine, hand_duration), repeats(3, 4, 4, rep_machine, rep_duration);
    if (propagate_case("ft06", ft06, ft_ubs, 5) || propagate_case("hand", hand, hand_ubs, 4) || propagate_case("repeats", repeats, rep_ubs, 5)) return 1;
    printf("PROPAGATE-TWIN-OK\n");
    return 0;
}
