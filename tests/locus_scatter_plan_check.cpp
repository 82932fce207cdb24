// The launch rule of k_locus_scatter (vstrains_amd/csrc/vs_pe_plan.h, product source, compiled unchanged) on the CPU, for
// tests/test_locus_scatter_cases_cpu.py: the plan's locus_scatter_keys for a list of graphs and blocks, and the launches the
// host loop of pe_launch makes from it (walked here as it walks them), each checked: the ranges tile [0, keys) in order, none
// is empty, none exceeds a pass's LDS cursors.
//   S <n_nodes> <n_pairs> <VS_LOCUS_SCATTER> | <keys> <per_pass> <scatter_keys> <launches>
// No device, no HIP call.
#include <stdio.h>
#include <stdlib.h>

#include "../vstrains_amd/csrc/vs_pe_plan.h"

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                              \
        }                                                                         \
    } while (0)

static void plan(uint32_t n_nodes, uint64_t n_pairs, int scatter) {
    PePlanIn in;
    in.n_nodes = n_nodes; in.K = STD_K; in.w = STD_W; in.s = STD_S;
    in.n_seed_pos = 3500000; in.n_distinct = 1000000; in.max_node_len = 30000; in.n_cu = 256;
    in.n_ends = 2 * n_pairs; in.max_len = 150;
    in.count = true;
    in.tune.locus_scatter = scatter;
    const PePlan p = vs_pe_plan(in);
    CHECK(p.status == 0 && p.use_sort && p.lds_sort);
    const uint64_t nk = p.locus_keys;
    CHECK(p.locus_scatter_keys >= 1u && p.locus_scatter_keys <= p.locus_per_pass);
    uint32_t launches = 0;
    uint64_t covered = 0;
    for (uint32_t key_lo = 0; key_lo < nk; key_lo += p.locus_scatter_keys) {  // (pe_launch's loop)
        const uint32_t n_here = (uint32_t)(nk - key_lo < p.locus_scatter_keys ? nk - key_lo : p.locus_scatter_keys);
        CHECK(key_lo == covered && n_here >= 1u && n_here <= p.locus_per_pass);
        covered += n_here;
        launches++;
    }
    CHECK(covered == nk);
    printf("S %u %llu %d | %llu %u %u %u\n", n_nodes, (unsigned long long)n_pairs, scatter, (unsigned long long)nk, p.locus_per_pass,
           p.locus_scatter_keys, launches);
}

int main() {
    const uint64_t sizes[] = {4096, 4097, 1u << 20, LOCUS_SCATTER_PAIRS, LOCUS_SCATTER_PAIRS + 1u, 2u * LOCUS_SCATTER_PAIRS + 1u, 10000000, 100000000};
    for (uint32_t n_nodes : {1u, 600u, 5039u, 36861u, 36862u, 40000u, 54000u, 147000u})
        for (uint64_t n_pairs : sizes) plan(n_nodes, n_pairs, 0);
    for (uint32_t n_nodes : {600u, 40000u})
        for (uint64_t n_pairs : {(uint64_t)4097, (uint64_t)2097153})
            for (int scatter : {1, 1024, 2500, 1048577}) plan(n_nodes, n_pairs, scatter);
    return 0;
}
