// The batch cut and the LDS budget of the staged key pass of the locus sort (vstrains_amd/csrc/vs_pe_plan.h, product source,
// compiled unchanged) on the CPU, for tests/test_locus_plan_cpu.py.  Walks the batches of constructed blocks at every buffer
// capacity exactly as a wavefront of k_locus_count_staged does (vs_locus_batch = the count of vs_locus_in_batch over the
// lanes, vs_locus_span, vs_locus_buf_words), checks every index a staged batch reads or writes against the buffer and the
// block's allocation, and prints the cuts; then prints the plan's staging decision for a list of geometries.
//   W <case> | <woff ...>                       the block: word offsets of its ends, two per pair, n_ends + 1 values
//   B <case> <cap> <lo> <hi> | <n>:<staged> ...  the batches of pairs [lo, hi) at capacity cap, in order
//   P <name> <lds_sort> <per_pass> <stage_words> <lds_bytes>
// No device, no HIP call.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../vstrains_amd/csrc/vs_pe_plan.h"

static const uint32_t PAD_WORDS = 16;  // VS_PAD_WORDS of vs_internal.h: zero words behind a block's packed words

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                              \
        }                                                                         \
    } while (0)

// a block from the word counts of its ends (two per pair)
static std::vector<uint32_t> block(const std::vector<uint32_t> &end_words) {
    std::vector<uint32_t> woff(end_words.size() + 1, 0u);
    for (size_t i = 0; i < end_words.size(); i++) woff[i + 1] = woff[i] + end_words[i];
    return woff;
}

static void walk(const char *name, const std::vector<uint32_t> &woff, uint64_t lo, uint64_t hi, uint32_t cap) {
    const uint32_t n_words = woff.back(), buf_words = vs_locus_buf_words(cap);
    std::vector<uint32_t> buf(buf_words, 0u);  // (indexed below: the sanitizer sees every staged index)
    printf("B %s %u %llu %llu |", name, cap, (unsigned long long)lo, (unsigned long long)hi);
    uint64_t p = lo;
    unsigned guard = 0;
    while (p < hi) {
        const LocusBatch b = vs_locus_batch(woff.data(), p, hi, cap);
        CHECK(b.n >= 1u && b.n <= LOCUS_STAGE_PAIRS && p + b.n <= hi);
        // the kernel's count: the lanes whose pair is in the batch
        uint32_t lanes = 0;
        for (uint32_t t = 0; t < LOCUS_STAGE_PAIRS; t++) {
            const bool exists = p + t < hi;
            lanes += vs_locus_in_batch(exists, woff[2 * p], exists ? woff[2 * (p + t) + 2] : 0u, cap) ? 1u : 0u;
        }
        CHECK(lanes == (b.staged ? b.n : 0u));
        if (b.staged) {
            const uint32_t w_first = woff[2 * p], w_end = woff[2 * (p + b.n)];
            CHECK(w_end - w_first <= cap);
            const LocusSpan sp = vs_locus_span(w_first, w_end);
            CHECK(sp.first <= w_first && w_first - sp.first < 4u && sp.first % 4u == 0u);
            CHECK(sp.quads >= 1u && 4u * sp.quads <= buf_words);                  // every quad stored lies in the buffer
            CHECK(sp.quads <= LOCUS_STAGE_QUADS * 64u);                           // ... and is some lane's load
            CHECK(sp.first + 4u * sp.quads <= n_words + PAD_WORDS);               // ... from inside the block's allocation
            CHECK(sp.first + 4u * sp.quads >= w_end + 4u);                        // the overshoot behind the last pair is staged
            for (uint32_t i = 0; i < 4u * sp.quads; i++) buf[i] = 1u;
            for (uint32_t t = 0; t < b.n; t++) {
                // the forward end of pair p + t: a window read at a seed touches up to two words behind the end's last
                const uint32_t ws = woff[2 * (p + t)], fwd_end = woff[2 * (p + t) + 1];
                for (uint32_t x = ws; x < fwd_end + 2u; x++) CHECK(buf[x - sp.first] == 1u);
            }
            for (uint32_t i = 0; i < 4u * sp.quads; i++) buf[i] = 0u;
        } else {
            CHECK(b.n == 1u && woff[2 * p + 2] - woff[2 * p] > cap);  // its own two ends do not fit
        }
        printf(" %u:%u", b.n, b.staged);
        p += b.n;
        CHECK(++guard < 100000u);
    }
    CHECK(p == hi);
    const LocusBatch none = vs_locus_batch(woff.data(), hi, hi, cap);  // an empty chunk, or the end of one
    CHECK(none.n == 0u);
    printf("\n");
}

static void cuts(const char *name, const std::vector<uint32_t> &end_words, uint32_t cap_max) {
    const std::vector<uint32_t> woff = block(end_words);
    const uint64_t n_pairs = end_words.size() / 2;
    printf("W %s |", name);
    for (uint32_t v : woff) printf(" %u", v);
    printf("\n");
    for (uint32_t cap = 1; cap <= cap_max; cap++) {
        walk(name, woff, 0, n_pairs, cap);
        if (n_pairs > 7) walk(name, woff, 3, n_pairs - 2, cap);  // a chunk inside the block: its last batch partial
    }
    for (uint32_t cap : {1104u, (uint32_t)LOCUS_STAGE_MAX}) walk(name, woff, 0, n_pairs, cap);  // (what the plan gives at configs[2], and the most it ever gives)
    walk(name, woff, n_pairs / 2, n_pairs / 2, 64u);  // a chunk of no pairs
    if (n_pairs) walk(name, woff, n_pairs - 1, n_pairs, 64u);  // ... of one
}

static void plan_line(const char *name, uint32_t n_nodes, int locus_stage, bool locus_global, uint64_t n_pairs = 10000000, uint32_t max_len = 150) {
    PePlanIn in;
    in.n_nodes = n_nodes; in.K = STD_K; in.w = STD_W; in.s = STD_S;
    in.n_seed_pos = 3500000; in.n_distinct = 1000000; in.max_node_len = 30000; in.n_cu = 256;
    in.n_ends = 2 * n_pairs; in.max_len = max_len;
    in.count = true;
    in.tune.locus_stage = locus_stage;
    in.tune.locus_global = locus_global;
    const PePlan p = vs_pe_plan(in);
    CHECK(p.status == VS_OK);
    printf("P %s %u %u %u %llu\n", name, p.lds_sort, p.locus_per_pass, p.locus_stage_words, (unsigned long long)p.locus_lds_bytes);
}

int main() {
    std::vector<uint32_t> e;
    // 2 x 150 bases: ten words an end
    e.assign(2 * 150, 10u);
    cuts("uniform", e, 70);
    // ends of no words: a singles block (every odd end absent), and whole pairs of nothing
    e.clear();
    for (int p = 0; p < 160; p++) { e.push_back(p % 7 == 3 ? 0u : 10u); e.push_back(0u); }
    cuts("singles", e, 40);
    e.assign(2 * 140, 0u);
    cuts("nothing", e, 4);
    // mixed lengths: 2 x 250 among 2 x 150, short ends, a pair of one word
    e.clear();
    for (int p = 0; p < 200; p++) {
        const uint32_t f = p % 13 == 5 ? 16u : p % 5 == 1 ? 2u : 10u, r = p % 13 == 5 ? 16u : p % 11 == 2 ? 1u : 10u;
        e.push_back(f);
        e.push_back(r);
    }
    cuts("mixed", e, 80);
    // every pair larger than most capacities
    e.assign(2 * 9, 33u);
    cuts("oversize", e, 70);
    e.assign(2, 10u);
    cuts("one", e, 24);
    e.clear();
    cuts("empty", e, 3);

    plan_line("config2", 5039, -1, false);
    plan_line("config2_off", 5039, 0, false);
    plan_line("config2_48", 5039, 48, false);
    plan_line("config2_257", 5039, 257, false);
    plan_line("config2_huge", 5039, 1000000, false);
    plan_line("config2_global", 5039, -1, true);
    plan_line("small_block", 5039, -1, false, 4096);
    plan_line("no_sort", 5039, -1, false, 4095);
    plan_line("keys_9000", 8998, -1, false);
    plan_line("keys_10000", 9998, -1, false);
    plan_line("len_176", 5039, -1, false, 10000000, 176);
    plan_line("len_177", 5039, -1, false, 10000000, 177);
    plan_line("len_250", 5039, -1, false, 10000000, 250);
    plan_line("len_250_huge", 5039, 1000000, false, 10000000, 250);
    plan_line("keys_36863", 36861, -1, false);
    plan_line("keys_36863_64", 36861, 64, false);
    plan_line("keys_36864", 36862, -1, false);
    plan_line("keys_36864_64", 36862, 64, false);
    plan_line("multipass", 54000, -1, false);
    plan_line("multipass_64", 54000, 64, false);
    plan_line("beyond_lds", 150000, -1, false);
    return 0;
}
