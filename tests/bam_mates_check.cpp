// The by-name matching of vs_bam_core.h as plain C++ under AddressSanitizer and UBSan: every buffer on the heap and exactly
// as long as the data (window, record list, hash, table, lists), so that a read or write one element beyond any of them is
// caught.  Records of a few names (a prefix of another, a differing last byte, l_read_name 1 and 255, bytes >= 0x80), with
// dropped records between them, are matched in one window and in two windows cut after EVERY record -- the second being
// [the waiting records of the first, whole][the rest], as the stream builds it -- at table sizes 2, 4 and the production
// size and hash widths 64, 2 and 0; pairs, their order and the waiting set must be the sequential FIFO rule's.  A table
// too small for the names must end in its status word, not beyond the table.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

#include "../vstrains_amd/csrc/vs_bam_core.h"

#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                               \
        }                                                           \
    } while (0)

static uint32_t rng_state = 777u;
static uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

struct Rec {
    std::string name;  // without the terminator
    uint32_t flag, l_seq;
};

static void put32(std::vector<uint8_t> &v, uint32_t x) {
    for (int k = 0; k < 4; k++) v.push_back((uint8_t)(x >> (8 * k)));
}

static std::vector<uint8_t> encode(const Rec &r) {
    std::vector<uint8_t> v;
    const uint32_t l_name = (uint32_t)r.name.size() + 1u, bs = 32u + l_name + (r.l_seq + 1u) / 2u + r.l_seq;
    put32(v, bs);
    put32(v, 0xFFFFFFFFu);
    put32(v, 0xFFFFFFFFu);
    v.push_back((uint8_t)l_name);
    v.push_back(0);
    v.push_back(0x48);
    v.push_back(0x12);
    v.push_back(0);
    v.push_back(0);
    v.push_back((uint8_t)r.flag);
    v.push_back((uint8_t)(r.flag >> 8));
    put32(v, r.l_seq);
    put32(v, 0xFFFFFFFFu);
    put32(v, 0xFFFFFFFFu);
    put32(v, 0);
    for (char c : r.name) v.push_back((uint8_t)c);
    v.push_back(0);
    for (uint32_t i = 0; i < (r.l_seq + 1u) / 2u + r.l_seq; i++) v.push_back((uint8_t)rnd());
    return v;
}

static int cls_of(uint32_t flag) {
    if (flag & 0x900u) return BAM_C_DROP900;
    if (!(flag & 1u) || ((flag >> 6) & 1u) == ((flag >> 7) & 1u)) return BAM_C_OTHER;
    return (flag & 0x40u) ? BAM_C_FIRST : BAM_C_SECOND;
}

typedef std::vector<std::pair<uint32_t, uint32_t>> Pairs;

// the sequential rule over records idx[0..): pairs (first, second) as positions in idx, and what waits
static void sequential(const std::vector<Rec> &recs, const std::vector<uint32_t> &idx, Pairs &pairs, std::vector<uint32_t> &waiting) {
    std::vector<uint32_t> wait;  // positions, oldest first
    for (uint32_t k = 0; k < idx.size(); k++) {
        const Rec &r = recs[idx[k]];
        const int c = cls_of(r.flag);
        if (c > BAM_C_SECOND) continue;
        size_t hit = wait.size();
        for (size_t w = 0; w < wait.size() && hit == wait.size(); w++)
            if (recs[idx[wait[w]]].name == r.name && cls_of(recs[idx[wait[w]]].flag) == 1 - c) hit = w;
        if (hit == wait.size()) {
            wait.push_back(k);
            continue;
        }
        pairs.push_back(c == BAM_C_FIRST ? std::make_pair(k, wait[hit]) : std::make_pair(wait[hit], k));
        wait.erase(wait.begin() + (long)hit);
    }
    waiting = wait;
}

// one window of records idx[0..) through the header with exactly sized buffers; table size `size` (0: the production
// size).  Returns 0 and the pairs / waiting as positions in idx; *full: the status word of a table too small.
static int window(const std::vector<Rec> &recs, const std::vector<uint32_t> &idx, uint32_t size, uint32_t bits, Pairs &pairs,
                  std::vector<uint32_t> &waiting, bool *full, uint64_t *crowded) {
    std::vector<uint8_t> bytes;
    for (uint32_t i : idx) {
        const std::vector<uint8_t> e = encode(recs[i]);
        bytes.insert(bytes.end(), e.begin(), e.end());
    }
    const uint64_t n = bytes.size();
    uint8_t *win = (uint8_t *)malloc(n ? n : 1);
    if (n) memcpy(win, bytes.data(), n);
    const uint32_t n_rec = (uint32_t)idx.size();
    uint32_t *rec4 = (uint32_t *)malloc(sizeof(uint32_t) * 4u * (n_rec ? n_rec : 1));
    std::vector<uint32_t> part_v;
    uint64_t p = 0;
    for (uint32_t k = 0; k < n_rec; k++) {
        uint64_t nx = 0;
        CHECK(bam_step(win, n, p, &nx) == BAM_STEP_OK && nx <= n);
        const BamRec r = bam_classify(win, p);
        rec4[4u * k] = r.off;
        rec4[4u * k + 1u] = r.flag_cls;
        rec4[4u * k + 2u] = r.l_seq;
        rec4[4u * k + 3u] = r.seq_off;
        CHECK((int)(r.flag_cls >> 16) == cls_of(recs[idx[k]].flag));
        if ((r.flag_cls >> 16) <= (uint32_t)BAM_C_SECOND) part_v.push_back(k);
        p = nx;
    }
    CHECK(p == n);
    const uint32_t np = (uint32_t)part_v.size();
    if (!size) size = bam_table_size(np);
    CHECK(size >= 2u && (size & (size - 1u)) == 0u);
    uint32_t *part = (uint32_t *)malloc(sizeof(uint32_t) * (np ? np : 1));
    if (np) memcpy(part, part_v.data(), sizeof(uint32_t) * np);
    uint64_t *hash = (uint64_t *)malloc(sizeof(uint64_t) * (np ? np : 1));
    uint32_t *table = (uint32_t *)malloc(sizeof(uint32_t) * size), *head = (uint32_t *)malloc(sizeof(uint32_t) * size);
    uint32_t *slot = (uint32_t *)malloc(sizeof(uint32_t) * (np ? np : 1)), *next = (uint32_t *)malloc(sizeof(uint32_t) * (np ? np : 1));
    uint32_t *rank = (uint32_t *)malloc(sizeof(uint32_t) * (np ? np : 1));
    uint32_t *out_pairs = (uint32_t *)malloc(sizeof(uint32_t) * (np ? np : 1)), *out_wait = (uint32_t *)malloc(sizeof(uint32_t) * (np ? np : 1));
    const BamMates m = {win, rec4, part, n_rec, np, hash, table, head, size, slot, next, rank};
    uint64_t info[4];
    bam_mates_serial(m, bits, out_pairs, np / 2u, out_wait, np, info);
    *full = info[3] != 0;
    *crowded = info[2];
    if (!*full && info[2] == ~0ull) {
        CHECK(2u * info[0] + info[1] == np);
        for (uint64_t k = 0; k < info[0]; k++) pairs.push_back(std::make_pair(out_pairs[2u * k], out_pairs[2u * k + 1u]));
        for (uint64_t k = 0; k < info[1]; k++) waiting.push_back(out_wait[k]);
    }
    free(out_wait); free(out_pairs); free(rank); free(next); free(slot); free(head); free(table); free(hash); free(part); free(rec4); free(win);
    return 0;
}

int main() {
    // names: the empty one (l_read_name 1), 254 bytes (l_read_name 255), a prefix of another, a last byte that differs, high bytes
    const std::string long_a(254, 'x'), long_b = std::string(253, 'x') + "y";
    const std::string names[8] = {"", long_a, long_b, "read", "read1", "read2", std::string("\xff\x80q"), std::string("\xff\x81q")};
    const uint32_t flags[8] = {0x41, 0x81, 0x51, 0x91, 0x41, 0x81, 0x141, 0x0};
    CHECK(bam_table_size(0) == 2 && bam_table_size(1) == 2 && bam_table_size(2) == 4 && bam_table_size(3) == 8 && bam_table_size(1000) == 2048);
    uint64_t windows = 0, checked = 0;
    for (uint32_t n_names : {2u, 4u, 8u}) {
        std::vector<Rec> recs;
        for (uint32_t i = 0; i < 48; i++) recs.push_back(Rec{names[rnd() % n_names], flags[rnd() % 8u], rnd() % 40u});
        std::vector<uint32_t> all(recs.size());
        for (uint32_t i = 0; i < all.size(); i++) all[i] = i;
        Pairs want;
        std::vector<uint32_t> want_wait;
        sequential(recs, all, want, want_wait);
        for (uint32_t size : {2u, 4u, 0u})
            for (uint32_t bits : {64u, 2u, 0u})
                for (uint32_t cut = 0; cut <= recs.size(); cut++) {
                    // window 1: records [0, cut); window 2: [its waiting records][cut, end)
                    std::vector<uint32_t> one(all.begin(), all.begin() + cut), two;
                    Pairs p1, p2, got;
                    std::vector<uint32_t> w1, w2;
                    bool full = false;
                    uint64_t crowded = ~0ull;
                    if (window(recs, one, size, bits, p1, w1, &full, &crowded)) return 1;
                    windows++;
                    if (size && size < n_names) {
                        if (full) continue;  // (more names than slots: said, and nothing beyond the table touched)
                    }
                    CHECK(!full && crowded == ~0ull);
                    for (auto &pr : p1) got.push_back(std::make_pair(one[pr.first], one[pr.second]));
                    for (uint32_t w : w1) two.push_back(one[w]);
                    two.insert(two.end(), all.begin() + cut, all.end());
                    if (window(recs, two, size, bits, p2, w2, &full, &crowded)) return 1;
                    windows++;
                    if (size && size < n_names && full) continue;
                    CHECK(!full && crowded == ~0ull);
                    for (auto &pr : p2) got.push_back(std::make_pair(two[pr.first], two[pr.second]));
                    CHECK(got == want);
                    std::vector<uint32_t> left;
                    for (uint32_t w : w2) left.push_back(two[w]);
                    CHECK(left == want_wait);
                    checked += got.size();
                }
    }
    // 64 firsts and 64 seconds of one name: accepted, the j-th with the j-th; a 65th first: refused, naming the newest
    {
        std::vector<Rec> recs;
        for (uint32_t i = 0; i < 64; i++) recs.push_back(Rec{"many", 0x41, 3});
        for (uint32_t i = 0; i < 64; i++) recs.push_back(Rec{"many", 0x81, 3});
        std::vector<uint32_t> all(recs.size());
        for (uint32_t i = 0; i < all.size(); i++) all[i] = i;
        Pairs p;
        std::vector<uint32_t> w;
        bool full = false;
        uint64_t crowded = 0;
        if (window(recs, all, 2, 64, p, w, &full, &crowded)) return 1;
        CHECK(!full && crowded == ~0ull && p.size() == 64 && w.empty());
        for (uint32_t j = 0; j < 64; j++) CHECK(p[j].first == j && p[j].second == 64u + j);
        recs.insert(recs.begin() + 10, Rec{"many", 0x41, 3});
        recs.push_back(Rec{"other", 0x41, 3});
        all.resize(recs.size());
        for (uint32_t i = 0; i < all.size(); i++) all[i] = i;
        p.clear();
        if (window(recs, all, 0, 64, p, w, &full, &crowded)) return 1;
        CHECK(!full && crowded == 128 && p.empty() && w.empty());
        // (a list far longer than the cap: every walk still ends)
        for (uint32_t i = 0; i < 400; i++) recs.push_back(Rec{"many", (i & 1u) ? 0x41u : 0x81u, 1});
        all.resize(recs.size());
        for (uint32_t i = 0; i < all.size(); i++) all[i] = i;
        if (window(recs, all, 0, 0, p, w, &full, &crowded)) return 1;
        CHECK(!full && crowded == recs.size() - 1u);
    }
    printf("windows matched: %llu, pairs checked: %llu\nOK\n", (unsigned long long)windows, (unsigned long long)checked);
    return 0;
}
