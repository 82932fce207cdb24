// vs_bam_core.h as plain C++ under AddressSanitizer and UBSan: every buffer on the heap and exactly as long as the data,
// so that a read one byte beyond a window, a table or an entry list is caught.  Records with pseudo-random name, quality
// and aux bytes (fake block_size fields among them) are chained; the window is cut at EVERY length and scanned at several
// segment sizes; the result must be the plain serial walk's.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../vstrains_amd/csrc/vs_bam_core.h"

static uint32_t rng_state = 12345u;
static uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

static void put32(std::vector<uint8_t> &v, uint32_t x) {
    for (int k = 0; k < 4; k++) v.push_back((uint8_t)(x >> (8 * k)));
}

static void add_record(std::vector<uint8_t> &v, uint32_t flag, uint32_t l_seq, uint32_t l_name, uint32_t aux) {
    const uint32_t bs = 32u + l_name + (l_seq + 1u) / 2u + l_seq + aux;
    put32(v, bs);
    put32(v, 0xFFFFFFFFu);
    put32(v, 0xFFFFFFFFu);
    v.push_back((uint8_t)l_name);
    v.push_back(0);
    v.push_back(0x48);
    v.push_back(0x12);
    v.push_back(0);
    v.push_back(0);
    v.push_back((uint8_t)flag);
    v.push_back((uint8_t)(flag >> 8));
    put32(v, l_seq);
    put32(v, 0xFFFFFFFFu);
    put32(v, 0xFFFFFFFFu);
    put32(v, 0);
    for (uint32_t i = 0; i < l_name + (l_seq + 1u) / 2u + l_seq + aux; i++) {
        // (mostly small values, so that four bytes in a row often read as a plausible block_size, sometimes one below 32)
        const uint32_t r = rnd();
        v.push_back((uint8_t)((r & 7u) == 0 ? r >> 3 : (r & 7u) == 1 ? 40u + ((r >> 3) & 63u) : 0u));
    }
}

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);     \
            return 1;                                                   \
        }                                                               \
    } while (0)

struct Plain {
    std::vector<uint64_t> starts;
    int end;
    uint64_t stop;
};

static Plain plain_walk(const uint8_t *w, uint64_t n, uint64_t start) {
    Plain out;
    uint64_t p = start;
    out.end = BAM_END_CLEAN;
    while (p < n) {
        uint64_t nx = 0;
        const int st = bam_step(w, n, p, &nx);
        if (st == BAM_STEP_NEED || (st == BAM_STEP_OK && nx > n)) { out.end = BAM_END_CUT; break; }
        if (st == BAM_STEP_DEAD) { out.end = BAM_END_DEAD; break; }
        out.starts.push_back(p);
        p = nx;
    }
    out.stop = out.end == BAM_END_CLEAN ? n : p;
    return out;
}

static int scan(const std::vector<uint8_t> &all, uint64_t n, uint64_t start, uint32_t seg, uint64_t *n_checked) {
    // exactly sized copies
    uint8_t *w = (uint8_t *)malloc(n ? n : 1);
    memcpy(w, all.data(), n);
    const uint64_t n_seg = (n + seg - 1u) / seg;
    uint16_t *tab = (uint16_t *)malloc(sizeof(uint16_t) * (n ? n : 1));
    uint32_t *entry = (uint32_t *)malloc(sizeof(uint32_t) * (n_seg ? n_seg : 1));
    for (uint64_t s = 0; s < n_seg; s++) entry[s] = BAM_NONE;
    for (uint64_t s = 0; s < n_seg; s++) bam_seg_exits_serial(w, n, s * seg, (s + 1u) * seg < n ? (s + 1u) * seg : n, tab);
    uint64_t stop = n;
    const int end = start < n ? bam_walk(w, n, tab, seg, start, entry, &stop) : BAM_END_CLEAN;
    const Plain want = plain_walk(w, n, start);
    CHECK(end == want.end);
    CHECK(stop == want.stop);
    size_t k = 0;
    for (uint64_t s = 0; s < n_seg; s++) {
        if (entry[s] == BAM_NONE) continue;
        uint64_t p = entry[s], at = 0;
        while (bam_seg_next(w, n, (s + 1u) * seg < n ? (s + 1u) * seg : n, &p, &at)) {
            CHECK(k < want.starts.size() && want.starts[k] == at);
            const BamRec r = bam_classify(w, at);
            CHECK(r.off == at);
            if ((r.flag_cls >> 16) != (uint32_t)BAM_C_MALFORMED) {
                uint32_t sum = 0;
                for (uint32_t i = 0; i < r.l_seq; i++) sum += bam_base(w + r.seq_off, r.l_seq, (r.flag_cls & 0x10u) != 0, i);
                CHECK(r.l_seq == 0 || sum != 0);
            }
            k++;
        }
    }
    CHECK(k == want.starts.size());
    *n_checked += k;
    free(entry);
    free(tab);
    free(w);
    return 0;
}

int main() {
    const char *letters = "=ACMGRSVTWYHKDBN", *comp = "=TGKCYSBAWRDMHVN";
    for (uint32_t c = 0; c < 16; c++) {
        CHECK(bam_letter(c) == (uint8_t)letters[c]);
        CHECK(bam_letter(bam_complement(c)) == (uint8_t)comp[c]);
    }
    const uint8_t two[2] = {0x12, 0x48};  // A C G T
    CHECK(bam_base(two, 4, false, 0) == 'A' && bam_base(two, 4, false, 3) == 'T' && bam_base(two, 3, true, 0) == 'C' && bam_base(two, 3, true, 2) == 'T');
    std::vector<uint8_t> all;
    const uint32_t start = 7;  // (bytes in front: the rest of a header)
    for (uint32_t i = 0; i < start; i++) all.push_back(0xEE);
    const uint32_t flags[6] = {0x41, 0x91, 0x141, 0x0, 0xC1, 0x881};
    for (uint32_t i = 0; i < 40; i++) add_record(all, flags[i % 6], i == 3 ? 0 : i == 4 ? 1 : 20 + (rnd() % 100), 1 + (rnd() % 30), i == 17 ? 700 : rnd() % 40);
    // a malformed record (l_seq beyond its block_size) and a long jump
    const size_t mal = all.size();
    add_record(all, 0x41, 50, 5, 0);
    all[mal + 20] = 0xFF;
    all[mal + 21] = 0xFF;
    add_record(all, 0x81, 60, 5, 70000);
    add_record(all, 0x41, 30, 5, 3);
    uint64_t checked = 0;
    const uint32_t segs[4] = {64, 128, 1000, 4096};
    for (uint32_t seg : segs) {
        const uint64_t step = seg == 64 ? 1 : 37;
        for (uint64_t n = start; n <= all.size(); n += (n < 6000 || n + 200 > all.size()) ? step : 1009)
            if (scan(all, n, start, seg, &checked)) return 1;
        if (scan(all, all.size(), start, seg, &checked)) return 1;
    }
    // a block_size below 32 at a true record start
    std::vector<uint8_t> dead(all.begin(), all.begin() + (long)mal);
    put32(dead, 31);
    for (int i = 0; i < 40; i++) dead.push_back(0);
    for (uint32_t seg : segs)
        if (scan(dead, dead.size(), start, seg, &checked)) return 1;
    printf("records checked: %llu\nOK\n", (unsigned long long)checked);
    return 0;
}
