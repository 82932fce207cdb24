// The pairing of vs_mates_core.h as plain C++ under AddressSanitizer and UBSan.
//  1. The scan form of the greedy rule, with the lanes of the kernels written as loops: match flags in wavefronts of 64 lanes
//     (their ballot a uint64), workgroups of 256, the composed 1-bit functions carried across wavefronts and workgroups as
//     k_il_match / k_il_carry / k_il_classify carry them -- against the sequential walk (il_step / il_class), on random flag
//     vectors of every density, on all-true vectors (one run) and on runs that start at every offset around 64 and 256.
//  2. il_mates on header lines held in heap buffers exactly as long as the lines, so that a read beyond a token is caught.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../vstrains_amd/csrc/vs_mates_core.h"

#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                               \
        }                                                           \
    } while (0)

static uint32_t rng_state = 4242u;
static uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

static const uint32_t WAVE = 64, TPB = 256;

// classes of n records from their match flags (m[n - 1] is false), the kernels' way
static std::vector<uint32_t> scan_classes(const std::vector<uint8_t> &m) {
    const uint32_t n = (uint32_t)m.size(), wgs = (n + TPB - 1u) / TPB;
    auto ballot = [&](uint32_t base) {
        uint64_t b = 0;
        for (uint32_t l = 0; l < WAVE; l++)
            if (base + l < n && m[base + l]) b |= 1ull << l;
        return b;
    };
    std::vector<uint32_t> wgfn(wgs);
    for (uint32_t g = 0; g < wgs; g++) {  // k_il_match: the workgroup's function
        uint32_t f = IL_F_ID;
        for (uint32_t w = 0; w < TPB / WAVE; w++) f = il_compose(f, il_wave_fn(ballot(g * TPB + w * WAVE)));
        wgfn[g] = f;
    }
    uint32_t p = 0;  // k_il_carry: the parity each workgroup starts with
    for (uint32_t g = 0; g < wgs; g++) {
        const uint32_t f = wgfn[g];
        wgfn[g] = p;
        p = il_apply(f, p);
    }
    std::vector<uint32_t> cls(n);
    for (uint32_t g = 0; g < wgs; g++)  // k_il_classify
        for (uint32_t w = 0; w < TPB / WAVE; w++) {
            uint32_t f = IL_F_ID;
            for (uint32_t v = 0; v < w; v++) f = il_compose(f, il_wave_fn(ballot(g * TPB + v * WAVE)));
            const uint32_t p_in = il_apply(f, wgfn[g]);
            const uint64_t b = ballot(g * TPB + w * WAVE);
            for (uint32_t l = 0; l < WAVE; l++) {
                const uint32_t i = g * TPB + w * WAVE + l;
                if (i < n) cls[i] = il_class(il_wave_parity(b, l, p_in), m[i] != 0);
            }
        }
    return cls;
}

static std::vector<uint32_t> walk_classes(const std::vector<uint8_t> &m) {
    std::vector<uint32_t> cls(m.size());
    uint32_t p = 0;
    for (size_t i = 0; i < m.size(); i++) {
        cls[i] = il_class(p, m[i] != 0);
        p = il_step(p, m[i] != 0);
    }
    return cls;
}

// the greedy rule itself, for the walk to be checked against
static std::vector<uint32_t> greedy_classes(const std::vector<uint8_t> &m) {
    std::vector<uint32_t> cls(m.size());
    for (size_t i = 0; i < m.size();) {
        if (m[i]) {
            cls[i] = IL_FIRST, cls[i + 1] = IL_SECOND;
            i += 2;
        } else {
            cls[i++] = IL_SINGLE;
        }
    }
    return cls;
}

static bool mates_exact(const std::string &a, const std::string &b) {
    uint8_t *pa = (uint8_t *)malloc(a.size() ? a.size() : 1), *pb = (uint8_t *)malloc(b.size() ? b.size() : 1);
    memcpy(pa, a.data(), a.size());
    memcpy(pb, b.data(), b.size());
    const bool r = il_mates(pa, (uint32_t)a.size(), pb, (uint32_t)b.size());
    free(pa);
    free(pb);
    return r;
}

int main() {
    // the function algebra: compose is application in order, for all sixteen pairs
    for (uint32_t f = 0; f < 4; f++)
        for (uint32_t g = 0; g < 4; g++)
            for (uint32_t x = 0; x < 2; x++) CHECK(il_apply(il_compose(f, g), x) == il_apply(g, il_apply(f, x)));
    CHECK(il_ones_below(~0ull, 64) == 64 && il_ones_below(~0ull, 0) == 0 && il_ones_below(~0ull >> 1, 64) == 0 && il_ones_below(0x7ull, 3) == 3);
    CHECK(il_ones_below(0x5ull, 3) == 1 && il_ones_below(0x6ull, 3) == 2 && il_ones_below(1ull << 63, 64) == 1);
    std::vector<std::vector<uint8_t>> vectors;
    for (uint32_t n : {0u, 1u, 2u, 3u, 63u, 64u, 65u, 127u, 128u, 129u, 255u, 256u, 257u, 511u, 512u, 513u, 1000u, 1001u, 2049u, 70000u}) {
        for (uint32_t density : {0u, 1u, 128u, 200u, 250u, 255u, 256u}) {
            std::vector<uint8_t> m(n);
            for (uint32_t i = 0; i + 1 < n; i++) m[i] = (rnd() & 255u) < density;
            vectors.push_back(m);
        }
    }
    for (uint32_t off = 55; off < 70; off++)
        for (uint32_t run = 1; run < 8; run++)
            for (uint32_t edge : {0u, 192u, 448u}) {
                std::vector<uint8_t> m(edge + off + run + 3u);
                for (uint32_t k = 0; k < run; k++) m[edge + off + k] = 1;
                vectors.push_back(m);
            }
    for (const auto &m : vectors) {
        // (a flag vector of the greedy rule: a pair start's successor is never itself tested as a start -- but m is defined for
        // every adjacent couple, so any vector with a false last flag is a legal input)
        const std::vector<uint32_t> want = walk_classes(m);
        CHECK(scan_classes(m) == want);
        // the walk against the greedy rule on the flags it looks at: greedy reads m[i] only at pair starts and singles
        std::vector<uint8_t> seen(m.size());
        for (size_t i = 0; i < m.size(); i++) seen[i] = want[i] != (uint32_t)IL_SECOND && m[i];
        std::vector<uint32_t> g = greedy_classes(seen);
        CHECK(g == want);
    }
    // names
    CHECK(mates_exact("@a", "@a") && !mates_exact("@a", "@b") && !mates_exact("", "") && !mates_exact(" x", " x"));
    CHECK(mates_exact("@a/1", "@a/2") && !mates_exact("@a/2", "@a/1") && mates_exact("@a/1", "@a/1") && !mates_exact("/1", "/2") && mates_exact("/1", "/1"));
    CHECK(mates_exact("@a 1:N", "@a 2:N") && mates_exact("@a\t1", "@a x") && !mates_exact("@abc", "@abcd") && !mates_exact("@abcd", "@abc"));
    CHECK(!mates_exact("@a/1", "@a") && !mates_exact("@a/1", "@b/2") && mates_exact("@a /1", "@a /2"));
    for (uint32_t len = 1; len <= 40; len++)
        for (uint32_t pos = 0; pos < len; pos++) {
            std::string x(len, 'a'), y(len, 'a');
            y[pos] = 'Z';
            CHECK(!mates_exact(x, y) && mates_exact(x, x) && mates_exact(y, y));
        }
    printf("OK\n");
    return 0;
}
