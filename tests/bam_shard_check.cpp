// The summary of a share and the plan of the sharded BAM open (vstrains_amd/csrc/vs_bam_core.h) as plain C++ with its own
// main: exactly sized heap buffers for every share, so that a read beyond the bytes a rank holds, or a table index beyond a
// window's limit, is an error AddressSanitizer sees; UBSan for the arithmetic.  Against a naive walk of the chain.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../vstrains_amd/csrc/vs_bam_core.h"

static uint32_t rng_state = 12345u;
static uint32_t rnd(uint32_t n) {
    rng_state = rng_state * 1664525u + 1013904223u;
    return (rng_state >> 8) % n;
}

static void put32(std::vector<uint8_t> &v, uint32_t x) {
    for (int i = 0; i < 4; i++) v.push_back((uint8_t)(x >> (8 * i)));
}

// a record with these flags, l_seq bases and `extra` bytes of anything behind the quality (fake size fields among them)
static void record(std::vector<uint8_t> &v, uint32_t flag, uint32_t l_seq, uint32_t extra) {
    const uint32_t l_name = 3, bs = BAM_FIXED + l_name + (l_seq + 1) / 2 + l_seq + extra;
    put32(v, bs);
    put32(v, 0xFFFFFFFFu);
    put32(v, 0xFFFFFFFFu);
    v.push_back((uint8_t)l_name);
    v.push_back(0);
    v.push_back(0x48);
    v.push_back(0x12);
    v.push_back(0);
    v.push_back(0);  // n_cigar
    v.push_back((uint8_t)flag);
    v.push_back((uint8_t)(flag >> 8));
    put32(v, l_seq);
    put32(v, 0xFFFFFFFFu);
    put32(v, 0xFFFFFFFFu);
    put32(v, 0);
    v.push_back('r');
    v.push_back('0');
    v.push_back(0);
    for (uint32_t i = 0; i < (l_seq + 1) / 2 + l_seq; i++) v.push_back((uint8_t)rnd(256));
    for (uint32_t i = 0; i < extra; i++) v.push_back(i % 7 == 0 ? (uint8_t)(32 + rnd(60)) : (uint8_t)(rnd(4) ? 0 : rnd(256)));
}

#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            fprintf(stderr, "line %d: %s\n", __LINE__, #c);          \
            exit(1);                                                 \
        }                                                            \
    } while (0)

// the chain from p through [.., hi) of the file, by the definition
static void naive(const std::vector<uint8_t> &f, uint64_t p, uint64_t hi, uint64_t *x, uint64_t *n) {
    *n = 0;
    while (p < hi) {
        if (p + 4 > f.size()) { *x = BAM_SUM_CUT; return; }
        const uint32_t bs = bam_le32(f.data() + p);
        if (bs < BAM_FIXED) { *x = BAM_SUM_DEAD; return; }
        if (p + 36 > f.size()) { *x = BAM_SUM_CUT; return; }
        *n += (bam_classify(f.data(), p).flag_cls >> 16) <= (uint32_t)BAM_C_SECOND ? 1u : 0u;
        p += 4ull + bs;
    }
    *x = p - hi;
}

int main() {
    const uint32_t flags[] = {0x41, 0x81, 0x51, 0x91, 0x141, 0x881, 0x0, 0xC1};
    uint64_t plans_ok = 0, plans = 0;
    for (int draw = 0; draw < 300; draw++) {
        std::vector<uint8_t> f;
        const uint64_t H = 12 + rnd(40);
        for (uint64_t i = 0; i < H; i++) f.push_back((uint8_t)rnd(256));  // (the header's bytes are never looked at)
        const uint32_t n_rec = 2 * (1 + rnd(12));
        for (uint32_t i = 0; i < n_rec; i++) {
            while (rnd(4) == 0) record(f, flags[4 + rnd(4)], rnd(40), rnd(50));
            record(f, flags[rnd(4)], rnd(100), rnd(3) ? 0 : rnd(300));
        }
        if (draw % 10 == 0) f.resize(f.size() - 1 - rnd(50));  // a file that ends inside a record, a fixed part or a size field
        const uint64_t T = f.size();
        const uint32_t world = 1 + rnd(6), seg = draw % 3 == 0 ? 64u : draw % 3 == 1 ? 100u : 4096u;
        const uint64_t chunk = draw % 4 == 0 ? 0u : 37u + rnd(300);
        std::vector<uint64_t> S(world + 1, 0);
        S[world] = T;
        for (uint32_t r = 1; r < world; r++) S[r] = S[r - 1] + rnd((uint32_t)((T - S[r - 1]) / (world - r + 1) * 2 + 1));
        std::vector<uint64_t> head(6 * world), xn, xn_off(world), plan(5 * world);
        for (uint32_t r = 0; r < world; r++) {
            const uint64_t lo = S[r], hi = S[r + 1], vis = hi + BAM_SUM_TAIL + rnd(20) < T ? hi + BAM_SUM_TAIL + rnd(20) : T;
            uint8_t *share = (uint8_t *)malloc(vis - lo ? vis - lo : 1);  // exactly the bytes the rank holds
            memcpy(share, f.data() + lo, vis - lo);
            const uint32_t n_lanes = r == 0 ? 1u : (uint32_t)(seg < hi - lo ? seg : hi - lo);
            std::vector<uint64_t> x(n_lanes), n(n_lanes);
            bam_share_summary_serial(share, vis - lo, hi - lo, r == 0 ? H : ~0ull, seg, chunk, n_lanes, x.data(), n.data());
            free(share);
            for (uint32_t c = 0; c < n_lanes; c++) {
                uint64_t wx = 0, wn = 0;
                naive(f, r == 0 ? H : lo + c, hi, &wx, &wn);
                if (r == 0 && H >= hi) { wx = H - hi; wn = 0; }
                CHECK(x[c] == wx);
                CHECK(wx >= BAM_SUM_CUT || n[c] == wn);
            }
            const uint64_t h[6] = {0, 1, 9, H, hi - lo, n_lanes};
            memcpy(&head[6 * r], h, sizeof h);
            xn_off[r] = xn.size();
            xn.insert(xn.end(), x.begin(), x.end());
            xn.insert(xn.end(), n.begin(), n.end());
        }
        xn.push_back(0);
        const int reason = bam_shard_plan(world, head.data(), xn.data(), xn_off.data(), plan.data());
        plans++;
        if (reason != BAM_PLAN_OK) continue;
        plans_ok++;
        // every entry is a start of the true chain, the first one at or behind the share's start
        uint64_t p = H, count = 0;
        uint32_t r = 1;
        while (p < T) {
            while (r < world && p >= S[r]) {
                CHECK(plan[5 * r] == p - S[r] && plan[5 * r + 2] == count && plan[5 * r + 3] == S[r]);
                CHECK(plan[5 * (r - 1) + 1] == p - S[r - 1] && plan[5 * (r - 1) + 4] == count);
                r++;
            }
            count += (bam_classify(f.data(), p).flag_cls >> 16) <= (uint32_t)BAM_C_SECOND ? 1u : 0u;
            p += 4ull + bam_le32(f.data() + p);
        }
        CHECK(p == T && r == world && (count & 1u) == 0 && plan[5 * (world - 1) + 4] == count && plan[5 * (world - 1) + 1] == ~0ull);
    }
    CHECK(plans_ok >= 20 && plans_ok < plans);
    printf("%llu plans, %llu without a fallback\nOK\n", (unsigned long long)plans, (unsigned long long)plans_ok);
    return 0;
}
