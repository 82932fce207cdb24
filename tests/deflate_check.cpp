// The deflate encoder (vstrains_amd/csrc/vs_deflate_core.h) as plain C++ with one lane, for a host build under
// AddressSanitizer and UBSan (tests/test_bgzf_deflate_cpu.py builds and runs this program).  Every text and every member
// lies in a heap buffer of exactly its size, so a read behind the text or a store behind the member is found; every
// member is inflated again with the project's own decoder (inf_member, one lane) and compared with the text.  The
// code-length builder is driven alone on Fibonacci-like weights, which is what takes an unlimited Huffman tree past 15
// (and 7) bits.  Prints one line per case: "<name> n=<n> size=<size> kind=<kind>", then "OK".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../vstrains_amd/csrc/vs_deflate_core.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
static std::vector<uint8_t> random_bytes(size_t n) {
    std::vector<uint8_t> v(n);
    for (auto &b : v) b = (uint8_t)rnd();
    return v;
}

static int failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");        \
            failures++;                   \
        }                                 \
    } while (0)

static uint32_t crc32_plain(const uint8_t *p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    }
    return ~c;
}

static void run_case(const char *name, const std::vector<uint8_t> &text_v, int want_kind = -1) {
    const uint32_t n = (uint32_t)text_v.size();
    uint8_t *text = new uint8_t[n];  // exactly n bytes
    if (n) memcpy(text, text_v.data(), n);
    DefState *S = new DefState();
    uint32_t size = 0, kind = 9;
    std::vector<uint8_t> big(65536);
    uint32_t st = def_member(S, text, n, big.data(), (uint32_t)big.size(), 0, 1, &size, &kind);
    CHECK(st == DEF_OK, "%s: status %u", name, st);
    CHECK(size >= 28u && size <= n + 31u, "%s: size %u for n %u", name, size, n);
    // exactly sized, and one byte too small
    uint8_t *out = new uint8_t[size];
    uint32_t size2 = 0, kind2 = 9;
    memset(S, 0x5A, sizeof *S);  // (whatever the state held before must not matter)
    st = def_member(S, text, n, out, size, 0, 1, &size2, &kind2);
    CHECK(st == DEF_OK && size2 == size && kind2 == kind, "%s: second run differs (%u %u %u)", name, st, size2, kind2);
    CHECK(memcmp(out, big.data(), size) == 0, "%s: second run's bytes differ", name);
    if (size > 1u) {
        uint8_t *small = new uint8_t[size - 1u];
        memset(small, 0xA5, size - 1u);
        uint32_t s3 = 0, k3 = 0;
        st = def_member(S, text, n, small, size - 1u, 0, 1, &s3, &k3);
        CHECK(st == DEF_E_CAP, "%s: cap one short gives %u", name, st);
        for (uint32_t i = 0; i + 1u < size; i++)
            if (small[i] != 0xA5) {
                CHECK(false, "%s: cap one short wrote byte %u", name, i);
                break;
            }
        delete[] small;
    }
    // the member: header, BSIZE, trailer, and the payload through the project's decoder
    static const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0};
    CHECK(memcmp(out, head, 16) == 0, "%s: header", name);
    CHECK(((uint32_t)out[16] | ((uint32_t)out[17] << 8)) + 1u == size, "%s: BSIZE", name);
    const uint8_t *t = out + size - 8;
    const uint32_t crc = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
    const uint32_t isize = (uint32_t)t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
    CHECK(isize == n, "%s: ISIZE %u", name, isize);
    CHECK(crc == crc32_plain(text, n), "%s: CRC32", name);
    uint8_t *back = new uint8_t[n ? n : 1];
    InfState *I = new InfState();
    const uint32_t ist = inf_member(I, out + 18, size - 26u, back, n, 0, 1);
    CHECK(ist == INF_OK, "%s: inf_member status %u", name, ist);
    CHECK(n == 0 || memcmp(back, text, n) == 0, "%s: inflated text differs", name);
    if (want_kind >= 0) CHECK((int)kind == want_kind, "%s: kind %u, expected %d", name, kind, want_kind);
    printf("%s n=%u size=%u kind=%u\n", name, n, size, kind);
    delete I;
    delete[] back;
    delete[] out;
    delete S;
    delete[] text;
}

static std::vector<uint8_t> rep(const char *s, size_t times) {
    std::vector<uint8_t> v;
    const size_t l = strlen(s);
    for (size_t i = 0; i < times; i++) v.insert(v.end(), s, s + l);
    return v;
}

// lines "id:id:count\n" as the project writes them
static std::vector<uint8_t> info_like(size_t bytes) {
    std::string s;
    for (uint32_t i = 0; s.size() < bytes; i++)
        for (uint32_t j = 0; j < 60 && s.size() < bytes; j++) {
            const uint32_t v = (rnd() % 7u) ? 0u : rnd() % 300u;
            s += std::to_string(1000 + 7 * i) + ":" + std::to_string(1000 + 7 * j) + ":" + std::to_string(v) + "\n";
        }
    s.resize(bytes);
    return std::vector<uint8_t>(s.begin(), s.end());
}

static void check_lengths(const char *name, const std::vector<uint32_t> &freq, uint32_t maxbits) {
    const uint32_t nsym = (uint32_t)freq.size();
    std::vector<uint8_t> len(nsym, 0xEE);
    std::vector<uint32_t> work(288);
    std::vector<uint16_t> order(288);
    std::vector<uint32_t> cnt(DEF_CNT_WORDS);
    def_code_lengths(freq.data(), nsym, maxbits, len.data(), work.data(), order.data(), cnt.data());
    uint64_t kraft = 0;
    uint32_t used = 0;
    for (uint32_t s = 0; s < nsym; s++) {
        CHECK(len[s] <= maxbits, "%s: symbol %u has %u bits", name, s, len[s]);
        if (freq[s]) CHECK(len[s] > 0, "%s: symbol %u in use has no code", name, s);
        if (len[s] && len[s] <= maxbits) kraft += 1ull << (maxbits - len[s]), used++;
    }
    CHECK(used >= 2, "%s: %u symbols", name, used);
    CHECK(kraft == (1ull << maxbits), "%s: Kraft sum %llu / %llu", name, (unsigned long long)kraft, 1ull << maxbits);
    // a lighter symbol never has a shorter code than a heavier one
    for (uint32_t a = 0; a < nsym; a++)
        for (uint32_t b = 0; b < nsym; b++)
            if (freq[a] && freq[b] && freq[a] < freq[b]) CHECK(len[a] >= len[b], "%s: %u (%u) shorter than %u (%u)", name, a, freq[a], b, freq[b]);
    std::vector<uint16_t> code(nsym);
    def_codes(len.data(), nsym, code.data(), cnt.data());
    printf("%s symbols=%u kraft=1\n", name, used);
}

int main() {
    std::vector<uint8_t> fq;
    {
        std::string s;
        for (uint32_t i = 0; s.size() < 0xFF00u; i++) {
            s += "@read" + std::to_string(i) + "/1\n";
            for (int k = 0; k < 150; k++) s += "ACGT"[rnd() & 3u];
            s += "\n+\n";
            for (int k = 0; k < 150; k++) s += "FFFFFFF:,#"[rnd() % 10u];
            s += "\n";
        }
        s.resize(0xFF00u);
        fq.assign(s.begin(), s.end());
    }
    for (uint32_t n = 0; n <= 4; n++) run_case(("len_" + std::to_string(n)).c_str(), std::vector<uint8_t>(fq.begin(), fq.begin() + n));
    run_case("a_259", rep("A", 259));
    run_case("a_full", rep("A", 0xFF00));
    run_case("zeros_full", std::vector<uint8_t>(0xFF00, 0));
    run_case("ab_20000", rep("AB", 20000));
    {
        std::vector<uint8_t> v;
        for (int r = 0; r < 2; r++)
            for (int b = 0; b < 256; b++) v.push_back((uint8_t)b);
        run_case("all_bytes_twice", v);
    }
    run_case("random_full", random_bytes(0xFF00), DEF_KIND_STORED);
    for (uint32_t dist : {32768u, 32769u}) {
        for (int zero_fill = 0; zero_fill < 2; zero_fill++) {
            std::vector<uint8_t> v = random_bytes(300);
            std::vector<uint8_t> fill = zero_fill ? std::vector<uint8_t>(dist - 300u, 0) : random_bytes(dist - 300u);
            v.insert(v.end(), fill.begin(), fill.end());
            v.insert(v.end(), v.begin(), v.begin() + 300);
            run_case(("far_" + std::to_string(dist) + (zero_fill ? "_zeros" : "_random")).c_str(), v);
        }
    }
    {
        std::vector<uint8_t> v = info_like(4000);
        v.insert(v.end(), v.begin() + 100, v.begin() + 358);  // the last 258 bytes repeat earlier text
        run_case("flush_258", v);
        std::vector<uint8_t> u = random_bytes(200);
        u.insert(u.end(), u.begin() + 50, u.begin() + 53);  // the last 3
        run_case("flush_3", u);
    }
    run_case("fastq", fq);
    run_case("info_like", info_like(27722), DEF_KIND_DYNAMIC);
    run_case("info_like_full", info_like(0xFF00), DEF_KIND_DYNAMIC);
    {  // n > 0xFF00 is refused before anything is read
        DefState *S = new DefState();
        uint32_t size = 7, kind = 7;
        uint8_t dummy = 0;
        CHECK(def_member(S, &dummy, 0xFF01u, &dummy, 1, 0, 1, &size, &kind) == DEF_E_ARG, "n = 0xFF01 accepted");
        delete S;
    }

    // the code-length builder alone
    for (uint32_t maxbits : {15u, 7u}) {
        const uint32_t cap = maxbits == 15u ? 286u : 19u;
        for (uint32_t nsym : {2u, 3u, 8u, 19u, 30u, 40u, 286u}) {
            if (nsym > cap) continue;
            std::vector<uint32_t> fib(nsym);
            uint32_t a = 1, b = 1;
            for (uint32_t s = 0; s < nsym; s++) {  // 1 1 2 3 5 ..., held at 60000 (a member has at most 65281 tokens)
                fib[s] = a;
                const uint32_t c = a + b > 60000u ? 60000u : a + b;
                a = b, b = c;
            }
            check_lengths(("fib_" + std::to_string(maxbits) + "_" + std::to_string(nsym)).c_str(), fib, maxbits);
            std::vector<uint32_t> rev(fib.rbegin(), fib.rend());
            check_lengths(("fib_rev_" + std::to_string(maxbits) + "_" + std::to_string(nsym)).c_str(), rev, maxbits);
            std::vector<uint32_t> flat(nsym, 5u);
            check_lengths(("flat_" + std::to_string(maxbits) + "_" + std::to_string(nsym)).c_str(), flat, maxbits);
        }
        // no symbol, one symbol (first, second, last): two 1-bit codes, which every inflater takes
        for (int which = -1; which < 3; which++) {
            std::vector<uint32_t> f(cap, 0u);
            if (which >= 0) f[which == 2 ? cap - 1u : (uint32_t)which] = 9u;
            check_lengths(("single_" + std::to_string(maxbits) + "_" + std::to_string(which)).c_str(), f, maxbits);
            std::vector<uint8_t> len(cap);
            std::vector<uint32_t> work(288);
            std::vector<uint16_t> order(288);
    std::vector<uint32_t> cnt(DEF_CNT_WORDS);
            def_code_lengths(f.data(), cap, maxbits, len.data(), work.data(), order.data(), cnt.data());
            uint32_t ones = 0, others = 0;
            for (uint32_t s = 0; s < cap; s++) ones += len[s] == 1u, others += len[s] > 1u;
            CHECK(ones == 2u && others == 0u, "single %d: %u one-bit codes, %u longer", which, ones, others);
        }
    }
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("OK\n");
    return 0;
}
