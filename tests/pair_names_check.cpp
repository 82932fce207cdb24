// The join by read name of vs_pair_names_core.h as plain C++ under AddressSanitizer and UBSan.
//  1. pn_join_host on windows held in heap buffers exactly as long as their text, line ends and tables -- so that a read
//     beyond a key, a line end or a slot is caught -- against a quadratic comparison of all keys; tables of 2 and 4 slots
//     (every probe wraps) and of the production size, all hash bits and only 2.
//  2. The window protocol (pn_decide) with the windows cut after every record, on random valid inputs with records deleted
//     from both files, against the same comparison on the whole files: pairs, their order, both single counts.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

#include "../vstrains_amd/csrc/vs_pair_names_core.h"

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

typedef std::vector<std::string> Heads;

static std::string fastq(const Heads &h, size_t from, size_t to) {
    std::string t;
    for (size_t k = from; k < to; k++) {
        const std::string seq(1u + (k * 7u) % 19u, "ACGT"[k & 3u]);
        t += h[k] + "\n" + seq + "\n+\n" + std::string(seq.size(), 'I') + "\n";
    }
    return t;
}

// a window on the heap: text and line ends in buffers of exactly their sizes
struct HeapWin {
    uint8_t *txt = nullptr;
    uint32_t *ends = nullptr;
    PnWin w;
    explicit HeapWin(const std::string &t) {
        txt = (uint8_t *)malloc(t.size() ? t.size() : 1u);
        if (!t.empty()) memcpy(txt, t.data(), t.size());
        std::vector<uint32_t> e;
        for (size_t i = 0; i < t.size(); i++)
            if (t[i] == '\n') e.push_back((uint32_t)i);
        ends = (uint32_t *)malloc(sizeof(uint32_t) * (e.size() ? e.size() : 1u));
        if (!e.empty()) memcpy(ends, e.data(), sizeof(uint32_t) * e.size());
        w = PnWin{txt, ends, (uint32_t)e.size(), (uint32_t)t.size(), (uint32_t)(e.size() / 4u)};
    }
    ~HeapWin() {
        free(txt);
        free(ends);
    }
    HeapWin(const HeapWin &) = delete;
    HeapWin &operator=(const HeapWin &) = delete;
};

struct Joined {
    std::vector<std::pair<uint32_t, uint32_t>> pairs;
    uint32_t res[5];
};

// pn_join_host with every array on the heap at its exact size; table 0: the production size
static Joined join(const PnWin &f0, const PnWin &f1, uint32_t table, uint32_t bits) {
    const uint32_t n_all = f0.n_rec + f1.n_rec, T = table ? table : pn_table_size(n_all), cap = f0.n_rec < f1.n_rec ? f0.n_rec : f1.n_rec;
    uint64_t *hash = (uint64_t *)malloc(sizeof(uint64_t) * (n_all ? n_all : 1u));
    uint32_t *klen = (uint32_t *)malloc(sizeof(uint32_t) * (n_all ? n_all : 1u)), *slot = (uint32_t *)malloc(sizeof(uint32_t) * (n_all ? n_all : 1u));
    uint32_t *claim = (uint32_t *)malloc(sizeof(uint32_t) * T), *mem0 = (uint32_t *)malloc(sizeof(uint32_t) * T), *mem1 = (uint32_t *)malloc(sizeof(uint32_t) * T);
    uint32_t *rec = (uint32_t *)malloc(sizeof(uint32_t) * (cap ? 2u * cap : 1u));
    const PnJoin J = {f0, f1, n_all, hash, klen, slot, T, claim, mem0, mem1};
    Joined out;
    pn_join_host(J, bits, rec, out.res);
    for (uint32_t p = 0; p < out.res[0] && p < cap; p++) out.pairs.push_back({rec[2u * p], rec[2u * p + 1u]});
    free(hash), free(klen), free(slot), free(claim), free(mem0), free(mem1), free(rec);
    return out;
}

static std::string key_of(const std::string &h, uint32_t file) { return h.substr(0, pn_key_len((const uint8_t *)h.data(), (uint32_t)h.size(), file)); }

// all keys against all keys; valid inputs only (no key twice in a file)
static std::vector<std::pair<uint32_t, uint32_t>> quadratic(const Heads &h0, const Heads &h1) {
    std::vector<std::pair<uint32_t, uint32_t>> out;
    for (uint32_t i = 0; i < h0.size(); i++)
        for (uint32_t j = 0; j < h1.size(); j++) {
            const std::string a = key_of(h0[i], 0), b = key_of(h1[j], 1);
            if (!a.empty() && a == b && il_mates((const uint8_t *)h0[i].data(), (uint32_t)h0[i].size(), (const uint8_t *)h1[j].data(), (uint32_t)h1[j].size()))
                out.push_back({i, j});
        }
    return out;
}

// a valid input: n names in one order, written three ways; records deleted from both files, lonely records added
static void random_input(uint32_t n, uint32_t drop_per_1000, Heads &h0, Heads &h1) {
    h0.clear(), h1.clear();
    for (uint32_t k = 0; k < n; k++) {
        const std::string name = "@r" + std::to_string(k * 7919u % 100003u) + std::string(k % 5u, 'x');
        const uint32_t kind = rnd() % 3u;
        const std::string a = kind == 0 ? name + "/1" : kind == 1 ? name + " 1:N:0" : name, b = kind == 0 ? name + "/2" : kind == 1 ? name + "\t2:N:0" : name;
        if (rnd() % 1000u >= drop_per_1000) h0.push_back(a);
        if (rnd() % 1000u >= drop_per_1000) h1.push_back(b);
        if (rnd() % 17u == 0) h0.push_back("@lonely1_" + std::to_string(k));
        if (rnd() % 19u == 0) h1.push_back("@lonely2_" + std::to_string(k) + "/2");
        if (rnd() % 23u == 0) h0.push_back(" empty token");
    }
}

// the window protocol, the windows growing by one record at a time: file f gets a record when pick says so
static int protocol(const Heads &h0, const Heads &h1, std::vector<std::pair<uint32_t, uint32_t>> &pairs, uint32_t singles[2]) {
    const Heads *h[2] = {&h0, &h1};
    size_t lo[2] = {0, 0}, hi[2] = {0, 0};  // the records of each window
    bool eof[2] = {h0.empty(), h1.empty()};
    singles[0] = singles[1] = 0;
    for (;;) {
        bool grew = false;
        for (int f = 0; f < 2; f++)
            if (!eof[f] && (eof[f ^ 1] || hi[f] - lo[f] <= hi[f ^ 1] - lo[f ^ 1] || rnd() % 3u == 0)) {
                hi[f]++;
                eof[f] = hi[f] == h[f]->size();
                grew = true;
            }
        CHECK(grew || (eof[0] && eof[1]));
        const HeapWin w0(fastq(h0, lo[0], hi[0])), w1(fastq(h1, lo[1], hi[1]));
        CHECK(w0.w.n_rec == hi[0] - lo[0] && w1.w.n_rec == hi[1] - lo[1]);
        const Joined jn = join(w0.w, w1.w, 0u, 64u);
        CHECK(jn.res[1] == PN_NONE && jn.res[2] == PN_NONE && jn.res[3] == PN_NONE && !jn.res[4]);
        uint32_t dec[2];
        const uint32_t P = jn.res[0];
        pn_decide(P, P ? jn.pairs.back().first : 0u, P ? jn.pairs.back().second : 0u, w0.w.n_rec, w1.w.n_rec, eof[0], eof[1], dec);
        for (const auto &p : jn.pairs) pairs.push_back({(uint32_t)lo[0] + p.first, (uint32_t)lo[1] + p.second});
        for (int f = 0; f < 2; f++) {
            CHECK(dec[f] >= P && dec[f] <= hi[f] - lo[f]);
            singles[f] += dec[f] - P;
            lo[f] += dec[f];
        }
        if (eof[0] && eof[1]) {
            CHECK(lo[0] == h0.size() && lo[1] == h1.size());
            return 0;
        }
    }
}

int main() {
    // 1. one pair of windows, every table
    for (uint32_t round = 0; round < 300; round++) {
        Heads h0, h1;
        random_input(round < 20 ? round % 3u : 1u + rnd() % 80u, round % 4u == 0 ? 0u : 100u, h0, h1);
        const HeapWin w0(fastq(h0, 0, h0.size())), w1(fastq(h1, 0, h1.size()));
        const auto want = quadratic(h0, h1);
        uint32_t keys = 0;
        for (const auto &s : h0) keys += !key_of(s, 0).empty();
        for (const auto &s : h1) keys += !key_of(s, 1).empty();
        for (uint32_t table : {0u, 2u, 4u, 64u, 256u})
            for (uint32_t bits : {64u, 2u}) {
                const Joined jn = join(w0.w, w1.w, table, bits);
                if (table && keys - (uint32_t)want.size() > table) {  // more distinct keys than slots: the probe ends in the status word
                    CHECK(jn.res[4] == 1u);
                    continue;
                }
                CHECK(!jn.res[4] && jn.res[1] == PN_NONE && jn.res[2] == PN_NONE && jn.res[3] == PN_NONE);
                CHECK(jn.pairs == want);
            }
    }
    // a key twice and three times: the smallest record involved, whichever table
    {
        const Heads h0 = {"@p", "@q/1", "@a", "@a/1", "@b", "@a"}, h1 = {"@p", "@b/2", "@b", "@zz"};
        const HeapWin w0(fastq(h0, 0, h0.size())), w1(fastq(h1, 0, h1.size()));
        for (uint32_t table : {0u, 8u, 16u}) {
            const Joined jn = join(w0.w, w1.w, table, table == 16u ? 2u : 64u);
            CHECK(jn.res[1] == 2u && jn.res[2] == 1u && !jn.res[4]);
        }
        // three records of file 1 name the one record of file 2: more matches than the pair list has room for
        const Heads m0 = {"@a", "@a/1", "@a x"}, m1 = {"@a"};
        const HeapWin u0(fastq(m0, 0, 3)), u1(fastq(m1, 0, 1));
        const Joined many = join(u0.w, u1.w, 0u, 64u);
        CHECK(many.res[1] == 0u && many.res[2] == PN_NONE);
        const Heads s0 = {"@a", "@b", "@c"}, s1 = {"@a", "@c", "@b"};
        const HeapWin v0(fastq(s0, 0, 3)), v1(fastq(s1, 0, 3));
        const Joined jn = join(v0.w, v1.w, 0u, 64u);
        CHECK(jn.res[0] == 3u && jn.res[3] == 2u && jn.res[1] == PN_NONE && jn.res[2] == PN_NONE);
    }
    // 2. the window protocol, cut after every record
    for (uint32_t round = 0; round < 120; round++) {
        Heads h0, h1;
        random_input(rnd() % 40u, round % 3u == 0 ? 30u : 200u, h0, h1);
        if (round % 10u == 1) h1.clear();
        if (round % 10u == 2) h0.clear();
        std::vector<std::pair<uint32_t, uint32_t>> got;
        uint32_t singles[2];
        if (protocol(h0, h1, got, singles)) return 1;
        const auto want = quadratic(h0, h1);
        CHECK(got == want);
        CHECK(singles[0] == h0.size() - want.size() && singles[1] == h1.size() - want.size());
    }
    printf("OK\n");
    return 0;
}
