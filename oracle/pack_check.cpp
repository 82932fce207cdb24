// CPU access to the host packing of a block of per-end node lists into the hand-off layouts of a PE count
// (vstrains_amd/csrc/vs_pe_pack.h, product source, compiled unchanged): arrays in, arrays out.  No device, no HIP call.
// tests/test_pe_pack_cpu.py drives it; with -DVS_PACK_CHECK_MAIN the file is a program of its own that packs and unpacks
// random blocks and tries every refusal (for a run under the host compiler's sanitizers).
#include "../vstrains_amd/csrc/vs_pe_pack.h"

extern "C" uint64_t vs_pack_check_words(uint64_t list_ends, int rows) { return vs_pe_pack_words(list_ends, rows != 0); }

// -> the status of vs_pe_pack_lists; msg[128]
extern "C" int vs_pack_check(uint32_t n_nodes, uint64_t n_pairs, const uint32_t *lists, const uint32_t *counts, uint32_t ept, uint64_t list_ends,
                             int rows, uint32_t *out_lists, uint32_t *out_counts, char *msg) {
    msg[0] = 0;
    return vs_pe_pack_lists(n_nodes, n_pairs, lists, counts, ept, list_ends, rows != 0, out_lists, out_counts, msg, 128);
}

extern "C" void vs_unpack_check(uint64_t n_ends, const uint32_t *in_lists, const uint32_t *in_counts, uint32_t ept, uint64_t list_ends, int rows,
                                uint32_t *lists, uint32_t *counts) {
    vs_pe_unpack_lists(n_ends, in_lists, in_counts, ept, list_ends, rows != 0, lists, counts);
}

#ifdef VS_PACK_CHECK_MAIN
#include <vector>

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((rng_state >> 33) % n);
}

int main() {
    int bad = 0;
    char msg[128];
    for (uint32_t ept : {2u, 6u, 32u, 64u, 128u})
        for (uint32_t round = 0; round < 40; round++) {
            const uint32_t n_nodes = 1u + rnd(300), max_n = n_nodes < VS_PACK_LCAP ? n_nodes : VS_PACK_LCAP;
            // a block whose tiles are closed early with empty pairs, as the Python face closes them
            std::vector<uint32_t> lists, counts;
            uint32_t used_p = 0, used_q = 0;
            const uint32_t n_real = rnd(200);
            for (uint32_t p = 0; p < n_real; p++) {
                uint32_t n[2] = {rnd(max_n + 1u), rnd(max_n + 1u)};
                if (ept == 2u) { n[0] = n[0] > 16u ? 16u : n[0]; n[1] = n[1] > 16u ? 16u : n[1]; }
                const uint32_t q = (n[0] + 3u) / 4u + (n[1] + 3u) / 4u;
                if (used_p == ept / 2u || used_q + q > ept * LC / 4u) {
                    for (; used_p < ept / 2u; used_p++) { counts.insert(counts.end(), 2u, 0u); lists.insert(lists.end(), 2u * VS_PACK_LCAP, VS_PACK_FILL); }
                    used_p = used_q = 0;
                }
                for (int side = 0; side < 2; side++) {
                    std::vector<uint32_t> row(VS_PACK_LCAP, VS_PACK_FILL);
                    for (uint32_t i = 0; i < n[side];) {
                        const uint32_t x = rnd(n_nodes);
                        bool dup = false;
                        for (uint32_t j = 0; j < i; j++) dup |= row[j] == x;
                        if (!dup) row[i++] = x;
                    }
                    lists.insert(lists.end(), row.begin(), row.end());
                    counts.push_back(n[side]);
                }
                used_p++;
                used_q += q;
            }
            const uint64_t n_pairs = counts.size() / 2u, n_tiles = (n_pairs + ept / 2u - 1u) / (ept / 2u), list_ends = n_tiles * ept;
            for (int rows = 0; rows < 2; rows++) {
                std::vector<uint32_t> out(vs_pe_pack_words(list_ends, rows)), oc(list_ends + 1u), back(lists.size() + 1u), bc(counts.size() + 1u);
                const int rc = vs_pe_pack_lists(n_nodes, n_pairs, lists.data(), counts.data(), ept, list_ends, rows, out.data(), oc.data(), msg, sizeof msg);
                if (rc != VS_OK) { printf("ept %u round %u rows %d: refused: %s\n", ept, round, rows, msg); bad++; continue; }
                vs_pe_unpack_lists(counts.size(), out.data(), oc.data(), ept, list_ends, rows, back.data(), bc.data());
                for (size_t i = 0; i < counts.size(); i++) bad += bc[i] != counts[i];
                for (size_t i = 0; i < lists.size(); i++) bad += back[i] != lists[i];
                for (uint32_t i = 0; i < VS_PACK_TAIL; i++) bad += out[out.size() - 1u - i] != VS_PACK_FILL;
            }
            if (!n_pairs) continue;
            // the refusals: a length above LCAP, a node >= n_nodes, a node twice, a tile that is too full, too few end slots
            std::vector<uint32_t> out(vs_pe_pack_words(list_ends + ept, true)), oc(list_ends + ept);
            for (int what = 0; what < 5; what++)
                for (int rows = 0; rows < 2; rows++) {
                    std::vector<uint32_t> l2 = lists, c2 = counts;
                    uint64_t ends = list_ends;
                    const uint64_t e = rnd((uint32_t)c2.size());
                    if (what == 0) c2[e] = VS_PACK_LCAP + 1u + rnd(300);
                    if (what == 1) { c2[e] = 1; l2[e * VS_PACK_LCAP] = n_nodes + rnd(3) * 0x3FFFFFFFu; }
                    if (what == 2) { if (n_nodes < 2u) continue; c2[e] = 3; l2[e * VS_PACK_LCAP] = 0; l2[e * VS_PACK_LCAP + 1] = 1; l2[e * VS_PACK_LCAP + 2] = 0; }
                    if (what == 3) {  // every end of one tile as long as the graph allows: 5 quads per end against 4 on average
                        if (n_nodes < 17u) continue;
                        const uint64_t t0 = e / ept * ept;
                        for (uint64_t k = t0; k < t0 + ept && k < c2.size(); k++) { c2[k] = 17; for (uint32_t i = 0; i < 17u; i++) l2[k * VS_PACK_LCAP + i] = i; }
                        if (c2.size() - t0 < ept) continue;
                    }
                    if (what == 4) ends = list_ends - ept;
                    const int rc = vs_pe_pack_lists(n_nodes, n_pairs, l2.data(), c2.data(), ept, ends, rows, out.data(), oc.data(), msg, sizeof msg);
                    if (rc != VS_E_RANGE) { printf("ept %u round %u rows %d refusal %d: status %d\n", ept, round, rows, what, rc); bad++; }
                }
        }
    printf("pack_check: %d problems\n", bad);
    return bad ? 1 : 0;
}
#endif
