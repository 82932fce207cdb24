// The hand-off between the mapping kernel and the counter kernels, written by the HOST: a block of per-end node lists
// (2 * n_pairs rows of LCAP words, lengths 0 .. LCAP, in the order given) into either layout k_pe_tiles leaves behind
// (vs_pe.hip, "The hand-off between the mapping kernel and the counter kernels"), and back.  Plain C++ and pure: a host
// compiler takes this header as it is (oracle/pack_check.cpp, tests/test_pe_pack_cpu.py); vs_pe_count_lists is its one
// caller in the library.  Nothing is clamped: what the mapping kernel would never hand over is refused.
#ifndef VS_PE_PACK_H
#define VS_PE_PACK_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "vs_pe_plan.h"

#define VS_PACK_LCAP 20u      // nodes an end may list (LCAP of vs_pe.hip)
#define VS_PACK_TAIL 16u      // padding words behind the lists (a run's 16-byte partner load may start at a list's last node)
#define VS_PACK_FILL 0xFFFFFFFFu  // what a word no list owns holds (the kernels must not care)

// words / counts the two layouts take for list_ends end slots (PePlan::list_words, list_ends)
inline uint64_t vs_pe_pack_words(uint64_t list_ends, bool rows) { return list_ends * (rows ? LC + 4u : LC) + VS_PACK_TAIL; }

// lists[2 * n_pairs][VS_PACK_LCAP], counts[2 * n_pairs] -> out_lists[vs_pe_pack_words(list_ends, rows)], out_counts[list_ends].
//   packed (rows = false): the ends of a tile (ept end slots) one after another in the tile's region of ept * LC words,
//       every list padded to whole quads; counts = n | quad offset inside the region << 8, 0 for an empty end
//   rows   (rows = true) : LC words per end, nodes 17 .. LCAP in the quad of a second array behind the rows; counts = n
// End slots past 2 * n_pairs (the unused ends of the last tile) get length 0.
// VS_E_RANGE (msg says which): a length above LCAP, a node >= n_nodes, a node twice in one list, a tile whose lists need
// more than ept * LC / 4 quads (the mapping kernel sends such pairs to the overflow kernels), list_ends that do not hold
// the block or are no whole number of tiles.
inline int vs_pe_pack_lists(uint32_t n_nodes, uint64_t n_pairs, const uint32_t *lists, const uint32_t *counts, uint32_t ept, uint64_t list_ends,
                            bool rows, uint32_t *out_lists, uint32_t *out_counts, char *msg, size_t msg_len) {
    const uint64_t n_ends = 2u * n_pairs;
    if (ept < 2u || (ept & 1u) || list_ends % ept || list_ends < n_ends) {
        snprintf(msg, msg_len, "%llu end slots in tiles of %u do not hold %llu ends", (unsigned long long)list_ends, ept, (unsigned long long)n_ends);
        return VS_E_RANGE;
    }
    const uint64_t words = vs_pe_pack_words(list_ends, rows);
    for (uint64_t i = 0; i < words; i++) out_lists[i] = VS_PACK_FILL;
    for (uint64_t i = 0; i < list_ends; i++) out_counts[i] = 0u;
    const uint32_t region_q = ept * LC / 4u;
    uint32_t *hi = out_lists + list_ends * LC;
    uint32_t used_q = 0;
    for (uint64_t e = 0; e < n_ends; e++) {
        const uint32_t n = counts[e], *row = lists + e * VS_PACK_LCAP;
        if (e % ept == 0) used_q = 0;
        if (n > VS_PACK_LCAP) {
            snprintf(msg, msg_len, "end %llu lists %u nodes (at most %u)", (unsigned long long)e, n, VS_PACK_LCAP);
            return VS_E_RANGE;
        }
        for (uint32_t i = 0; i < n; i++) {
            if (row[i] >= n_nodes) {
                snprintf(msg, msg_len, "end %llu lists node %u of %u", (unsigned long long)e, row[i], n_nodes);
                return VS_E_RANGE;
            }
            for (uint32_t j = 0; j < i; j++)
                if (row[j] == row[i]) {
                    snprintf(msg, msg_len, "end %llu lists node %u twice", (unsigned long long)e, row[i]);
                    return VS_E_RANGE;
                }
        }
        const uint32_t q = (n + 3u) / 4u;
        if (used_q + q > region_q) {
            snprintf(msg, msg_len, "the lists of tile %llu need more than %u quads", (unsigned long long)(e / ept), region_q);
            return VS_E_RANGE;
        }
        if (!rows) {
            uint32_t *dst = out_lists + (e / ept) * ept * LC + 4u * used_q;
            for (uint32_t i = 0; i < n; i++) dst[i] = row[i];
            out_counts[e] = n ? n | used_q << 8 : 0u;
        } else {
            for (uint32_t i = 0; i < n; i++) (i < LC ? out_lists[e * LC + i] : hi[e * 4u + (i - LC)]) = row[i];
            out_counts[e] = n;
        }
        used_q += q;
    }
    return VS_OK;
}

// The way back: the first n_ends end slots of a layout as rows of VS_PACK_LCAP words (unused words VS_PACK_FILL) and lengths.
inline void vs_pe_unpack_lists(uint64_t n_ends, const uint32_t *in_lists, const uint32_t *in_counts, uint32_t ept, uint64_t list_ends, bool rows,
                               uint32_t *lists, uint32_t *counts) {
    const uint32_t *hi = in_lists + list_ends * LC;
    for (uint64_t e = 0; e < n_ends; e++) {
        const uint32_t c = in_counts[e], n = rows ? c : c & 0xFFu;
        const uint32_t *src = in_lists + (e / ept) * ept * LC + 4u * (c >> 8);
        counts[e] = n;
        for (uint32_t i = 0; i < VS_PACK_LCAP; i++)
            lists[e * VS_PACK_LCAP + i] = i >= n ? VS_PACK_FILL : !rows ? src[i] : i < LC ? in_lists[e * LC + i] : hi[e * 4u + (i - LC)];
    }
}

#endif  // VS_PE_PACK_H
