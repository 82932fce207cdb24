// The plan of one block of the site-pair pass (vs_node_site_pairs): the launch of k_node_site_pairs (vs_pe.hip) as ONE pure
// function of scalars, shaped like vs_pileup_plan.h, and the rows of the cell table (vs_site_pairs_rows_host).  Plain C++: a
// host compiler takes this header as it is.
//
// What the pass computes (tests/site_pairs_model.py states it).  A SITE is a position of a segment of K = k + 1 bases or more,
// given as its pileup slot (vs_pileup_layout).  A FRAGMENT is the two ends 2p, 2p + 1 of a block.  Every alignment the pileup
// credits makes one raw observation (site, column) per site under its overlap; a fragment with more than 32 of them is
// overflow and deposits nothing; a site the fragment saw with two different columns is discordant and left out; every pair
// s < t of the sites that remain adds 1 to cells[row_first[s] + (t - s - 1)][column at s][column at t] when t lies on s's
// segment at most `span` positions behind s, and is tallied as unstored otherwise.
//
// Launch.  A wavefront works through batches of 64 ends, which are 32 WHOLE fragments only if every workgroup's share and
// every batch starts at an even end: ends_per_wg is a multiple of 64 (vs_pileup_plan_for rounds to the quotient, which may
// be odd), and a block of an odd number of ends is refused.  Beside the 324 words of the pileup's wavefront each wavefront
// holds 32 lists of a counter and 32 entries, 1 056 words: workgroups of 512 threads take 44 KB of LDS, three to a CU.
#ifndef VS_SITE_PAIRS_PLAN_H
#define VS_SITE_PAIRS_PLAN_H
#include <stdint.h>
#include <stdio.h>

#include "../../include/vstrains_hip.h"
#include "vs_pileup_plan.h"
#include "vs_site_pairs_core.h"

#define SITE_PAIRS_TPB 512u  // threads of a k_node_site_pairs workgroup: eight wavefronts
#define SITE_PAIRS_WAVES (SITE_PAIRS_TPB / 64u)
#define SITE_PAIRS_FRAGS 32u                          // fragments of a batch of 64 ends
#define SITE_PAIRS_LIST_WORDS (SITE_PAIRS_CAP + 1u)   // a list: its counter and its entries (33: lane f's list starts in bank f)
#define SITE_PAIRS_WAVE_WORDS (PILEUP_WAVE_WORDS + SITE_PAIRS_FRAGS * SITE_PAIRS_LIST_WORDS)
#define SITE_PAIRS_LDS_WORDS (PILEUP_HEAD_WORDS + SITE_PAIRS_WAVES * SITE_PAIRS_WAVE_WORDS)
#define SITE_PAIRS_WG_PER_CU 3u
#define SITE_PAIRS_MIN_ENDS (64u * SITE_PAIRS_WAVES)  // a workgroup's share is at least one batch per wavefront
#define SITE_PAIRS_TALLIES 5u  // fragments that observed, overflow fragments, discordant (fragment, site), pairs stored, pairs unstored

struct SitePairsPlan {
    int status;  // VS_OK, VS_E_ARG or VS_E_RANGE with msg
    char msg[128];
    uint32_t launch;       // 0: nothing is launched (no ends, or no end holds K bases)
    uint32_t grid;         // workgroups
    uint64_t ends_per_wg;  // workgroup g takes ends [g * ends_per_wg, (g + 1) * ends_per_wg): a multiple of 64
};

inline SitePairsPlan vs_site_pairs_plan_for(uint32_t n_nodes, uint32_t K, uint64_t n_ends, uint32_t max_len, uint32_t n_cu) {
    SitePairsPlan p = {};
    if (n_ends & 1u) {
        p.status = VS_E_ARG;
        snprintf(p.msg, sizeof p.msg, "a block of %llu ends: fragments are the ends 2p and 2p + 1", (unsigned long long)n_ends);
        return p;
    }
    if (n_nodes > 0x01FFFFFEu) {
        p.status = VS_E_RANGE;
        snprintf(p.msg, sizeof p.msg, "more than 2^25-2 nodes");
        return p;
    }
    if (n_ends > 0xFFFFFFF0ull) {
        p.status = VS_E_RANGE;
        snprintf(p.msg, sizeof p.msg, "a block of 2^32 ends or more");
        return p;
    }
    if (!n_ends || !n_nodes || !K || max_len < K) return p;  // no end holds an anchor
    const uint64_t slots = (uint64_t)(n_cu ? n_cu : 1u) * SITE_PAIRS_WG_PER_CU;
    uint64_t per = (n_ends + slots - 1u) / slots;
    per = (per + 63u) & ~63ull;  // no workgroup and no batch boundary cuts a pair
    if (per < SITE_PAIRS_MIN_ENDS) per = SITE_PAIRS_MIN_ENDS;
    if (per > PILEUP_MAX_ENDS) per = PILEUP_MAX_ENDS;
    p.ends_per_wg = per;
    p.grid = (uint32_t)((n_ends + per - 1u) / per);
    p.launch = 1u;
    return p;
}

// (seg[i], pos[i]): the sites, strictly ascending by segment, then position.  row_first[i] = the cells before site i's,
// row_first[n_sites] = *n_cells = all of them; site i's partners are the sites j > i with seg[j] == seg[i] and
// pos[j] - pos[i] <= span.  A two-pointer pass.  VS_E_ARG: not ascending; VS_E_RANGE: 2^29 sites or more, 2^32 cells or more
// (*n_cells is set; row_first is then not to be used).
inline int vs_site_pairs_rows_for(const uint32_t *seg, const uint32_t *pos, uint64_t n_sites, uint32_t span, uint32_t *row_first, uint64_t *n_cells) {
    *n_cells = 0u;
    if (n_sites >= SITE_PAIRS_MAX_SITES) return VS_E_RANGE;
    uint64_t total = 0u, j = 0u;
    for (uint64_t i = 0u; i < n_sites; i++) {
        if (i && (seg[i] < seg[i - 1u] || (seg[i] == seg[i - 1u] && pos[i] <= pos[i - 1u]))) return VS_E_ARG;
        if (j < i + 1u) j = i + 1u;
        while (j < n_sites && seg[j] == seg[i] && (uint64_t)pos[j] - pos[i] <= span) j++;  // (checked ascending when i gets there)
        row_first[i] = (uint32_t)total;
        total += j - (i + 1u);
        if (total >= (1ull << 32)) {
            *n_cells = total;
            return VS_E_RANGE;
        }
    }
    row_first[n_sites] = (uint32_t)total;
    *n_cells = total;
    return VS_OK;
}

#endif  // VS_SITE_PAIRS_PLAN_H
