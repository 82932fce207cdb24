// What one lane of k_node_site_pairs (vs_pe.hip) does beyond the pileup's walk (vs_pileup_core.h), as __host__ __device__
// functions, so that the code the kernel runs is held to tests/site_pairs_model.py on a CPU (vs_site_pairs_frag_host,
// tests/test_site_pairs_host_cpu.py).  Plain C++: a host compiler takes this header as it is.
//
//   range  : the sites are an ascending array of pileup slots (first[n] + position, vs_pileup_layout), so the sites under one
//            alignment's overlap -- forward slots lo .. hi -- are ONE contiguous range of it: two binary searches.
//   column : the read's byte at a site as it reads on the forward strand: the pileup's column rule for alt, taken at
//            agreeing positions too.
//   entry  : one raw observation, site << 3 | column: an order on entries is the order by site, then by column.
//   reduce : what ONE fragment saw, from its raw list to its observations, in place (no array of its own: the list lies in
//            LDS on the device): sorted, then every site whose entries all carry one column is kept once, a site with two
//            different columns is left out and counted as discordant.  A property of the SET of entries: the order in which
//            lanes appended them does not matter.
//   cell   : site i's partners are the later sites of its segment within the span, contiguous behind it: the cell of (s, t)
//            is row_first[s] + (t - s - 1), and t is a partner exactly when that stays below row_first[s + 1].
#ifndef VS_SITE_PAIRS_CORE_H
#define VS_SITE_PAIRS_CORE_H
#include <stdint.h>

#include "vs_pileup_core.h"

#define SITE_PAIRS_CAP 32u    // raw observations a fragment may hold: one more and it is overflow
#define SITE_PAIRS_COLS 5u    // A C G T and `other`
#define SITE_PAIRS_CELL 25u   // counts of one pair of sites: [column at s][column at t]
#define SITE_PAIRS_MAX_SITES (1u << 29)  // an entry is site << 3 | column

// the first index i of the ascending a[0 .. n) with a[i] >= v (n: none)
VS_PL_HD uint32_t vs_sp_lower(const uint32_t *a, uint32_t n, uint32_t v) {
    uint32_t lo = 0u, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < v) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// the sites whose slot lies in lo .. hi (both included, lo <= hi): [*i0, *i1)
VS_PL_HD void vs_site_pairs_range(const uint32_t *site_slot, uint32_t n_sites, uint32_t lo, uint32_t hi, uint32_t *i0, uint32_t *i1) {
    const uint32_t a = vs_sp_lower(site_slot, n_sites, lo);
    *i0 = a;
    *i1 = a + vs_sp_lower(site_slot + a, n_sites - a, hi + 1u);  // (hi + 1 does not wrap: a slot total stays below 2^32)
}

// the column of read offset x: the read's base as it reads on the forward strand (opp: the alignment lies on the reverse
// complement), 4 for a byte outside ACGT
VS_PL_HD uint32_t vs_site_pairs_col(const uint32_t *rw, uint64_t rbase, const uint32_t *mk, uint32_t x, uint32_t opp) {
    const uint64_t at = rbase + x;
    if (mk && ((mk[at >> 4] >> ((uint32_t)(at & 15u) * 2u)) & 3u)) return 4u;
    const uint32_t code = (rw[at >> 4] >> ((uint32_t)(at & 15u) * 2u)) & 3u;
    return opp ? 3u - code : code;
}

// e[0 .. n), n <= SITE_PAIRS_CAP, raw entries in any order -> the observations in e[0 .. return), ascending; *discordant =
// the sites left out
VS_PL_HD uint32_t vs_site_pairs_reduce(uint32_t *e, uint32_t n, uint32_t *discordant) {
    for (uint32_t i = 1u; i < n; i++) {  // (insertion sort in place: lists are short, and mostly a few entries)
        const uint32_t v = e[i];
        uint32_t j = i;
        for (; j > 0u && e[j - 1u] > v; j--) e[j] = e[j - 1u];
        e[j] = v;
    }
    uint32_t m = 0u, bad = 0u;
    for (uint32_t i = 0u; i < n;) {
        const uint32_t v = e[i], site = v >> 3;
        uint32_t j = i + 1u, last = v;
        for (; j < n && (e[j] >> 3) == site; j++) last = e[j];
        if (last == v) e[m++] = v; else bad++;  // (sorted: the run's first and last entry are equal iff all are)
        i = j;
    }
    *discordant = bad;
    return m;
}

// sites s < t (indices): 1 and *cell = the pair's cell if t is one of s's partners, else 0 (unstored)
VS_PL_HD uint32_t vs_site_pairs_cell(const uint32_t *row_first, uint32_t s, uint32_t t, uint32_t *cell) {
    const uint32_t at = row_first[s] + (t - s - 1u);
    *cell = at;
    return t - s - 1u < row_first[s + 1u] - row_first[s] ? 1u : 0u;
}

#endif  // VS_SITE_PAIRS_CORE_H
