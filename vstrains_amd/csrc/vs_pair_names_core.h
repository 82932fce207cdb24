// Which records of TWO FASTQ windows -- one of each file of a pair -- are mates (vs_pair_names.hip): the key of a record, the
// hash that nominates, the open-address table of the join, what a round of the window protocol decides.  One statement for the
// kernels and for the one-thread host twin (pn_join_host), as vs_mates_core.h is for the interleaved ingest.
//
// Token and mates: il_token_len and il_mates(a, b) of vs_mates_core.h, unchanged; a = the header line of the file-1 record,
// b = that of the file-2 record.
// Key: the token, without a trailing "/1" on a file-1 record and without a trailing "/2" on a file-2 record.  The key only
// nominates: two records are a PAIR iff they are of different files, their keys are non-empty and equal byte for byte, and
// il_mates says so ("x/1" against "x": equal keys, no mates -- two singles).
// Hash: FNV-1a over the key bytes, then the finaliser of MurmurHash3 (as bam_name_hash); `bits` keeps the low bits only.
//
// The join of two windows (R0 + R1 records, g = r for file 1's, R0 + r for file 2's): a table of T slots, a power of two;
// a slot holds a claim word (the record that owns it: its key is the slot's) and one member word per file.  A record with a
// non-empty key probes linearly from its hash: it claims an empty slot by compare-and-swap or finds its key there (hash
// first, then the bytes), then enters itself as its file's member, again by compare-and-swap.  A taken member word means that
// the key occurs twice in that file's window (V1): min(own record, occupant) goes into a minimum, so the record reported is
// the smallest one involved whichever lane came first.  A file-1 record's partner is member[1] of its slot, if il_mates says
// so.  The matched file-1 records in order are the pairs; their file-2 records must rise (V2).
//
// WHOLE-FILE MEANING.  An input is valid when (V1) within one file no non-empty key occurs twice and (V2) the file-1 records
// that have a mate, in file order, have their mates in increasing file-2 order.  For a valid input the pairs are exactly the
// records whose key is in both files (and il_mates), in file-1 order; every other complete record is a single of its file.
//
// WHAT A ROUND DECIDES (pn_decide).  Both windows start at a record boundary; all their complete records are joined.  With P
// pairs, the last one (i*, j*): every record up to i* (file 1) and j* (file 2) is decided -- the unmatched ones among them
// are singles; records behind the last match wait.  When a file is at its end (its whole window took part in the join), every
// complete record of the OTHER file's window is decided.  Singles of a file = decided - P.
//
// CUT INDEPENDENCE.  Let (a_i, b_j) be a pair of a valid input.  a_i is decided as a single only by a later match
// (a_i', b_j'), i' > i; by V2, j' > j.  So b_j was in the window -- and the exhaustive join would have matched it -- or it was
// consumed by an earlier cut.  An earlier cut falls behind a match (a_i'', b_j'') with j'' > j, hence (V2) i'' > i: a_i was in
// that window, and so was b_j, and they would have matched then.  (The same with the files exchanged; a file's end decides
// records of the other only when none of its own are still to come.)  So for valid inputs the pairs, their order and both
// single counts do not depend on where the windows are cut.
#pragma once
#include <stdint.h>

#include "vs_mates_core.h"

#define PN_NONE 0xFFFFFFFFu

// the bytes of the key of the header line q[0, n) of a record of file `file` (0: file 1, 1: file 2)
IL_HD uint32_t pn_key_len(const uint8_t *q, uint32_t n, uint32_t file) {
    const uint32_t l = il_token_len(q, n);
    if (l >= 2u && q[l - 2u] == '/' && q[l - 1u] == (file ? '2' : '1')) return l - 2u;
    return l;
}

IL_HD uint64_t pn_hash(const uint8_t *q, uint32_t l, uint32_t bits) {
    uint64_t h = 0xCBF29CE484222325ull;  // FNV-1a, then the finaliser of MurmurHash3 so that the low bits depend on every byte
    for (uint32_t i = 0; i < l; i++) h = (h ^ q[i]) * 0x100000001B3ull;
    h ^= h >> 33;
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    h *= 0xC4CEB9FE1A85EC53ull;
    h ^= h >> 33;
    return bits >= 64u ? h : bits == 0u ? 0ull : h & ((1ull << bits) - 1ull);
}

// One window: its text (size bytes), the byte offsets of its n_nl line ends, n_rec complete records.
struct PnWin {
    const uint8_t *txt;
    const uint32_t *ends;
    uint32_t n_nl, size, n_rec;
};

// the header line of record r of w: false (and an empty line) where the line ends do not describe one inside the window
IL_HD bool pn_header(const PnWin &w, uint32_t r, uint32_t *at, uint32_t *n) {
    *at = *n = 0u;
    if (r >= w.n_rec || 4ull * r >= w.n_nl) return false;
    const uint32_t a0 = r ? w.ends[4u * r - 1u] + 1u : 0u, a1 = w.ends[4u * r];
    if (a0 > a1 || a1 > w.size) return false;
    *at = a0;
    *n = a1 - a0;
    return true;
}

// m = il_mates(record i of f0, record j of f1)
IL_HD bool pn_mates_at(const PnWin &f0, uint32_t i, const PnWin &f1, uint32_t j) {
    uint32_t a, na, b, nb;
    if (!pn_header(f0, i, &a, &na) || !pn_header(f1, j, &b, &nb)) return false;
    return il_mates(f0.txt + a, na, f1.txt + b, nb);
}

// The join's arrays.  hash, klen, slot: one entry per record g in [0, n_all), n_all = f0.n_rec + f1.n_rec.  claim, mem0, mem1:
// T entries each, PN_NONE before the join.
struct PnJoin {
    PnWin f0, f1;
    uint32_t n_all;
    uint64_t *hash;
    uint32_t *klen, *slot;
    uint32_t T;  // a power of two
    uint32_t *claim, *mem0, *mem1;
};

IL_HD const PnWin &pn_win_of(const PnJoin &J, uint32_t g, uint32_t *r) {
    const bool second = g >= J.f0.n_rec;
    *r = second ? g - J.f0.n_rec : g;
    return second ? J.f1 : J.f0;
}

// key bounds and hash of record g (g < n_all)
IL_HD void pn_hash_at(const PnJoin &J, uint32_t g, uint32_t bits) {
    uint32_t r, at, n;
    const PnWin &w = pn_win_of(J, g, &r);
    uint32_t l = 0u;
    if (pn_header(w, r, &at, &n)) l = pn_key_len(w.txt + at, n, g >= J.f0.n_rec ? 1u : 0u);
    J.klen[g] = l;
    J.hash[g] = l ? pn_hash(w.txt + at, l, bits) : 0ull;
}

// the keys of records g and o: equal?  (hash first, then the bytes; both have non-empty keys)
IL_HD bool pn_key_eq(const PnJoin &J, uint32_t g, uint32_t o) {
    if (J.hash[g] != J.hash[o] || J.klen[g] != J.klen[o]) return false;
    uint32_t rg, ro, ag, ao, n;
    const PnWin &wg = pn_win_of(J, g, &rg), &wo = pn_win_of(J, o, &ro);
    if (!pn_header(wg, rg, &ag, &n) || !pn_header(wo, ro, &ao, &n)) return false;
    const uint8_t *a = wg.txt + ag, *b = wo.txt + ao;
    for (uint32_t k = 0; k < J.klen[g]; k++)
        if (a[k] != b[k]) return false;
    return true;
}

// 32-bit compare-and-swap and minimum: atomics on the device, plain on the one host thread
IL_HD uint32_t pn_cas(uint32_t *p, uint32_t expect, uint32_t v) {
#ifdef __HIP_DEVICE_COMPILE__
    return atomicCAS(p, expect, v);
#else
    const uint32_t old = *p;
    if (old == expect) *p = v;
    return old;
#endif
}
IL_HD void pn_min(uint32_t *p, uint32_t v) {
#ifdef __HIP_DEVICE_COMPILE__
    atomicMin(p, v);
#else
    if (v < *p) *p = v;
#endif
}

// Record g (g < n_all) enters the table.  dup[f]: the smallest record of file f whose key occurs twice (a minimum, PN_NONE
// before); *full: set when the probe went round the whole table.  No lane waits for another; the loop is bounded by T.
IL_HD void pn_claim_at(const PnJoin &J, uint32_t g, uint32_t *dup, uint32_t *full) {
    J.slot[g] = PN_NONE;
    if (!J.klen[g]) return;  // (an empty key is never a mate)
    const uint32_t file = g >= J.f0.n_rec ? 1u : 0u, r = file ? g - J.f0.n_rec : g, mask = J.T - 1u;
    uint32_t s = (uint32_t)J.hash[g] & mask;
    for (uint32_t probe = 0; probe < J.T; probe++, s = (s + 1u) & mask) {
        const uint32_t cur = pn_cas(&J.claim[s], PN_NONE, g);  // (what the swap returns is the re-read)
        const uint32_t owner = cur == PN_NONE ? g : cur;
        if (owner != g && (owner >= J.n_all || !pn_key_eq(J, g, owner))) continue;
        uint32_t *mem = file ? J.mem1 : J.mem0;
        const uint32_t prev = pn_cas(&mem[s], PN_NONE, r);
        if (prev != PN_NONE) pn_min(&dup[file], prev < r ? prev : r);
        J.slot[g] = s;
        return;
    }
    *full = 1u;
}

// the file-2 record that is the mate of file-1 record i (i < f0.n_rec), PN_NONE: none in the window
IL_HD uint32_t pn_partner_at(const PnJoin &J, uint32_t i) {
    const uint32_t s = J.slot[i];
    if (s >= J.T) return PN_NONE;
    const uint32_t j = J.mem1[s];
    if (j >= J.f1.n_rec) return PN_NONE;
    return pn_mates_at(J.f0, i, J.f1, j) ? j : PN_NONE;
}

// the smallest table the stream takes for n_all records: a power of two, at most half full, at least 2
IL_HD uint32_t pn_table_size(uint32_t n_all) {
    uint32_t t = 2u;
    while (t < 2u * n_all && t < 0x80000000u) t <<= 1;
    return t;
}

// What a round decides: records decided per file from the pairs (n_pairs of them, the last one (li, lj)), the complete
// records of the two windows and which files are at their ends.
IL_HD void pn_decide(uint32_t n_pairs, uint32_t li, uint32_t lj, uint32_t r0, uint32_t r1, bool eof0, bool eof1, uint32_t dec[2]) {
    dec[0] = n_pairs ? li + 1u : 0u;
    dec[1] = n_pairs ? lj + 1u : 0u;
    if (eof1) dec[0] = r0;
    if (eof0) dec[1] = r1;
}

// KEPT SINGLES (VS_PN_KEEP).  A kept single of a round is a DECIDED record that is in no pair: file-1 record i < dec[0] with
// mate[i] none; file-2 record j < dec[1] that no pair names (mated[j], one byte per file-2 record, scattered from mate[]).
// A record behind dec[f] is not a single of this round: it is in the next windows and is judged there, once.  With the cut
// independence above, the kept singles of file f over all rounds are, for a valid input, exactly the complete records of file
// f whose key is not in both files, in file order.  The two predicates, for the compaction kernels and the host twin:
struct PnUnmated0 {
    const uint32_t *mate;
    IL_HD bool operator()(uint32_t i) const { return mate[i] == PN_NONE; }
};
struct PnUnmated1 {
    const uint8_t *mated;
    IL_HD bool operator()(uint32_t j) const { return mated[j] == 0u; }
};

// mated[] of the n1 file-2 records from mate[] of the n0 file-1 records, on one host thread
inline void pn_mated_host(const uint32_t *mate, uint32_t n0, uint8_t *mated, uint32_t n1) {
    for (uint32_t j = 0; j < n1; j++) mated[j] = 0u;
    for (uint32_t i = 0; i < n0; i++)
        if (mate[i] < n1) mated[mate[i]] = 1u;
}

// the records r < dec with pred(r), in order, into out (at most cap of them); returns how many there are
template <class Pred>
inline uint32_t pn_singles_host(const Pred &pred, uint32_t dec, uint32_t *out, uint64_t cap) {
    uint32_t q = 0;
    for (uint32_t r = 0; r < dec; r++)
        if (pred(r)) {
            if (q < cap) out[q] = r;
            q++;
        }
    return q;
}

// The join on one host thread.  rec (2 * min(R0, R1) words): rec[2p], rec[2p + 1] = the file-1 and the file-2 record of pair p.
// res: [0] pairs (beyond min(R0, R1) only with res[1] set), [1] the smallest file-1 record whose key occurs twice, [2] the same of file 2, [3] the first pair whose
// file-2 record does not lie behind the one before it, [4] table full (PN_NONE / 0: none).
inline void pn_join_host(const PnJoin &J, uint32_t bits, uint32_t *rec, uint32_t res[5]) {
    res[0] = 0u;
    res[1] = res[2] = res[3] = PN_NONE;
    res[4] = 0u;
    for (uint32_t s = 0; s < J.T; s++) J.claim[s] = J.mem0[s] = J.mem1[s] = PN_NONE;
    for (uint32_t g = 0; g < J.n_all; g++) pn_hash_at(J, g, bits);
    for (uint32_t g = 0; g < J.n_all; g++) pn_claim_at(J, g, &res[1], &res[4]);
    const uint32_t cap = J.f0.n_rec < J.f1.n_rec ? J.f0.n_rec : J.f1.n_rec;
    uint32_t p = 0;
    for (uint32_t i = 0; i < J.f0.n_rec; i++) {
        const uint32_t j = pn_partner_at(J, i);
        if (j == PN_NONE) continue;
        if (p < cap) {  // (more only where a key occurs twice in file 1: res[1] says so, and the caller gives no pairs then)
            if (p && j <= rec[2u * p - 1u] && res[3] == PN_NONE) res[3] = p;
            rec[2u * p] = i;
            rec[2u * p + 1u] = j;
        }
        p++;
    }
    res[0] = p;
}
