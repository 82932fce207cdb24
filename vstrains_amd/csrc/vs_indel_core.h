// The look left of a breakpoint on a shifted diagonal (vs_node_indels, k_node_indels in vs_pe.hip): what one lane does with a
// maximal exact match (a, qa, len) of a read end with a strand of a segment whose left neighbour lies inside both texts -- and
// so does not agree -- as __host__ __device__ functions over packed text, so that the window arithmetic runs on a CPU exactly
// as it runs on the device (vs_indel_scan_host, tests/test_indel_scan_cpu.py).  Plain C++: a host compiler takes this header
// as it is.  Packed text, windows and the agreement rule are vs_pileup_core.h's.
//
//   find      : the candidates deletion 1, insertion 1, deletion 2, ... insertion G, in this order; the first whose K-base left
//               flank agrees is the event.  A deletion of L lays the read's [a - K, a) on the diagonal qa - a - L, an insertion of
//               L lays [a - L - K, a - L) on the diagonal qa - a + L.  The flank is compared in windows of 32 bases from the
//               breakpoint leftwards: the first window rejects almost every candidate.
//   normalise : the raw event in forward coordinates of the segment (mirrored, the insert reverse complemented, on strand 1),
//               then moved left along the forward text as far as it goes.
#ifndef VS_INDEL_CORE_H
#define VS_INDEL_CORE_H
#include "vs_pileup_core.h"

#define VS_INDEL_MAX_LEN 32u
#define VS_INDEL_UNTESTED 0u  // a == 0 or qa == 0: the match has no left neighbour inside both texts
#define VS_INDEL_NONE 1u      // tested, no candidate holds
#define VS_INDEL_EVENT 2u
#define VS_INDEL_DROPPED 3u   // an insertion whose inserted bytes hold one outside ACGT
#define VS_INDEL_DEL 0u
#define VS_INDEL_INS 1u

// 1: the K read bases [x, x + K) all agree with the strand on diagonal d (x + d >= 0 is the caller's to keep)
VS_PL_HD uint32_t vs_indel_flank(const uint32_t *rw, uint64_t rbase, const uint32_t *tw, uint64_t tbase, const uint32_t *mk, uint32_t x, int64_t d, uint32_t K) {
    uint32_t left = K;  // bases [x, x + left) are still to be compared
    while (left) {
        const uint32_t n = left < 32u ? left : 32u;
        if (vs_pl_differ(rw, rbase, tw, tbase, mk, x + left - n, d, n)) return 0u;
        left -= n;
    }
    return 1u;
}

// The candidate loop of a tested match (a > 0, qa > 0).  -> VS_INDEL_NONE / EVENT / DROPPED; *kind and *len are written with
// the candidate that held (EVENT, DROPPED).
VS_PL_HD uint32_t vs_indel_find(const uint32_t *rw, uint64_t rbase, const uint32_t *tw, uint64_t tbase, const uint32_t *mk, uint32_t a, uint32_t qa, uint32_t K,
                                uint32_t G, uint32_t *kind, uint32_t *len) {
    if (a < K || qa < K) return VS_INDEL_NONE;  // no candidate has room for its flank
    const int64_t d0 = (int64_t)qa - (int64_t)a;
    for (uint32_t L = 1u; L <= G; L++) {
        if (qa >= L + K && vs_indel_flank(rw, rbase, tw, tbase, mk, a - K, d0 - (int64_t)L, K)) {
            *kind = VS_INDEL_DEL;
            *len = L;
            return VS_INDEL_EVENT;
        }
        if (a >= L + K && vs_indel_flank(rw, rbase, tw, tbase, mk, a - L - K, d0 + (int64_t)L, K)) {
            *kind = VS_INDEL_INS;
            *len = L;
            if (mk && (vs_pl_win(mk, rbase + a - L) & vs_pl_lowmask(2u * L))) return VS_INDEL_DROPPED;
            return VS_INDEL_EVENT;
        }
    }
    return VS_INDEL_NONE;
}

VS_PL_HD uint32_t vs_indel_base(const uint32_t *fw, uint64_t fbase, uint32_t p) {
    const uint64_t at = fbase + p;
    return (fw[at >> 4] >> ((uint32_t)(at & 15u) * 2u)) & 3u;
}

// The event of vs_indel_find on strand `strand` of a segment of tlen bases, forward text fw from base fbase: `ins` the inserted
// bases as the read has them (2 bits each, the first lowest; a deletion: anything).  -> *u: the forward position of the first
// deleted base / the position the insert stands before, left-aligned; *w1: the insert on the forward strand, 0 for a deletion.
VS_PL_HD void vs_indel_normalise(const uint32_t *fw, uint64_t fbase, uint32_t tlen, uint32_t strand, uint32_t kind, uint32_t L, uint32_t qa, uint64_t ins,
                                 uint32_t *u_out, uint64_t *w1_out) {
    if (kind == VS_INDEL_DEL) {
        uint32_t u = strand ? tlen - qa : qa - L;  // (the strand's [qa - L, qa) is the forward [tlen - qa, tlen - qa + L))
        while (u > 0u && vs_indel_base(fw, fbase, u - 1u) == vs_indel_base(fw, fbase, u + L - 1u)) u--;
        *u_out = u;
        *w1_out = 0ull;
        return;
    }
    const uint64_t keep = vs_pl_lowmask(2u * L);
    uint32_t u = qa;
    ins &= keep;
    if (strand) {
        uint64_t rc = 0ull;
        for (uint32_t i = 0u; i < L; i++) rc |= (3ull - ((ins >> (2u * i)) & 3ull)) << (2u * (L - 1u - i));
        ins = rc;
        u = tlen - qa;
    }
    while (u > 0u) {
        const uint64_t f = vs_indel_base(fw, fbase, u - 1u);
        if (f != ((ins >> (2u * (L - 1u))) & 3ull)) break;
        ins = ((ins << 2) | f) & keep;
        u--;
    }
    *u_out = u;
    *w1_out = ins;
}

#endif  // VS_INDEL_CORE_H
