// The diagonal walk of the base pileup (vs_node_pileup, k_node_pileup in vs_pe.hip): what one lane does with a maximal exact
// match (a, qa, len) of a read end with a strand of a segment, as __host__ __device__ functions over packed text, so that the
// window arithmetic runs on a CPU exactly as it runs on the device (vs_pileup_scan_host, tests/test_pileup_scan_cpu.py).
// Plain C++: a host compiler takes this header as it is.
//
// Packed text: 2 bits a base, 16 bases a word, the first base in the lowest bits; the mask has 0b11 where the read's byte is
// outside ACGT (the word holds code 0 there).  A window is 32 bases (64 bits) from any base offset; it may reach past the
// end of a text into the buffer's padding (VS_PAD_WORDS), and the bits beyond the valid range are masked off before use,
// as in vs_extend.
//
// The alignment of a match lies on its diagonal d = qa - a (strand offset - read offset).  Its overlap is the read offsets
// x with 0 <= x < rlen and 0 <= x + d < tlen: [x_lo, x_hi) with x_lo = max(0, -d), x_hi = min(rlen, tlen - d).  A position
// AGREES when the read byte is one of ACGT and equals the strand's base: the 2-bit XOR is 0 and the mask is 0 there.
//
//   owner : several maximal matches may lie on one diagonal, cut apart by mismatches; the alignment is deposited once, by the
//           LEFTMOST of them.  The match's own left neighbour a - 1 does not agree (or is outside the overlap), so the walk
//           goes from a - 2 down to x_lo and stops at the first run of K agreeing bases: another match, which owns the
//           alignment -- or, by the same rule, hands it further left.  No run: this match is the leftmost and owns it.
//   count : the non-agreeing positions of the whole overlap, a popcount over the folded XOR.
#ifndef VS_PILEUP_CORE_H
#define VS_PILEUP_CORE_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VS_PL_HD __host__ __device__ __forceinline__
#else
#define VS_PL_HD inline
#endif

#define VS_PL_ODD 0x5555555555555555ull

// 32 bases from base offset `base` of a packed word array (vs_win64 of vs_internal.h, for host and device)
VS_PL_HD uint64_t vs_pl_win(const uint32_t *w, uint64_t base) {
    const uint64_t i = base >> 4;
    const uint32_t sh = (uint32_t)(base & 15u) * 2u;
    const uint64_t lo = (uint64_t)w[i] | ((uint64_t)w[i + 1] << 32);
    const uint64_t hi = (uint64_t)w[i + 2];
    return sh ? (lo >> sh) | (hi << (64u - sh)) : lo;
}

VS_PL_HD uint64_t vs_pl_lowmask(uint32_t bits) {  // bits in 0..64
    return bits >= 64u ? ~0ull : ((1ull << bits) - 1ull);
}

VS_PL_HD uint32_t vs_pl_popc(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(x);
#else
    return (uint32_t)__builtin_popcountll(x);
#endif
}

VS_PL_HD uint32_t vs_pl_top(uint64_t x) {  // index of the highest set bit, x != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return 63u - (uint32_t)__clzll((long long)x);
#else
    return 63u - (uint32_t)__builtin_clzll(x);
#endif
}

// One bit per base (bit 2i for base i of the window): set where the n bases from read offset x do NOT agree with the strand
// on diagonal (tbase + x + d).  rbase / tbase: first base of the read / the strand in their word arrays; mk: the read's
// mask (same layout as rw) or NULL.  x + d >= 0 is the caller's to keep.
VS_PL_HD uint64_t vs_pl_differ(const uint32_t *rw, uint64_t rbase, const uint32_t *tw, uint64_t tbase, const uint32_t *mk, uint32_t x, int64_t d,
                               uint32_t n) {
    uint64_t v = vs_pl_win(rw, rbase + x) ^ vs_pl_win(tw, (uint64_t)((int64_t)tbase + (int64_t)x + d));
    if (mk) v |= vs_pl_win(mk, rbase + x);
    return (v | (v >> 1)) & VS_PL_ODD & vs_pl_lowmask(2u * n);
}

struct VsPileupSpan {
    int64_t d;      // the diagonal: strand offset - read offset
    uint32_t x_lo;  // the overlap in read offsets: [x_lo, x_hi)
    uint32_t x_hi;
};

// (a <= rlen, qa <= tlen: a match lies inside both texts, so x_lo <= a < x_hi)
VS_PL_HD VsPileupSpan vs_pileup_span(uint32_t rlen, uint32_t tlen, uint32_t a, uint32_t qa) {
    VsPileupSpan sp;
    sp.d = (int64_t)qa - (int64_t)a;
    sp.x_lo = a > qa ? a - qa : 0u;
    const uint64_t hi = (uint64_t)a + (tlen - qa);  // tlen - d
    sp.x_hi = hi < rlen ? (uint32_t)hi : rlen;
    return sp;
}

// 1: the match that starts at read offset a is the leftmost anchor of its diagonal
VS_PL_HD uint32_t vs_pileup_owner(const uint32_t *rw, uint64_t rbase, const uint32_t *tw, uint64_t tbase, const uint32_t *mk, VsPileupSpan sp, uint32_t a,
                                  uint32_t K) {
    if (a < sp.x_lo + 1u + K) return 1u;  // no room for K bases left of the mismatch at a - 1
    uint32_t p = a - 1u;  // the bases below p are still to be looked at: x_lo .. p - 1
    uint32_t run = 0u;    // agreeing bases in a row from p upwards
    while (p > sp.x_lo) {
        if (p - sp.x_lo + run < K) return 1u;  // what is left cannot hold a run of K
        const uint32_t n = p - sp.x_lo < 32u ? p - sp.x_lo : 32u;
        uint64_t f = vs_pl_differ(rw, rbase, tw, tbase, mk, p - n, sp.d, n);
        uint32_t top = n;  // the window's bases below `top` are not yet counted
        while (f) {
            const uint32_t h = vs_pl_top(f) >> 1;
            if (run + (top - 1u - h) >= K) return 0u;
            run = 0u;
            top = h;
            f &= ~(1ull << (2u * h));
        }
        run += top;
        if (run >= K) return 0u;
        p -= n;
    }
    return 1u;
}

// the non-agreeing positions of the overlap
VS_PL_HD uint32_t vs_pileup_count(const uint32_t *rw, uint64_t rbase, const uint32_t *tw, uint64_t tbase, const uint32_t *mk, VsPileupSpan sp) {
    uint32_t c = 0u;
    for (uint32_t x = sp.x_lo; x < sp.x_hi; x += 32u) {
        const uint32_t n = sp.x_hi - x < 32u ? sp.x_hi - x : 32u;
        c += vs_pl_popc(vs_pl_differ(rw, rbase, tw, tbase, mk, x, sp.d, n));
    }
    return c;
}

#endif  // VS_PILEUP_CORE_H
