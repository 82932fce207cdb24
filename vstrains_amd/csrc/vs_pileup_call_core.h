// The rule by which ONE position of the base pileup becomes records of --variants (vs_pileup_call), as one __host__ __device__
// function, so that the code both passes of the device caller run (k_pileup_call_count, k_pileup_call_write, vs_pe.hip) is
// held to tests/strand_pileup_model.py on a CPU (vs_pileup_call_host, tests/test_strand_pileup_call_cpu.py).  Plain C++: a
// host compiler takes this header as it is.
//
//   planes : 1 -- the tables of the unstranded pileup (vs_node_pileup): depth, alt[5]; 2 -- those of the stranded one
//            (vs_node_pileup_strands): plane 0 the alignments on the segment's forward text, plane 1 those on its reverse
//            complement.  A missing second plane counts as zeros.
//   counts : count[t][b] = alt[t][b] for b != ref, count[t][ref] = depth[t] - (alt[t][0] + .. + alt[t][4]): the reads that
//            agree.  `other` (column 4) stays out of every number below.
//   DP     : the sum of count[t][b] over both planes and A, C, G, T.
//   AD     : for an alternate base b != ref, count[0][b] + count[1][b].
//   record : b is one when AD > 0, AD >= min_alt_count and (double)AD >= min_alt_frac * (double)DP -- ONE IEEE double product,
//            compared as it stands (the library is built with -ffp-contract=off; no division, no fused operation): what
//            Python forms in `ad >= min_alt_frac * dp`.  Up to three per position, in ACGT order.
//   DP4    : ref_f, ref_r, alt_f, alt_r = count[0][ref], count[1][ref], count[0][b], count[1][b].
//   strand : with min_alt_strand >= 1 a record FAILS when alt_f or alt_r is below it; the record stays.
//
// A record is six uint64: slot << 5 | strand_fail << 4 | ref << 2 | alt, then DP, ref_f, ref_r, alt_f, alt_r.
#ifndef VS_PILEUP_CALL_CORE_H
#define VS_PILEUP_CALL_CORE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define VS_PC_HD __host__ __device__ __forceinline__
#else
#define VS_PC_HD inline
#endif

#define PILEUP_CALL_WORDS 6u  // uint64 words of a record
#define PILEUP_CALL_MOST 3u   // records of one position: the three bases that are not the reference
#define PILEUP_CALL_TPB 256u  // threads of a workgroup of either pass: one lane per slot

// may these thresholds be applied to tables of `planes` planes?  (a negated comparison: a NaN fraction fails it)
VS_PC_HD bool vs_pileup_call_args_ok(uint32_t planes, double min_alt_frac, uint64_t min_alt_strand) {
    if (planes != 1u && planes != 2u) return false;
    if (!(min_alt_frac >= 0.0)) return false;
    return planes == 2u || !min_alt_strand;
}

// The records of one position.  ref: the segment's base there (0..3); depth[2], alt[2][5]: both planes (zeros for a plane the
// tables do not have); slot: what the records carry as their place; out: NULL (count only), or room for PILEUP_CALL_MOST
// records.  -> how many.  Every array is indexed by constants once the loops are unrolled: no lane keeps one in memory.
VS_PC_HD uint32_t vs_pileup_call_slot(uint32_t ref, const uint64_t depth[2], const uint64_t alt[2][5], uint64_t min_alt_count, double min_alt_frac,
                                      uint64_t min_alt_strand, uint64_t slot, uint64_t *out) {
    uint64_t cnt[2][4];
    uint64_t dp = 0u, ref_f = 0u, ref_r = 0u;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t t = 0u; t < 2u; t++) {
        const uint64_t agree = depth[t] - (alt[t][0] + alt[t][1] + alt[t][2] + alt[t][3] + alt[t][4]);
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t b = 0u; b < 4u; b++) {
            cnt[t][b] = b == ref ? agree : alt[t][b];
            dp += cnt[t][b];
        }
        if (t) ref_r = agree; else ref_f = agree;
    }
    const double bar = min_alt_frac * (double)dp;
    uint32_t n = 0u;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t b = 0u; b < 4u; b++) {
        const uint64_t ad = cnt[0][b] + cnt[1][b];
        if (b == ref || !ad || ad < min_alt_count || !((double)ad >= bar)) continue;
        if (out) {
            const uint64_t fail = min_alt_strand && (cnt[0][b] < min_alt_strand || cnt[1][b] < min_alt_strand) ? 1u : 0u;
            uint64_t *r = out + (uint64_t)n * PILEUP_CALL_WORDS;
            r[0] = slot << 5 | fail << 4 | (uint64_t)ref << 2 | b;
            r[1] = dp;
            r[2] = ref_f;
            r[3] = ref_r;
            r[4] = cnt[0][b];
            r[5] = cnt[1][b];
        }
        n++;
    }
    return n;
}

#endif  // VS_PILEUP_CALL_CORE_H
