// Which records of ONE interleaved FASTQ window are mates (vs_interleaved.hip): the name token of a record, the rule that
// says two adjacent records are mates, and the greedy pairing of `bwa mem -p` written so that it can be scanned.  One
// statement for the kernels and for the one-thread host twin (vs_fastq_mates_host), as vs_bam_core.h is for the BAM ingest.
//
// Name token: a record's first line from its first byte up to (not including) the first space, tab or the line's end.
// mates(a, b): the two tokens -- without their last two bytes when a's ends in "/1" AND b's in "/2" -- are non-empty and
// equal byte for byte.
//
// Pairing, greedy from the front: record i and i + 1 are a pair when they are mates, else i is a single.  With
// m[i] = mates(i, i + 1) (false for the last record) and t(i) = the number of consecutive true m directly below i, record i
// is the SECOND of a pair iff t(i) is odd; else the FIRST iff m[i]; else a SINGLE.  Only the parity p(i) of t(i) matters:
//     p(0) = 0,  p(i + 1) = m[i] ? !p(i) : 0
// -- per record a function of one bit (flip or const-0), and functions of one bit compose: four of them exist (const-0,
// const-1, identity, flip), so the parity is a scan however long a run of equal names is.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define IL_HD __host__ __device__ inline
#else
#define IL_HD inline
#endif

enum { IL_FIRST = 0, IL_SECOND = 1, IL_SINGLE = 2, IL_HELD = 3 };
#define IL_NONE 0xFFFFFFFFu

// bytes of the name token of the line q[0, n)
IL_HD uint32_t il_token_len(const uint8_t *q, uint32_t n) {
    uint32_t k = 0;
    while (k < n && q[k] != 0x20u && q[k] != 0x09u) k++;
    return k;
}

// the header lines a[0, na) and b[0, nb) (without their line ends) of two adjacent records: are the records mates?
IL_HD bool il_mates(const uint8_t *a, uint32_t na, const uint8_t *b, uint32_t nb) {
    uint32_t la = il_token_len(a, na), lb = il_token_len(b, nb);
    if (la >= 2u && lb >= 2u && a[la - 2u] == '/' && a[la - 1u] == '1' && b[lb - 2u] == '/' && b[lb - 1u] == '2') la -= 2u, lb -= 2u;
    if (!la || la != lb) return false;
    for (uint32_t k = 0; k < la; k++)
        if (a[k] != b[k]) return false;
    return true;
}

// the class of record i from p(i) and m[i]; the parity of the record behind it
IL_HD uint32_t il_class(uint32_t parity, bool m) { return parity ? (uint32_t)IL_SECOND : m ? (uint32_t)IL_FIRST : (uint32_t)IL_SINGLE; }
IL_HD uint32_t il_step(uint32_t parity, bool m) { return m ? parity ^ 1u : 0u; }

// A function f of one bit as two bits: f(0) | f(1) << 1.
enum { IL_F_CONST0 = 0, IL_F_FLIP = 1, IL_F_ID = 2, IL_F_CONST1 = 3 };
IL_HD uint32_t il_apply(uint32_t f, uint32_t x) { return (f >> x) & 1u; }
// g after f
IL_HD uint32_t il_compose(uint32_t f, uint32_t g) { return il_apply(g, il_apply(f, 0u)) | (il_apply(g, il_apply(f, 1u)) << 1); }

// 64 records in a row, bit l of b = m of the l-th: the number of consecutive set bits directly below bit l (l in 0..64)
IL_HD uint32_t il_ones_below(uint64_t b, uint32_t l) {
    if (!l) return 0u;
    const uint64_t x = ~(b << (64u - l));  // (the bits below l at the top, zeros for ones; the low 64 - l bits are set)
    if (!x) return 64u;                    // (l = 64 and every bit set)
#ifdef __HIP_DEVICE_COMPILE__
    return (uint32_t)__clzll((long long)x);
#else
    return (uint32_t)__builtin_clzll(x);
#endif
}
// p of the l-th of those records from p of the first; the function that takes p of the first to p of the one behind the last
IL_HD uint32_t il_wave_parity(uint64_t b, uint32_t l, uint32_t p_in) {
    const uint32_t c = il_ones_below(b, l);
    return c < l ? (c & 1u) : (l & 1u) ^ p_in;
}
IL_HD uint32_t il_wave_fn(uint64_t b) {
    const uint32_t c = il_ones_below(b, 64u);
    return c < 64u ? ((c & 1u) ? (uint32_t)IL_F_CONST1 : (uint32_t)IL_F_CONST0) : (uint32_t)IL_F_ID;
}
// the same for the first n (1..64) of those records alone: a run of n true m flips n times
IL_HD uint32_t il_run_fn(uint64_t b, uint32_t n) {
    const uint32_t c = il_ones_below(b, n);
    if (c < n) return (c & 1u) ? (uint32_t)IL_F_CONST1 : (uint32_t)IL_F_CONST0;
    return (n & 1u) ? (uint32_t)IL_F_FLIP : (uint32_t)IL_F_ID;
}

// The records of one window: its text, the byte offsets of its line ends (n_nl of them), R complete records.  Header line
// of record i = [start, end): it has a line end of its own whenever the record is complete.
struct IlWin {
    const uint8_t *txt;
    const uint32_t *ends;
    uint32_t n_rec;
};
IL_HD bool il_mates_at(const IlWin &w, uint32_t i) {  // m[i], i + 1 < n_rec
    const uint32_t a0 = i ? w.ends[4u * i - 1u] + 1u : 0u, a1 = w.ends[4u * i];
    const uint32_t b0 = w.ends[4u * i + 3u] + 1u, b1 = w.ends[4u * i + 4u];
    return il_mates(w.txt + a0, a1 - a0, w.txt + b0, b1 - b0);
}
