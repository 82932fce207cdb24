// BAM records in a window of inflated bytes: the record rule, the chain of record starts through segments of `seg` bytes, the
// checks of a record and the 4-bit base table.  One text for the kernels (vs_bam.hip) and the host twin (vs_bam_scan_host),
// and plain C++ for tests/bam_check.cpp.
//
// A record at p is block_size = le32(p) and block_size bytes behind it: next(p) = p + 4 + block_size, block_size >= 32 (the
// fixed part).  Record starts are therefore a serial chain from a KNOWN start; nothing here ever guesses a start from what
// bytes look like -- quality and aux bytes may hold anything.
//
//   pass 1  per segment [lo, lo + seg): exit(p) for every byte p of it = the first position >= lo + seg the chain from p
//           reaches, as 16 bits relative to lo + seg (bam_exit_encode): BAM_X_DEAD when the chain meets a block_size < 32,
//           BAM_X_NEED when it meets a size field the window's end cuts, BAM_X_FAR when the exit lies further than the
//           16 bits say (bam_walk then follows the records of the segment from the bytes).
//   pass 2  bam_walk: from the start through the tables, one lookup per segment the chain touches; entry[s] = where the
//           chain enters segment s (BAM_NONE: it does not).
//   pass 3  per segment with an entry: its records, one after the other (bam_seg_next), each classified (bam_classify).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BAM_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define BAM_HD inline
#endif

#define BAM_SEG_MIN 64u
#define BAM_SEG_MAX 12288u  // (uint32 per byte in LDS: 48 KiB, three workgroups of k_bam_exits on a CU)
#define BAM_SEG_DEFAULT 12288u
#define BAM_NONE 0xFFFFFFFFu
#define BAM_FIXED 32u  // bytes of a record's fixed part behind block_size

enum { BAM_X_FAR = 0xFFFD, BAM_X_NEED = 0xFFFE, BAM_X_DEAD = 0xFFFF };  // exit codes; below BAM_X_FAR: exit - (lo + seg)
// what the chain from a position does next
enum { BAM_STEP_OK = 0, BAM_STEP_NEED = 1, BAM_STEP_DEAD = 2 };
// how a walk ended (bam_walk): at the window's end exactly, in front of a record the window's end cuts, at a block_size < 32
enum { BAM_END_CLEAN = 0, BAM_END_CUT = 1, BAM_END_DEAD = 2 };
// class of a record
enum { BAM_C_FIRST = 0, BAM_C_SECOND = 1, BAM_C_DROP900 = 2, BAM_C_OTHER = 3, BAM_C_MALFORMED = 4 };

BAM_HD uint32_t bam_le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
BAM_HD uint32_t bam_le16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

// one step of the chain from p < n: *next = p + 4 + block_size (64 bits: it may lie far beyond the window)
BAM_HD int bam_step(const uint8_t *win, uint64_t n, uint64_t p, uint64_t *next) {
    if (p + 4u > n) return BAM_STEP_NEED;
    const uint32_t bs = bam_le32(win + p);
    if (bs < BAM_FIXED) return BAM_STEP_DEAD;
    *next = p + 4u + (uint64_t)bs;
    return BAM_STEP_OK;
}

BAM_HD uint32_t bam_exit_encode(uint64_t exit, uint64_t seg_end) {
    const uint64_t d = exit - seg_end;
    return d < (uint64_t)BAM_X_FAR ? (uint32_t)d : (uint32_t)BAM_X_FAR;
}

// pass 1 with one thread: the table of segment [lo, hi), hi <= n, from its last byte to its first (exit(p) follows from
// exit(next(p)), which lies behind p)
inline void bam_seg_exits_serial(const uint8_t *win, uint64_t n, uint64_t lo, uint64_t hi, uint16_t *tab) {
    for (uint64_t p = hi; p-- > lo;) {
        uint64_t nx = 0;
        const int st = bam_step(win, n, p, &nx);
        tab[p] = (uint16_t)(st == BAM_STEP_NEED ? (uint32_t)BAM_X_NEED : st == BAM_STEP_DEAD ? (uint32_t)BAM_X_DEAD
                            : nx >= hi ? bam_exit_encode(nx, hi) : (uint32_t)tab[nx]);
    }
}

// pass 2: the chain from `start` through the tables.  entry[s] for s < n_seg = ceil(n / seg) must be BAM_NONE before.
// Returns BAM_END_*; *stop = n (clean), the start of the cut record, or the position of the block_size < 32.
BAM_HD int bam_walk(const uint8_t *win, uint64_t n, const uint16_t *tab, uint32_t seg, uint64_t start, uint32_t *entry, uint64_t *stop) {
    uint64_t pos = start;
    while (pos < n) {
        const uint64_t s = pos / seg, lo = s * seg, hi = lo + seg < n ? lo + seg : n;
        entry[s] = (uint32_t)pos;
        uint32_t code = tab[pos];
        if (code == (uint32_t)BAM_X_FAR || code >= (uint32_t)BAM_X_NEED) {  // from the bytes: the records of this segment
            uint64_t q = pos;
            for (;;) {
                uint64_t nx = 0;
                const int st = bam_step(win, n, q, &nx);
                if (st != BAM_STEP_OK) {
                    *stop = q;
                    return st == BAM_STEP_NEED ? BAM_END_CUT : BAM_END_DEAD;
                }
                if (nx > n) {
                    *stop = q;
                    return BAM_END_CUT;
                }
                q = nx;
                if (q >= hi) break;
            }
            pos = q;
            continue;
        }
        const uint64_t nx = hi + code;
        if (nx > n) {  // the last record of the segment's chain runs beyond the window: pass 3 finds it; here only that it is cut
            uint64_t q = pos, step = 0;
            while (bam_step(win, n, q, &step) == BAM_STEP_OK && step <= n) q = step;
            *stop = q;
            return BAM_END_CUT;
        }
        pos = nx;
    }
    *stop = n;
    return BAM_END_CLEAN;
}

struct BamRec {
    uint32_t off;      // of block_size in the window
    uint32_t flag_cls; // flag | BAM_C_* << 16
    uint32_t l_seq;
    uint32_t seq_off;  // of the 4-bit bases in the window
};

// the record at p (whole in the window: p + 4 + block_size <= n, block_size >= 32)
BAM_HD BamRec bam_classify(const uint8_t *win, uint64_t p) {
    const uint8_t *r = win + p;
    const uint32_t bs = bam_le32(r), l_name = r[12], n_cigar = bam_le16(r + 16), flag = bam_le16(r + 18), l_seq = bam_le32(r + 20);
    BamRec out;
    out.off = (uint32_t)p;
    out.l_seq = l_seq;
    const uint64_t front = (uint64_t)BAM_FIXED + l_name + 4ull * n_cigar;
    out.seq_off = (uint32_t)(p + 4u + front);
    uint32_t cls;
    if (front + ((uint64_t)l_seq + 1u) / 2u + (uint64_t)l_seq > (uint64_t)bs) {
        cls = BAM_C_MALFORMED;
        out.l_seq = 0;
    } else if (flag & 0x900u) cls = BAM_C_DROP900;
    else if (!(flag & 1u) || ((flag >> 6) & 1u) == ((flag >> 7) & 1u)) cls = BAM_C_OTHER;
    else cls = (flag & 0x40u) ? BAM_C_FIRST : BAM_C_SECOND;
    out.flag_cls = flag | (cls << 16);
    return out;
}

// pass 3: the next whole record of segment [.., hi) at or behind *p (start with the segment's entry): true and *p moved
// to the record behind it, *at = its start; false when the chain leaves the segment, is cut by the window's end or dead
BAM_HD bool bam_seg_next(const uint8_t *win, uint64_t n, uint64_t hi, uint64_t *p, uint64_t *at) {
    if (*p >= hi) return false;
    uint64_t nx = 0;
    if (bam_step(win, n, *p, &nx) != BAM_STEP_OK || nx > n) return false;
    *at = *p;
    *p = nx;
    return true;
}

// "=ACMGRSVTWYHKDBN": base i of a sequence is the high nibble of byte i / 2 for even i
BAM_HD uint32_t bam_nibble(const uint8_t *seq, uint32_t i) { return (seq[i >> 1] >> ((~i & 1u) * 4u)) & 15u; }
// the complement of a code: A=1 C=2 G=4 T=8 are the bits of the set of bases it stands for, so the four bits reversed
BAM_HD uint32_t bam_complement(uint32_t c) { return ((c & 1u) << 3) | ((c & 2u) << 1) | ((c & 4u) >> 1) | ((c & 8u) >> 3); }
BAM_HD uint8_t bam_letter(uint32_t c) {
    // (a 64-bit literal per half instead of a table in memory: "=ACMGRSV" and "TWYHKDBN", first letter in the low byte)
    const uint64_t lo = 0x565352474D43413Dull, hi = 0x4E42444B48595754ull;
    return (uint8_t)(((c & 8u) ? hi : lo) >> ((c & 7u) * 8u));
}
// letter p of an end of len bases as samtools fastq prints it: reversed and complemented when the flag has 0x10
BAM_HD uint8_t bam_base(const uint8_t *seq, uint32_t len, bool rev, uint32_t p) {
    return rev ? bam_letter(bam_complement(bam_nibble(seq, len - 1u - p))) : bam_letter(bam_nibble(seq, p));
}

// a couple of participating records: one first and one second, in either order
BAM_HD bool bam_couple_ok(uint32_t flag_cls_a, uint32_t flag_cls_b) { return ((flag_cls_a >> 16) ^ (flag_cls_b >> 16)) == 1u; }
