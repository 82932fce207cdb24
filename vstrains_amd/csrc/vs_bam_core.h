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

#include <vector>

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

// ---- mates by name ---------------------------------------------------------------------------------------------------------
// The rule, once: the participating records (classes first and second) are walked in file order and a set of waiting
// records is kept.  A record of class c looks for waiting records of the same name and the OTHER class; it forms a pair
// with the OLDEST of them (which stops waiting), or waits itself when there is none.  So the j-th first of a name pairs
// with the j-th second of that name, pairs are delivered in the order of the record that completed them, and what waits
// at the end of the input are singletons.  The name of a record is its l_read_name bytes as they lie in the record,
// terminator included; names are equal when lengths and bytes are, never because a hash is.
//
// Window-wise, which is what the kernels and the host twin run: in a window [waiting records of earlier windows, in file
// order][new records] the members of a name are ranked within their own class in window order; member i is paired exactly
// when its rank is below the number of members of the other class, with the other class's member of the same rank, and the
// LATER of the two emits the pair.  The waiting records of one name are all of one class (two of different classes would
// have paired), they are the oldest unpaired of it and keep their order, so ranks in the window continue the ranks in the
// file and the two forms give the same pairs, the same order and the same waiting set wherever the windows are cut.
//
//   hash     bam_name_hash of every participating record (VS_BAM_NAME_BITS / hash_bits keep the low bits only: tests)
//   claim    bam_mate_claim: an open-address table of participating indices, a power of two and at most half full; a
//            record probes linearly from its hash, claims an empty slot by compare-and-swap or finds its name's
//            representative there (hash first, then the bytes); then it pushes itself on the slot's list (exchange)
//   rank     bam_mate_rank: a walk of the name's list, at most 2 * BAM_MATE_CAP + 1 steps: rank in the own class, paired or
//            not; more than BAM_MATE_CAP records of one name and class in a window are refused ("crowded"), which bounds
//            every walk
//   partner  bam_mate_partner: the same walk for the other class's member of the same rank
#define BAM_MATE_CAP 64u
#define BAM_MATE_PAIRED 0x80000000u  // in rank[]: the member is paired in this window

struct BamMates {
    const uint8_t *win;
    const uint32_t *recs;  // 4 words per record: BamRec
    const uint32_t *part;  // record index of every participating record, in window order
    uint32_t n_rec, n_part;
    uint64_t *hash;         // [n_part]
    uint32_t *table, *head; // [size]: participating index of the name's representative / of the newest pushed member
    uint32_t size;          // a power of two >= 2 * n_part
    uint32_t *slot, *next, *rank;  // [n_part]
};

BAM_HD uint32_t bam_table_size(uint32_t n_part) {
    uint32_t s = 2u;
    while (s < 2u * n_part && s < 0x80000000u) s <<= 1;
    return s;
}

BAM_HD uint32_t bam_cas(uint32_t *p, uint32_t expect, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicCAS(p, expect, v);
#else
    const uint32_t old = *p;
    if (old == expect) *p = v;
    return old;
#endif
}
BAM_HD uint32_t bam_exch(uint32_t *p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicExch(p, v);
#else
    const uint32_t old = *p;
    *p = v;
    return old;
#endif
}

// the name of the (well-formed, whole) record at off: l_read_name bytes behind the fixed part
BAM_HD uint64_t bam_name_hash(const uint8_t *win, uint32_t off, uint32_t bits) {
    const uint8_t *p = win + off;
    const uint32_t l = p[12];
    uint64_t h = 0xCBF29CE484222325ull;  // FNV-1a, then the finaliser of MurmurHash3 so that the low bits depend on every byte
    for (uint32_t i = 0; i < l; i++) h = (h ^ p[36u + i]) * 0x100000001B3ull;
    h ^= h >> 33;
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    h *= 0xC4CEB9FE1A85EC53ull;
    h ^= h >> 33;
    return bits >= 64u ? h : bits == 0u ? 0ull : h & ((1ull << bits) - 1ull);
}
BAM_HD bool bam_name_eq(const uint8_t *win, uint32_t off_a, uint32_t off_b) {
    const uint8_t *a = win + off_a, *b = win + off_b;
    const uint32_t l = a[12];
    if (l != b[12]) return false;
    for (uint32_t i = 0; i < l; i++)
        if (a[36u + i] != b[36u + i]) return false;
    return true;
}

// participating record i < n_part: its record (BAM_NONE: an index out of range), offset and class
BAM_HD uint32_t bam_mate_rec(const BamMates &m, uint32_t i) {
    const uint32_t r = m.part[i];
    return r < m.n_rec ? r : BAM_NONE;
}
BAM_HD uint32_t bam_mate_off(const BamMates &m, uint32_t i) { return m.recs[4u * m.part[i]]; }
BAM_HD uint32_t bam_mate_cls(const BamMates &m, uint32_t i) { return m.recs[4u * m.part[i] + 1u] >> 16; }

// the slot of i's name (table[] and head[] are BAM_NONE before the first claim); BAM_NONE: no slot within `size` probes
BAM_HD uint32_t bam_mate_claim(const BamMates &m, uint32_t i) {
    const uint32_t mask = m.size - 1u, off = bam_mate_off(m, i);
    const uint64_t h = m.hash[i];
    uint32_t s = (uint32_t)h & mask;
    for (uint32_t probe = 0; probe < m.size; probe++, s = (s + 1u) & mask) {
        const uint32_t v = bam_cas(&m.table[s], BAM_NONE, i);  // (what the slot held: a lost race reads the winner here)
        if (v == BAM_NONE || v == i) return s;
        if (v < m.n_part && m.hash[v] == h && bam_name_eq(m.win, bam_mate_off(m, v), off)) return s;
    }
    return BAM_NONE;
}
BAM_HD void bam_mate_push(const BamMates &m, uint32_t i, uint32_t s) {
    m.slot[i] = s;
    m.next[i] = s < m.size ? bam_exch(&m.head[s], i) : BAM_NONE;
}

// rank of i among the members of its name and class in window order | BAM_MATE_PAIRED; *crowded: the name has more than
// BAM_MATE_CAP members of one class in the window (the rank then means nothing)
BAM_HD uint32_t bam_mate_rank(const BamMates &m, uint32_t i, bool *crowded) {
    const uint32_t cls = bam_mate_cls(m, i), s = m.slot[i];
    uint32_t lower = 0, own = 0, other = 0, steps = 0;
    uint32_t j = s < m.size ? m.head[s] : BAM_NONE;
    while (j < m.n_part && steps <= 2u * BAM_MATE_CAP) {  // (BAM_NONE ends a list)
        if (bam_mate_cls(m, j) == cls) {
            own++;
            lower += j < i ? 1u : 0u;
        } else other++;
        j = m.next[j];
        steps++;
    }
    *crowded = j < m.n_part || own > BAM_MATE_CAP || other > BAM_MATE_CAP;
    return lower | (lower < other ? BAM_MATE_PAIRED : 0u);
}

// the member of the other class with i's rank (rank[] complete), BAM_NONE: there is none
BAM_HD uint32_t bam_mate_partner(const BamMates &m, uint32_t i) {
    const uint32_t cls = bam_mate_cls(m, i), s = m.slot[i], r = m.rank[i] & ~BAM_MATE_PAIRED;
    uint32_t steps = 0;
    uint32_t j = s < m.size ? m.head[s] : BAM_NONE;
    while (j < m.n_part && steps <= 2u * BAM_MATE_CAP) {
        if (bam_mate_cls(m, j) != cls && (m.rank[j] & ~BAM_MATE_PAIRED) == r) return j;
        j = m.next[j];
        steps++;
    }
    return BAM_NONE;
}

// All passes with one thread.  pairs[2 p], [2 p + 1]: record index of the first and the second of pair p, in delivery order
// (at most cap_pairs pairs written); waiting[]: record index of every record left waiting, in window order (at most
// cap_waiting); info[0] = pairs, [1] = waiting, [2] = the newest record of a crowded name (then no pair and no waiting
// record is reported) or ~0, [3] = 1 when a record found no slot (the table was not half empty).
inline void bam_mates_serial(const BamMates &m, uint32_t bits, uint32_t *pairs, uint64_t cap_pairs, uint32_t *waiting, uint64_t cap_waiting,
                             uint64_t info[4]) {
    for (uint32_t s = 0; s < m.size; s++) m.table[s] = m.head[s] = BAM_NONE;
    uint64_t full = 0, crowded = ~0ull, n_pairs = 0, n_wait = 0;
    for (uint32_t i = 0; i < m.n_part; i++) m.hash[i] = bam_name_hash(m.win, bam_mate_off(m, i), bits);
    for (uint32_t i = 0; i < m.n_part; i++) {
        const uint32_t s = bam_mate_claim(m, i);
        if (s == BAM_NONE) full = 1;
        bam_mate_push(m, i, s);
    }
    for (uint32_t i = 0; i < m.n_part; i++) {
        bool c = false;
        m.rank[i] = bam_mate_rank(m, i, &c);
        if (c) crowded = m.part[i];  // (i rises: the newest stays)
    }
    if (crowded == ~0ull && !full)
        for (uint32_t i = 0; i < m.n_part; i++) {
            if (!(m.rank[i] & BAM_MATE_PAIRED)) {
                if (n_wait < cap_waiting) waiting[n_wait] = m.part[i];
                n_wait++;
                continue;
            }
            const uint32_t j = bam_mate_partner(m, i);
            if (j >= i) continue;  // (the later of the two emits)
            const bool i_first = bam_mate_cls(m, i) == (uint32_t)BAM_C_FIRST;
            if (n_pairs < cap_pairs) {
                pairs[2u * n_pairs] = m.part[i_first ? i : j];
                pairs[2u * n_pairs + 1u] = m.part[i_first ? j : i];
            }
            n_pairs++;
        }
    info[0] = n_pairs;
    info[1] = n_wait;
    info[2] = crowded;
    info[3] = full;
}

// ---- the summary of a share (member-sharded BAM) ---------------------------------------------------------------------------
// A rank of a sharded run holds the inflated bytes [S, S + E) of its members ("the share") and at least BAM_SUM_TAIL bytes
// behind them, or everything up to the end of the file.  It does not know where the true chain enters the share, so it
// follows the chain from every candidate start c (positions are relative to S) and keeps, per candidate,
//   X[c]  the first position >= E the chain from c reaches, minus E; BAM_SUM_DEAD when it meets a block_size < 32 first;
//         BAM_SUM_CUT when the end of the file cuts a size field or the fixed part of a record that starts in the share
//         (a record whose variable part runs beyond the end of the file shows as an X beyond it: bam_shard_plan sees that);
//   N[c]  the participating records (classes first and second) that start on that chain inside the share; its parity is
//         the Q of the plan, the count itself places the rank's couples among the file's.
// Nothing guesses which candidate is a record start: every candidate is followed, and the one the previous share's chain
// hands over is picked after the exchange (bam_shard_plan).
//
//   tables   per segment [lo, hi) of a window, hi clipped to the window's limit `lim`: exit(p) as above and cnt(p) = the
//            participating records on the chain from p that start in [p, hi) (bam_seg_exits_cnt_serial / k_bam_exits_cnt);
//            every p < lim has its size field and its fixed part inside the window's n bytes, unless the file ends there
//   lanes    bam_lane_walk: a lane per live candidate, one lookup per segment it touches; position and count are carried
//            from window to window.  Chains go strictly forward: a lane's loop is bounded by the segments of the window.
#define BAM_SUM_TAIL 64u
#define BAM_SUM_DEAD 0xFFFFFFFFFFFFFFFFull
#define BAM_SUM_CUT 0xFFFFFFFFFFFFFFFEull
enum { BAM_LANE_LIVE = 0, BAM_LANE_DEAD = 1, BAM_LANE_CUT = 2 };

// the record at p (its size field read, block_size >= 32) counts when its fixed part lies in win[0, n) and it takes part
BAM_HD uint32_t bam_takes_part(const uint8_t *win, uint64_t n, uint64_t p) {
    return p + 4u + BAM_FIXED <= n && (bam_classify(win, p).flag_cls >> 16) <= (uint32_t)BAM_C_SECOND ? 1u : 0u;
}

// one step of a summary chain from p < n: BAM_STEP_NEED also when the window's end cuts the fixed part (with the limits of
// the summary windows that is the end of the file); *part = 1 when the record takes part
BAM_HD int bam_step_cnt(const uint8_t *win, uint64_t n, uint64_t p, uint64_t *next, uint32_t *part) {
    const int st = bam_step(win, n, p, next);
    if (st != BAM_STEP_OK) return st;
    if (p + 4u + BAM_FIXED > n) return BAM_STEP_NEED;
    *part = bam_takes_part(win, n, p);
    return BAM_STEP_OK;
}

// the tables of segment [lo, hi), hi <= lim <= n, with one thread (from the last byte to the first)
inline void bam_seg_exits_cnt_serial(const uint8_t *win, uint64_t n, uint64_t lo, uint64_t hi, uint16_t *tab, uint16_t *cnt) {
    for (uint64_t p = hi; p-- > lo;) {
        uint64_t nx = 0;
        uint32_t part = 0;
        const int st = bam_step_cnt(win, n, p, &nx, &part);
        if (st != BAM_STEP_OK) {
            tab[p] = (uint16_t)(st == BAM_STEP_NEED ? BAM_X_NEED : BAM_X_DEAD);
            cnt[p] = 0;
        } else if (nx >= hi) {
            tab[p] = (uint16_t)bam_exit_encode(nx, hi);
            cnt[p] = (uint16_t)part;
        } else {
            tab[p] = tab[nx];
            cnt[p] = (uint16_t)(cnt[nx] + part);
        }
    }
}

struct BamLane {
    uint64_t pos;    // relative to S: where the chain stands (live), or where it met what ended it
    uint64_t count;  // participating records passed so far
    uint32_t state;  // BAM_LANE_*
    uint32_t pad;
};

// A live lane through the window win[0, n) that starts at position `base` (relative to S), tables for [0, lim): it moves
// while base <= pos < base + lim.  At most one table lookup or one walk of a segment's records per segment of the window.
BAM_HD void bam_lane_walk(const uint8_t *win, uint64_t n, uint64_t lim, const uint16_t *tab, const uint16_t *cnt, uint32_t seg, uint64_t base,
                          BamLane *lane) {
    if (lane->state != (uint32_t)BAM_LANE_LIVE || lane->pos < base) return;
    uint64_t p = lane->pos - base, count = lane->count;
    uint32_t state = BAM_LANE_LIVE;
    while (p < lim) {
        const uint64_t lo = p / seg * seg, hi = lo + seg < lim ? lo + seg : lim;
        const uint32_t code = tab[p];
        if (code < (uint32_t)BAM_X_FAR) {
            count += cnt[p];
            p = hi + code;
            continue;
        }
        for (;;) {  // from the bytes: the records of this segment (a far exit, a dead or a cut chain)
            uint64_t nx = 0;
            uint32_t part = 0;
            const int st = bam_step_cnt(win, n, p, &nx, &part);
            if (st != BAM_STEP_OK) {
                state = st == BAM_STEP_NEED ? BAM_LANE_CUT : BAM_LANE_DEAD;
                break;
            }
            count += part;
            p = nx;
            if (p >= hi) break;
        }
        if (state != (uint32_t)BAM_LANE_LIVE) break;
    }
    lane->pos = base + p;
    lane->count = count;
    lane->state = state;
}

// what a lane says once the share's last window is done: X (BAM_SUM_*), N
BAM_HD uint64_t bam_lane_exit(const BamLane &lane, uint64_t share) {
    if (lane.state == (uint32_t)BAM_LANE_DEAD) return BAM_SUM_DEAD;
    if (lane.state == (uint32_t)BAM_LANE_CUT || lane.pos < share) return BAM_SUM_CUT;  // (pos < share: the bytes ended before the share did)
    return lane.pos - share;
}

// the limit of a summary window of n bytes at `base`: positions below it are walked in this window.  More bytes follow
// (`last` = 0): the final BAM_FIXED + 3 bytes wait for them, so that every walked record has its fixed part in the window.
BAM_HD uint64_t bam_sum_limit(uint64_t n, uint64_t base, uint64_t share, int last) {
    const uint64_t keep = (uint64_t)BAM_FIXED + 3u, here = last ? n : (n > keep ? n - keep : 0u);
    const uint64_t left = share > base ? share - base : 0u;
    return here < left ? here : left;
}

// The summary with one thread: share[0, n) are the inflated bytes from S on (share_size of them the share, then
// BAM_SUM_TAIL or more, or everything up to the end of the file), taken in windows of `chunk` new bytes (0: one window).
// n_lanes = 1 and the candidate `start`, or the candidates 0 .. n_lanes - 1 when start = ~0.  Returns the windows.
inline uint64_t bam_share_summary_serial(const uint8_t *share, uint64_t n, uint64_t share_size, uint64_t start, uint32_t seg, uint64_t chunk,
                                         uint32_t n_lanes, uint64_t *x, uint64_t *cnt) {
    std::vector<BamLane> lanes(n_lanes);
    for (uint32_t i = 0; i < n_lanes; i++) lanes[i] = BamLane{start == ~0ull ? (uint64_t)i : start, 0, BAM_LANE_LIVE, 0};
    if (!chunk) chunk = n ? n : 1u;
    uint64_t base = 0, windows = 0;
    for (uint64_t have = n < chunk ? n : chunk;; have = n - have < chunk ? n : have + chunk) {  // the window: share[base, have)
        const uint64_t wn = have - base, lim = bam_sum_limit(wn, base, share_size, have == n);
        std::vector<uint16_t> tab(lim), tcnt(lim);  // (exactly sized: an index beyond the limit is an error a sanitizer sees)
        for (uint64_t lo = 0; lo < lim; lo += seg) bam_seg_exits_cnt_serial(share + base, wn, lo, lo + seg < lim ? lo + seg : lim, tab.data(), tcnt.data());
        for (BamLane &l : lanes) bam_lane_walk(share + base, wn, lim, tab.data(), tcnt.data(), seg, base, &l);
        base += lim;
        windows++;
        if (have == n) break;
    }
    for (uint32_t i = 0; i < n_lanes; i++) {
        x[i] = bam_lane_exit(lanes[i], share_size);
        cnt[i] = lanes[i].count;
    }
    return windows;
}

// ---- the plan of a sharded open: a pure function of what the ranks gathered ----------------------------------------------------
// head[6 r ..] = failed, whole BGZF, members M, header bytes H, the share's inflated size, candidates C_r; xn + xn_off[r]:
// X_r[0 .. C_r) then N_r[0 .. C_r).  Rank 0's one candidate is H.  plan[5 r ..] = bytes in front of the rank's first record
// (e_r - S_r), where its ownership ends relative to S_r (~0: at the end of the file), participating records in front of e_r,
// S_r, participating records in front of e_{r+1}.  Returns BAM_PLAN_*: 0, or why every rank leaves the file to rank 0.
enum {
    BAM_PLAN_OK = 0,
    BAM_PLAN_FAILED = 1,      // a rank failed in pass 1
    BAM_PLAN_DIFFER = 2,      // the ranks do not see the same file
    BAM_PLAN_NOT_BGZF = 3,
    BAM_PLAN_HEADER = 4,      // H >= S_1
    BAM_PLAN_ACROSS = 5,      // some x >= C_r
    BAM_PLAN_DEAD = 6,
    BAM_PLAN_CUT = 7,
    BAM_PLAN_NOT_AT_END = 8,
    BAM_PLAN_ODD = 9
};

inline int bam_shard_plan(uint32_t world, const uint64_t *head, const uint64_t *xn, const uint64_t *xn_off, uint64_t *plan) {
    if (!world) return BAM_PLAN_FAILED;
    for (uint32_t r = 0; r < world; r++)
        if (head[6u * r]) return BAM_PLAN_FAILED;
    for (uint32_t r = 1; r < world; r++)
        if (head[6u * r + 1u] != head[1] || head[6u * r + 2u] != head[2] || head[6u * r + 3u] != head[3]) return BAM_PLAN_DIFFER;
    if (!head[1]) return BAM_PLAN_NOT_BGZF;
    uint64_t total = 0;
    for (uint32_t r = 0; r < world; r++) total += head[6u * r + 4u];
    if (world > 1u && head[3] >= head[4]) return BAM_PLAN_HEADER;
    if (head[5] != 1u) return BAM_PLAN_FAILED;
    uint64_t S = 0, x = xn[xn_off[0]], count = xn[xn_off[0] + 1u];
    plan[0] = head[3];
    plan[2] = 0;
    plan[3] = 0;
    for (uint32_t r = 0;; r++) {
        // x: the exit of share r on the true chain, relative to S_{r+1}
        S += head[6u * r + 4u];
        if (x == BAM_SUM_DEAD) return BAM_PLAN_DEAD;
        if (x == BAM_SUM_CUT || (r + 1u < world && x > total - S)) return BAM_PLAN_CUT;  // (beyond the file from an inner share)
        plan[5u * r + 4u] = count;
        if (r + 1u == world) {
            plan[5u * r + 1u] = ~0ull;
            break;
        }
        const uint64_t C = head[6u * (r + 1u) + 5u];
        if (x >= C) return BAM_PLAN_ACROSS;
        plan[5u * r + 1u] = S + x - plan[5u * r + 3u];
        plan[5u * (r + 1u)] = x;
        plan[5u * (r + 1u) + 2u] = count;
        plan[5u * (r + 1u) + 3u] = S;
        const uint64_t *mine = xn + xn_off[r + 1u];
        count += mine[C + x];
        x = mine[x];
    }
    if (x != 0u) return BAM_PLAN_NOT_AT_END;
    if (count & 1u) return BAM_PLAN_ODD;
    return BAM_PLAN_OK;
}
