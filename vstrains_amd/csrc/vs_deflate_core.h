// The deflate encoder of vs_deflate.hip as ONE routine for the device and the host: text[0, n), n <= 0xFF00, becomes one
// whole BGZF member (18-byte header, one final deflate block, CRC32, ISIZE).  On the device a wavefront runs it for one
// member: `lane` = 0..63, `nl` = 64, the state in LDS.  On the host the same text runs with lane = 0, nl = 1 (every
// "for (i = lane; i < 64; i += nl)" then walks the 64 lane phases in order).  EVERY OUTPUT BYTE IS THE SAME FOR 1 LANE AND
// FOR 64: nothing below depends on which lane stores last.  Plain C++: a host compiler takes this header as it is.
//
// The matcher works on chunks of 64 text positions, a position per lane phase, in phases separated by DEF_SYNC:
//   A  w[l] = the 3 bytes at the position (a unique value where fewer than 3 are left), h[l] = their 11-bit hash;
//   B  two candidates: the table's entry for h[l] (a position in front of the chunk), and the NEAREST earlier position of
//      the SAME chunk with equal w (a 64-step compare against w[0..l)); lines of this text are 10 - 25 bytes, so most matches
//      lie inside the chunk and the table alone would find none of them.  A candidate further back than 32768 is refused,
//      and so is a match of length 3 further back than 4096 (it costs more than three literals).  Of two candidates the
//      LONGER match wins, the NEARER one if they are equally long.  A match is 3 .. 258 bytes and ends inside the text;
//   C  greedy parse: from the position where the last token ended, a match of 3 or more is taken, else a literal; the
//      walk is wave-uniform (every lane reads the same LDS word);
//   D  the table takes the chunk's positions: of several positions with one hash the LARGEST wins -- a lane phase stores
//      only if no later phase of the chunk has its hash -- so no two stores ever meet in one bucket.
// The text is tokenised TWICE: pass 1 fills the literal/length and distance histograms, the sizes of the stored, fixed and
// dynamic form follow from the histograms alone, the smallest is chosen (a tie goes to stored, then fixed), and pass 2,
// identical by determinism, emits.  No token is kept anywhere.  A token's bits are known before they are written: the
// bit offsets of a chunk's tokens are a prefix sum over the lane phases, the tokens are ORed into a 416-byte LDS image,
// whole bytes go to global memory and the partial byte is carried.
//
// Bounds (the contract, not error handling):
//   text     every read tests its index against n; a match length is capped by n - position before the first compare;
//   tables   the hash is masked to the table; symbol indexes come from def_len_sym / def_dist_sym, whose ranges are
//            257..285 and 0..29 for the lengths 3..258 and distances 1..32768 that the matcher lets through;
//   output   the member's size is known before its first byte is written and tested against cap there; every store tests
//            its index against that size again.  Nothing is written outside out[0, cap).
#ifndef VS_DEFLATE_CORE_H
#define VS_DEFLATE_CORE_H
#include <stdint.h>

#include "vs_inflate_core.h"  // INF_FN, INF_UNI, INF_SYNC, and the CRC32 by slices (inf_crc_table, inf_crc_part)

#define DEF_SYNC() INF_SYNC()
#if defined(__HIP_DEVICE_COMPILE__)
// lanes of one wavefront add to / OR into one LDS word: integer add and OR commute, the sum does not depend on the order
#define DEF_ADD(p, v) ((void)__hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT))
#define DEF_OR(p, v) ((void)__hip_atomic_fetch_or((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT))
#else
#define DEF_ADD(p, v) ((void)(*(p) += (v)))
#define DEF_OR(p, v) ((void)(*(p) |= (v)))
#endif

enum {
    DEF_OK = 0,
    DEF_E_ARG = 1,    // n > DEF_MAX_TEXT
    DEF_E_CAP = 2,    // the member does not fit into cap bytes
    DEF_E_STATE = 3   // pass 2 did not emit the bits pass 1 counted (the text changed between the passes)
};
enum { DEF_KIND_STORED = 0, DEF_KIND_FIXED = 1, DEF_KIND_DYNAMIC = 2 };

#define DEF_MAX_TEXT 0xFF00u    // bgzip's cut: a stored block of it, with header and trailer, stays below 65536
#define DEF_MEMBER_EXTRA 31u    // 18 header + 1 block header + 4 LEN/NLEN + 8 trailer: the stored form is n + 31 bytes
#define DEF_MIN_MATCH 3u
#define DEF_MAX_MATCH 258u
#define DEF_MAX_DIST 32768u
#define DEF_FAR_3 4096u         // a match of length 3 is taken up to this distance
#define DEF_HASH_BITS 11u
#define DEF_CHUNK 64u
#define DEF_BUF_WORDS 104u      // 64 tokens of at most 48 bits + a carried partial byte = 3079 bits
#define DEF_NLIT 286u
#define DEF_NDIST 30u
#define DEF_CNT_WORDS 33u       // counts per code length 0 .. 32 of the code-length builder (and 16 + 16 words of def_codes)

struct DefCore {  // LDS on the device (about 9.6 KB per wavefront)
    uint16_t head[1u << DEF_HASH_BITS];  // position + 1 of the latest text position with this hash, 0: none
    uint32_t lfreq[288], dfreq[32], cfreq[19];
    uint16_t lcode[288], dcode[32], ccode[19];  // bit-reversed canonical codes
    uint8_t llen[288], dlen[32], clen[19];
    uint8_t lens[320];                   // the code-length sequence of the dynamic header: llen[0, hlit) then dlen[0, hdist)
    uint32_t work[288];                  // code-length builder: sorted weights, then depths
    uint16_t order[288];                 // code-length builder: symbols by (weight, symbol)
    uint32_t cnt[DEF_CNT_WORDS];         // code-length builder: codes per length
    uint32_t w[DEF_CHUNK];               // per lane phase: the 3 bytes at the position
    uint16_t h[DEF_CHUNK];               // their hash
    uint16_t mlen[DEF_CHUNK], mdist[DEF_CHUNK];
    uint8_t tbits[DEF_CHUNK];            // bits of the token that starts here, 0: none starts here
    uint32_t buf[DEF_BUF_WORDS];         // the bit image of a chunk: byte i is bits 8 (i & 3) .. of word i >> 2
    uint32_t sizes[5];                   // lane 0's verdict: bits of the fixed and of the dynamic form, hlit, hdist, hclen
};
struct DefState {
    union {
        DefCore d;
        InfState crc;  // the CRC32 table, needed only before the encoder starts
    };
};

struct DefOut {
    uint32_t bits;  // bits in buf
    uint32_t pos;   // bytes of `out` written
    uint32_t end;   // one past the last byte this member may write
};

// ---- symbols -----------------------------------------------------------------------------------------------------------
INF_FN uint32_t def_log2(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); }  // x > 0

// length 3..258 -> symbol 257..285, *eb extra bits holding *ev
INF_FN uint32_t def_len_sym(uint32_t len, uint32_t *eb, uint32_t *ev) {
    const uint32_t l = len - 3u;
    *eb = 0, *ev = 0;
    if (len >= 258u) return 285u;
    if (l < 8u) return 257u + l;
    const uint32_t e = def_log2(l) - 2u;
    *eb = e, *ev = l & ((1u << e) - 1u);
    return 261u + 4u * e + ((l >> e) & 3u);
}
INF_FN uint32_t def_len_extra(uint32_t sym) {  // extra bits of length symbol 257..285
    const uint32_t s = sym - 257u;
    return s < 8u || s >= 28u ? 0u : (s >> 2) - 1u;
}
// distance 1..32768 -> symbol 0..29
INF_FN uint32_t def_dist_sym(uint32_t dist, uint32_t *eb, uint32_t *ev) {
    const uint32_t d = dist - 1u;
    *eb = 0, *ev = 0;
    if (d < 4u) return d;
    const uint32_t e = def_log2(d) - 1u;
    *eb = e, *ev = d & ((1u << e) - 1u);
    return 2u * e + 2u + ((d >> e) & 1u);
}
INF_FN uint32_t def_dist_extra(uint32_t sym) { return sym < 4u ? 0u : (sym >> 1) - 1u; }
INF_FN uint32_t def_fixed_len(uint32_t s) { return s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : 8u; }

// ---- code lengths (one lane, serial) -------------------------------------------------------------------------------------
// freq[0, nsym) -> len[0, nsym), every length <= maxbits, nsym <= 288.  Fewer than two symbols in use: symbol 0 (and 1)
// join with weight 1, as zlib's deflate does, so the code always has two or more symbols and is complete (Kraft sum 1);
// zlib and inf_build accept every code this returns.  Symbols are ordered by (weight, symbol), Huffman depths come from
// Moffat and Katajainen's in-place algorithm, and a code deeper than maxbits is cut the way miniz does it: on the counts
// per length, one unit of the Kraft sum at a time, which ends exactly at 1.  The longest lengths go to the lightest symbols.
INF_FN void def_code_lengths(const uint32_t *freq, uint32_t nsym, uint32_t maxbits, uint8_t *len, uint32_t *work, uint16_t *order, uint32_t *cnt) {
    uint32_t m = 0;
    for (uint32_t s = 0; s < nsym; s++) {
        len[s] = 0;
        if (freq[s]) m++;
    }
    const uint32_t force0 = m < 2u && !freq[0] ? 1u : 0u, force1 = (m + force0) < 2u ? 1u : 0u;  // (nsym >= 2 always)
    m = 0;
    for (uint32_t s = 0; s < nsym && m < 288u; s++) {  // insertion sort by (weight, symbol): symbols arrive in order
        uint32_t f = freq[s];
        if (!f && ((s == 0u && force0) || (s == 1u && force1))) f = 1u;
        if (!f) continue;
        uint32_t at = m;
        while (at > 0u && work[at - 1u] > f) {
            work[at] = work[at - 1u];
            order[at] = order[at - 1u];
            at--;
        }
        work[at] = f;
        order[at] = (uint16_t)s;
        m++;
    }
    if (m < 2u) return;  // (cannot happen: two symbols are forced)
    // Moffat / Katajainen: work[0, m) ascending weights -> depths, deepest first
    if (m == 2u) {
        work[0] = work[1] = 1u;
    } else {
        work[0] += work[1];
        uint32_t root = 0, leaf = 2;
        for (uint32_t next = 1; next < m - 1u; next++) {
            if (leaf >= m || work[root] < work[leaf]) {
                work[next] = work[root];
                work[root++] = next;
            } else {
                work[next] = work[leaf++];
            }
            if (leaf >= m || (root < next && work[root] < work[leaf])) {
                work[next] += work[root];
                work[root++] = next;
            } else {
                work[next] += work[leaf++];
            }
        }
        work[m - 2u] = 0;
        for (int32_t next = (int32_t)m - 3; next >= 0; next--) work[next] = work[work[next]] + 1u;
        int32_t avbl = 1, used = 0, root2 = (int32_t)m - 2, next = (int32_t)m - 1;
        uint32_t dpth = 0;
        while (avbl > 0) {
            while (root2 >= 0 && work[root2] == dpth) {
                used++;
                root2--;
            }
            while (avbl > used) {
                work[next--] = dpth;
                avbl--;
            }
            avbl = 2 * used;
            dpth++;
            used = 0;
        }
    }
    // counts per length, everything deeper than maxbits at maxbits, then the Kraft sum brought back to 1
    for (uint32_t l = 0; l <= 32u; l++) cnt[l] = 0;  // (cnt: DEF_CNT_WORDS words of the caller's, LDS on the device)
    for (uint32_t i = 0; i < m; i++) cnt[work[i] < maxbits ? work[i] : maxbits]++;
    uint32_t total = 0;
    for (uint32_t l = maxbits; l > 0u; l--) total += cnt[l] << (maxbits - l);
    while (total > (1u << maxbits)) {
        cnt[maxbits]--;
        for (uint32_t l = maxbits - 1u; l > 0u; l--)
            if (cnt[l]) {
                cnt[l]--;
                cnt[l + 1u] += 2u;
                break;
            }
        total--;
    }
    uint32_t at = 0;
    for (uint32_t l = maxbits; l > 0u; l--)
        for (uint32_t c = cnt[l]; c > 0u && at < m; c--) len[order[at++]] = (uint8_t)l;
}

// canonical codes of len[0, nsym), bit-reversed for an LSB-first bit stream
INF_FN void def_codes(const uint8_t *len, uint32_t nsym, uint16_t *code, uint32_t *cnt) {
    uint32_t *next = cnt + 16;
    for (uint32_t l = 0; l < 16u; l++) cnt[l] = 0;
    for (uint32_t s = 0; s < nsym; s++) cnt[len[s] & 15u]++;
    cnt[0] = 0;
    uint32_t c = 0;
    next[0] = 0;
    for (uint32_t l = 1; l < 16u; l++) {
        c = (c + cnt[l - 1u]) << 1;
        next[l] = c;
    }
    for (uint32_t s = 0; s < nsym; s++) {
        const uint32_t l = len[s] & 15u;
        code[s] = l ? (uint16_t)inf_rev(next[l]++, l) : (uint16_t)0;
    }
}

// ---- bit output ----------------------------------------------------------------------------------------------------------
// v (at most 48 bits of it set) at bit `off` of the image; off + 48 <= 32 * DEF_BUF_WORDS is the caller's, and tested again
INF_FN void def_or_bits(DefCore *S, uint32_t off, uint64_t v) {
    const uint32_t wi = off >> 5, sh = off & 31u;
    const uint64_t lo = (v & 0xFFFFFFFFull) << sh, hi = (v >> 32) << sh;
    const uint32_t w0 = (uint32_t)lo, w1 = (uint32_t)(lo >> 32) | (uint32_t)hi, w2 = (uint32_t)(hi >> 32);
    if (w0 && wi < DEF_BUF_WORDS) DEF_OR(&S->buf[wi], w0);
    if (w1 && wi + 1u < DEF_BUF_WORDS) DEF_OR(&S->buf[wi + 1u], w1);
    if (w2 && wi + 2u < DEF_BUF_WORDS) DEF_OR(&S->buf[wi + 2u], w2);
}

// the image's whole bytes to out, the partial byte to the image's front
INF_FN void def_flush(DefCore *S, DefOut &o, uint8_t *out, uint32_t lane, uint32_t nl, bool all) {
    DEF_SYNC();
    const uint32_t nb = all ? (o.bits + 7u) >> 3 : o.bits >> 3;
    for (uint32_t i = lane; i < nb; i += nl)
        if (o.pos + i < o.end) out[o.pos + i] = (uint8_t)(S->buf[i >> 2] >> (8u * (i & 3u)));
    const uint32_t part = all ? 0u : (INF_UNI(S->buf[(nb >> 2) < DEF_BUF_WORDS ? nb >> 2 : 0u]) >> (8u * (nb & 3u))) & ((1u << (o.bits & 7u)) - 1u);
    DEF_SYNC();
    for (uint32_t i = lane; i < DEF_BUF_WORDS; i += nl) S->buf[i] = i ? 0u : part;
    DEF_SYNC();
    o.pos += nb;
    o.bits = all ? 0u : o.bits & 7u;
}

// wave-uniform bits (a header field, the end-of-block code): lane 0 stores them
INF_FN void def_put(DefCore *S, DefOut &o, uint8_t *out, uint32_t v, uint32_t nbits, uint32_t lane, uint32_t nl) {
    if (o.bits + nbits > 32u * DEF_BUF_WORDS - 64u) def_flush(S, o, out, lane, nl, false);
    if (lane == 0) def_or_bits(S, o.bits, (uint64_t)v);
    o.bits += nbits;
}

// ---- the matcher: one chunk of 64 positions ------------------------------------------------------------------------------
// Phases A .. D of the head comment for the chunk at c0.  carry: the position where the next token starts (wave-uniform).
// Afterwards tbits[l] != 0 marks a token start (its value is set by the caller's pass), mlen / mdist hold its match.
INF_FN void def_chunk(DefCore *S, const uint8_t *text, uint32_t n, uint32_t c0, uint32_t &carry, uint32_t lane, uint32_t nl) {
    DEF_SYNC();
    for (uint32_t l = lane; l < DEF_CHUNK; l += nl) {  // A
        const uint32_t p = c0 + l;
        uint32_t w = 0xFF000000u | l, h = 0xFFFFu;  // (a 3-byte value never has the top byte set)
        if (p < n && n - p >= 3u) {
            w = (uint32_t)text[p] | ((uint32_t)text[p + 1u] << 8) | ((uint32_t)text[p + 2u] << 16);
            h = ((w * 2654435761u) >> (32u - DEF_HASH_BITS)) & ((1u << DEF_HASH_BITS) - 1u);
        }
        S->w[l] = w;
        S->h[l] = (uint16_t)h;
        S->tbits[l] = 0;
        S->mlen[l] = 0;
        S->mdist[l] = 0;
    }
    DEF_SYNC();
    const uint32_t stop = c0 + DEF_CHUNK < n ? c0 + DEF_CHUNK : n;
    if (carry < stop) {  // (a chunk that a match covers whole is not searched)
        for (uint32_t l = lane; l < DEF_CHUNK; l += nl) {  // B
            const uint32_t p = c0 + l, w = S->w[l], h = S->h[l];
            if (p < carry || h == 0xFFFFu) continue;
            const uint32_t limit = n - p < DEF_MAX_MATCH ? n - p : DEF_MAX_MATCH;
            uint32_t best_len = 0, best_dist = 0;
            uint32_t near = DEF_CHUNK;
            for (uint32_t k = 0; k < l; k++)
                if (S->w[k] == w) near = k;  // the nearest earlier position of the chunk with these 3 bytes
            if (near < DEF_CHUNK) {
                const uint32_t q = c0 + near;
                uint32_t len = 3;
                while (len < limit && text[q + len] == text[p + len]) len++;
                best_len = len, best_dist = p - q;
            }
            const uint32_t e = S->head[h];
            if (e != 0u && e - 1u < c0) {
                const uint32_t q = e - 1u, dist = p - q;
                if (dist <= DEF_MAX_DIST) {
                    uint32_t len = 0;
                    while (len < limit && text[q + len] == text[p + len]) len++;
                    if (len == 3u && dist > DEF_FAR_3) len = 0;
                    if (len >= DEF_MIN_MATCH && len > best_len) best_len = len, best_dist = dist;  // (equally long: the nearer stays)
                }
            }
            S->mlen[l] = (uint16_t)best_len;
            S->mdist[l] = (uint16_t)(best_dist & 0xFFFFu);  // (32768 fits)
        }
    }
    DEF_SYNC();
    uint32_t p = carry;  // C
    while (p < stop) {
        const uint32_t i = (p - c0) & (DEF_CHUNK - 1u);
        const uint32_t len = INF_UNI(S->mlen[i]);
        if (lane == 0) S->tbits[i] = 1;
        p += len >= DEF_MIN_MATCH ? len : 1u;
    }
    if (p > carry) carry = p;
    for (uint32_t l = lane; l < DEF_CHUNK; l += nl) {  // D
        const uint32_t h = S->h[l];
        if (h == 0xFFFFu) continue;
        bool last = true;
        for (uint32_t k = l + 1u; k < DEF_CHUNK; k++)
            if (S->h[k] == h) last = false;
        if (last) S->head[h & ((1u << DEF_HASH_BITS) - 1u)] = (uint16_t)(c0 + l + 1u);
    }
    DEF_SYNC();
}

// ---- the dynamic header ----------------------------------------------------------------------------------------------------
// The run-length coding of lens[0, total) (RFC 1951 3.2.7) walked once: emit == false adds to cfreq (lane 0), emit == true
// puts the codes.  Every value is wave-uniform.
INF_FN void def_rle(DefCore *S, uint32_t total, bool emit, DefOut &o, uint8_t *out, uint32_t lane, uint32_t nl) {
    uint32_t i = 0, prev = 0xFFu;
    while (i < total) {
        const uint32_t v = INF_UNI(S->lens[i]);
        uint32_t run = 1;
        while (i + run < total && INF_UNI(S->lens[i + run]) == v) run++;
        i += run;
        while (run) {
            uint32_t sym, take, eb = 0, ev = 0;
            if (v == 0u && run >= 11u) sym = 18u, take = run < 138u ? run : 138u, eb = 7u, ev = take - 11u;
            else if (v == 0u && run >= 3u) sym = 17u, take = run, eb = 3u, ev = take - 3u;
            else if (v != 0u && prev == v && run >= 3u) sym = 16u, take = run < 6u ? run : 6u, eb = 2u, ev = take - 3u;
            else sym = v, take = 1u;
            if (!emit) {
                if (lane == 0) S->cfreq[sym]++;
            } else {
                def_put(S, o, out, (uint32_t)INF_UNI(S->ccode[sym]) | (ev << INF_UNI(S->clen[sym])), INF_UNI(S->clen[sym]) + eb, lane, nl);
            }
            run -= take;
            prev = v;
        }
    }
}

INF_FN uint32_t def_cl_order(uint32_t i) {  // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
    return i < 12u ? (uint32_t)((0x022CAA324E804A30ull >> (5u * i)) & 31u) : (uint32_t)((0x3C2E1346Cull >> (5u * (i - 12u))) & 31u);
}

// ---- one member ------------------------------------------------------------------------------------------------------------
// text[0, n) -> out[0, *size), *size <= n + 31, *kind = DEF_KIND_*.  Returns DEF_*: DEF_E_CAP, with nothing written, when the
// member chosen is larger than cap (cap = n + 31 always suffices).
INF_FN uint32_t def_member(DefState *St, const uint8_t *text, uint32_t n, uint8_t *out, uint32_t cap, uint32_t lane, uint32_t nl, uint32_t *size,
                           uint32_t *kind) {
    *size = 0, *kind = DEF_KIND_STORED;
    if (n > DEF_MAX_TEXT) return DEF_E_ARG;
    DefCore *S = &St->d;
    // CRC32 of the text: 64 slices, combined (the table lies where the encoder's state will)
    inf_crc_table(&St->crc, lane, nl);
    uint32_t crc = 0;
    for (uint32_t part = lane; part < INF_CRC_PARTS; part += nl) crc ^= inf_crc_part(&St->crc, text, n, part);
    DEF_SYNC();
    for (uint32_t l = lane; l < DEF_CHUNK; l += nl) S->w[l] = l == lane ? crc : 0u;
    DEF_SYNC();
    crc = 0;
    for (uint32_t l = 0; l < DEF_CHUNK; l++) crc ^= INF_UNI(S->w[l]);
    DEF_SYNC();
    // pass 1: histograms
    for (uint32_t i = lane; i < (1u << DEF_HASH_BITS); i += nl) S->head[i] = 0;
    for (uint32_t i = lane; i < 288u; i += nl) S->lfreq[i] = i == 256u ? 1u : 0u;
    for (uint32_t i = lane; i < 32u; i += nl) S->dfreq[i] = 0;
    for (uint32_t i = lane; i < 19u; i += nl) S->cfreq[i] = 0;
    uint32_t carry = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += DEF_CHUNK) {
        def_chunk(S, text, n, c0, carry, lane, nl);
        for (uint32_t l = lane; l < DEF_CHUNK; l += nl) {
            if (!S->tbits[l]) continue;
            const uint32_t len = S->mlen[l];
            uint32_t eb, ev;
            if (len >= DEF_MIN_MATCH) {
                DEF_ADD(&S->lfreq[def_len_sym(len, &eb, &ev)], 1u);
                DEF_ADD(&S->dfreq[def_dist_sym(S->mdist[l] ? S->mdist[l] : 1u, &eb, &ev) & 31u], 1u);
            } else {
                DEF_ADD(&S->lfreq[c0 + l < n ? text[c0 + l] : 0u], 1u);
            }
        }
    }
    DEF_SYNC();
    // the three sizes (lane 0, serial: a member of this text uses a few dozen symbols)
    if (lane == 0) {
        def_code_lengths(S->lfreq, DEF_NLIT, 15u, S->llen, S->work, S->order, S->cnt);
        def_code_lengths(S->dfreq, DEF_NDIST, 15u, S->dlen, S->work, S->order, S->cnt);
        S->llen[286] = S->llen[287] = S->dlen[30] = S->dlen[31] = 0;
        uint32_t hlit = DEF_NLIT, hdist = DEF_NDIST;
        while (hlit > 257u && !S->llen[hlit - 1u]) hlit--;
        while (hdist > 1u && !S->dlen[hdist - 1u]) hdist--;
        for (uint32_t i = 0; i < hlit; i++) S->lens[i] = S->llen[i];
        for (uint32_t i = 0; i < hdist; i++) S->lens[hlit + i] = S->dlen[i];
        S->sizes[2] = hlit, S->sizes[3] = hdist;
    }
    DEF_SYNC();
    const uint32_t hlit = INF_UNI(S->sizes[2]), hdist = INF_UNI(S->sizes[3]);
    DefOut o = {0u, 0u, 0u};
    def_rle(S, hlit + hdist, false, o, out, lane, nl);
    DEF_SYNC();
    if (lane == 0) {
        def_code_lengths(S->cfreq, 19u, 7u, S->clen, S->work, S->order, S->cnt);
        def_codes(S->clen, 19u, S->ccode, S->cnt);
        uint32_t hclen = 19u;
        while (hclen > 4u && !S->clen[def_cl_order(hclen - 1u)]) hclen--;
        uint32_t fixed = 3u, dyn = 3u + 14u + 3u * hclen;
        for (uint32_t c = 0; c < 19u; c++) dyn += S->cfreq[c] * (S->clen[c] + (c == 16u ? 2u : c == 17u ? 3u : c == 18u ? 7u : 0u));
        for (uint32_t s = 0; s < DEF_NLIT; s++) {
            const uint32_t f = S->lfreq[s], x = s > 256u ? def_len_extra(s) : 0u;
            fixed += f * (def_fixed_len(s) + x);
            dyn += f * (S->llen[s] + x);
        }
        for (uint32_t s = 0; s < DEF_NDIST; s++) {
            const uint32_t f = S->dfreq[s], x = def_dist_extra(s);
            fixed += f * (5u + x);
            dyn += f * (S->dlen[s] + x);
        }
        S->sizes[0] = fixed, S->sizes[1] = dyn;
        S->sizes[4] = hclen;
    }
    DEF_SYNC();
    const uint32_t fixed_bits = INF_UNI(S->sizes[0]), dyn_bits = INF_UNI(S->sizes[1]), hclen = INF_UNI(S->sizes[4]);
    const uint32_t stored_bytes = n + 5u, fixed_bytes = (fixed_bits + 7u) >> 3, dyn_bytes = (dyn_bits + 7u) >> 3;
    uint32_t k = DEF_KIND_STORED, pay = stored_bytes;
    if (fixed_bytes < pay) k = DEF_KIND_FIXED, pay = fixed_bytes;
    if (dyn_bytes < pay) k = DEF_KIND_DYNAMIC, pay = dyn_bytes;
    const uint32_t total = 18u + pay + 8u;  // <= n + 31 <= 65311
    if (total > cap) return DEF_E_CAP;
    o.pos = 18u, o.end = 18u + pay;
    if (k == DEF_KIND_STORED) {
        for (uint32_t i = lane; i < 5u; i += nl) {
            const uint32_t v = i == 0u ? 1u : i == 1u ? n & 255u : i == 2u ? n >> 8 : i == 3u ? (~n) & 255u : ((~n) >> 8) & 255u;
            out[18u + i] = (uint8_t)v;
        }
        for (uint32_t i = lane; i < n; i += nl)
            if (23u + i < o.end) out[23u + i] = text[i];
        o.pos = o.end;
    } else {
        DEF_SYNC();
        for (uint32_t i = lane; i < DEF_BUF_WORDS; i += nl) S->buf[i] = 0;
        for (uint32_t i = lane; i < (1u << DEF_HASH_BITS); i += nl) S->head[i] = 0;
        if (k == DEF_KIND_FIXED) {
            for (uint32_t i = lane; i < 288u; i += nl) S->llen[i] = (uint8_t)def_fixed_len(i);
            for (uint32_t i = lane; i < 32u; i += nl) S->dlen[i] = 5;
        }
        DEF_SYNC();
        if (lane == 0) {
            def_codes(S->llen, 288u, S->lcode, S->cnt);
            def_codes(S->dlen, 32u, S->dcode, S->cnt);
        }
        DEF_SYNC();
        def_put(S, o, out, 1u | (k << 1), 3u, lane, nl);
        if (k == DEF_KIND_DYNAMIC) {
            def_put(S, o, out, (hlit - 257u) | ((hdist - 1u) << 5) | ((hclen - 4u) << 10), 14u, lane, nl);
            for (uint32_t i = 0; i < hclen; i++) def_put(S, o, out, INF_UNI(S->clen[def_cl_order(i)]), 3u, lane, nl);
            def_rle(S, hlit + hdist, true, o, out, lane, nl);
        }
        // pass 2: the same tokens, emitted
        carry = 0;
        for (uint32_t c0 = 0; c0 < n; c0 += DEF_CHUNK) {
            def_flush(S, o, out, lane, nl, false);
            def_chunk(S, text, n, c0, carry, lane, nl);
            for (uint32_t l = lane; l < DEF_CHUNK; l += nl) {
                if (!S->tbits[l]) continue;
                const uint32_t len = S->mlen[l];
                uint32_t bits;
                if (len >= DEF_MIN_MATCH) {
                    uint32_t eb, ev, db, dv;
                    const uint32_t ls = def_len_sym(len, &eb, &ev), ds = def_dist_sym(S->mdist[l] ? S->mdist[l] : 1u, &db, &dv) & 31u;
                    bits = S->llen[ls] + eb + S->dlen[ds] + db;
                } else {
                    bits = S->llen[c0 + l < n ? text[c0 + l] : 0u];
                }
                S->tbits[l] = (uint8_t)bits;  // (a code in use has 1 .. 15 bits: never 0)
            }
            DEF_SYNC();
            uint32_t sum = 0;
            for (uint32_t l = lane; l < DEF_CHUNK; l += nl) {
                uint32_t before = 0;
                for (uint32_t j = 0; j < l; j++) before += S->tbits[j];
                if (!S->tbits[l]) continue;
                const uint32_t len = S->mlen[l];
                uint64_t v;
                uint32_t bits;
                if (len >= DEF_MIN_MATCH) {
                    uint32_t eb, ev, db, dv;
                    const uint32_t ls = def_len_sym(len, &eb, &ev), ds = def_dist_sym(S->mdist[l] ? S->mdist[l] : 1u, &db, &dv) & 31u;
                    v = (uint64_t)S->lcode[ls];
                    bits = S->llen[ls];
                    v |= (uint64_t)ev << bits;
                    bits += eb;
                    v |= (uint64_t)S->dcode[ds] << bits;
                    bits += S->dlen[ds];
                    v |= (uint64_t)dv << bits;
                    bits += db;
                } else {
                    const uint32_t b = c0 + l < n ? text[c0 + l] : 0u;
                    v = (uint64_t)S->lcode[b];
                    bits = S->llen[b];
                }
                def_or_bits(S, o.bits + before, v);
            }
            DEF_SYNC();
            for (uint32_t j = 0; j < DEF_CHUNK; j++) sum += INF_UNI(S->tbits[j]);
            o.bits += sum;
        }
        def_flush(S, o, out, lane, nl, false);
        def_put(S, o, out, INF_UNI(S->lcode[256]), INF_UNI(S->llen[256]), lane, nl);
        def_flush(S, o, out, lane, nl, true);
    }
    if (o.pos != 18u + pay) return DEF_E_STATE;
    for (uint32_t i = lane; i < 26u; i += nl) {
        const uint32_t bs = total - 1u;
        uint32_t v;
        switch (i) {
            case 0: v = 0x1f; break;
            case 1: v = 0x8b; break;
            case 2: v = 8; break;
            case 3: v = 4; break;
            case 9: v = 0xff; break;
            case 10: v = 6; break;
            case 12: v = 0x42; break;
            case 13: v = 0x43; break;
            case 14: v = 2; break;
            case 16: v = bs & 255u; break;
            case 17: v = bs >> 8; break;
            default: v = i < 18u ? 0u : i < 22u ? (crc >> (8u * (i - 18u))) & 255u : (n >> (8u * (i - 22u))) & 255u;
        }
        out[i < 18u ? i : 18u + pay + (i - 18u)] = (uint8_t)v;
    }
    DEF_SYNC();
    *size = total, *kind = k;
    return DEF_OK;
}

#endif  // VS_DEFLATE_CORE_H
