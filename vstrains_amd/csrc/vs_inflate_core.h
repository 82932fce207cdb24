// The deflate decoder of vs_inflate.hip as ONE routine for the device and the host (RFC 1951: stored, fixed and dynamic
// blocks).  On the device a wavefront runs it for one member: `lane` = 0..63, `nl` = 64, the state in LDS.  On the host
// the same text runs with lane = 0, nl = 1 (vs_inflate_host), so that every bound below can be exercised -- corrupt
// members included -- before a kernel is launched.  Plain C++: a host compiler takes this header as it is.
//
// Every value that steers control flow is wave-uniform: it comes from the payload through INF_UNI (readfirstlane on the
// device), so all lanes take the same branches and the lane-strided loops (table fill, match copy, window load) are the
// only divergent code.
//
// Bounds (the contract, not error handling):
//   payload   bytes enter the bit buffer only from [0, len): the window load and the stored copy test every index against
//             len, and a code or field that needs more bits than are buffered ends the member (INF_E_INPUT);
//   output    a literal, a match and a stored copy test opos (+ length) against isize BEFORE the first byte is written;
//   matches   dist <= opos is tested before the copy: a source index never lies before the member's own first byte;
//   tables    fast-table indexes are masked to the table, symbol-array indexes are tested against the array, code lengths
//             are masked to 0..15, the code-length loop runs to hlit + hdist <= 286 + 30 and tests every repeat against it,
//             the 19 code-length codes go through a fixed permutation of 0..18.
#ifndef VS_INFLATE_CORE_H
#define VS_INFLATE_CORE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define INF_FN __host__ __device__ inline
#else
#define INF_FN inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define INF_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
// Lanes of one wavefront hand bytes to each other through LDS and through the member's output in global memory.  A
// wavefront's LDS and vector-memory instructions are issued and performed in program order for all of its lanes (the
// AMDGPU memory model needs no instruction for a fence at wavefront scope for that reason), so what is left to pin is the
// compiler's order: a release and an acquire fence at wavefront scope around a scheduling barrier.
#define INF_SYNC()                                              \
    do {                                                        \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                        \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
    } while (0)
#else
#define INF_UNI(x) ((uint32_t)(x))
#define INF_SYNC() \
    do {           \
    } while (0)
#endif

// the status word of a member: 0, or the first thing wrong
enum {
    INF_OK = 0,
    INF_E_BTYPE = 1,       // block type 3
    INF_E_STORED = 2,      // LEN != ~NLEN
    INF_E_OVERSUB = 3,     // over-subscribed code lengths
    INF_E_INCOMPLETE = 4,  // incomplete code lengths (other than the single 1-bit code zlib accepts)
    INF_E_LITLEN = 5,      // invalid literal/length symbol
    INF_E_DIST = 6,        // invalid distance symbol
    INF_E_FAR = 7,         // distance further back than the member's own output
    INF_E_INPUT = 8,       // payload exhausted
    INF_E_OUT_OVER = 9,    // output beyond ISIZE
    INF_E_OUT_SHORT = 10,  // output short of ISIZE
    INF_E_CRC = 11,        // CRC32 mismatch
    INF_E_LENGTHS = 12,    // bad code-length section: too many symbols, a repeat with nothing before it or past the end,
                           // no end-of-block code
    INF_E_TRAILING = 13,   // payload bytes left behind the final block (the trailer is then not where BSIZE puts it)
    INF_E_ARG = 14         // the member's descriptor does not lie inside the buffers
};

#define INF_LIT_BITS 10u
#define INF_DIST_BITS 8u
#define INF_CL_BITS 7u
#define INF_IN_BYTES 512u
#define INF_MAX_ISIZE 65536u
#define INF_CRC_PARTS 64u

enum { INF_KIND_CODES = 0, INF_KIND_LIT = 1, INF_KIND_DIST = 2 };
#define INF_SYM_INVALID 0xFFFFu
#define INF_SYM_INPUT 0xFFFEu

struct InfState {  // LDS on the device (about 5.5 KB per wavefront)
    uint16_t lit_fast[1u << INF_LIT_BITS];    // (symbol << 4) | length for codes of up to INF_LIT_BITS bits, 0: not here
    uint16_t dist_fast[1u << INF_DIST_BITS];  // also the code-length code's (7 bits)
    uint16_t lit_sym[288], dist_sym[32];      // symbols in canonical order
    uint16_t lit_cnt[16], dist_cnt[16];       // codes per length
    uint16_t lit_off[16], dist_off[16];       // first position of a length in *_sym
    uint16_t lit_first[16], dist_first[16];   // first code of a length
    uint16_t run[16];
    uint8_t lens[320];  // literal/length then distance code lengths
    uint8_t cl[32];     // code-length code lengths
    uint32_t crc_tab[256];
    uint8_t in[INF_IN_BYTES];  // window of the payload the bit buffer is filled from
};

struct InfBits {
    uint64_t buf;
    uint32_t cnt;  // bits in buf
    uint32_t pos;  // next payload byte to enter buf
    uint32_t win;  // payload offset of in[0]
};

INF_FN void inf_load_window(InfState *S, const uint8_t *pay, uint32_t len, InfBits &b, uint32_t lane, uint32_t nl) {
    INF_SYNC();
    for (uint32_t i = lane; i < INF_IN_BYTES; i += nl) {
        const uint32_t at = b.pos + i;
        S->in[i] = (at >= b.pos && at < len) ? pay[at] : (uint8_t)0;
    }
    b.win = b.pos;
    INF_SYNC();
}

// whole bytes into the bit buffer while they fit and the payload has some
INF_FN void inf_refill(InfState *S, const uint8_t *pay, uint32_t len, InfBits &b, uint32_t lane, uint32_t nl) {
    while (b.cnt <= 56u && b.pos < len) {
        if (b.pos - b.win >= INF_IN_BYTES) inf_load_window(S, pay, len, b, lane, nl);  // (also pos < win: a stored block stepped back)
        b.buf |= (uint64_t)INF_UNI(S->in[(b.pos - b.win) & (INF_IN_BYTES - 1u)]) << b.cnt;
        b.cnt += 8u;
        b.pos++;
    }
}

INF_FN void inf_drop(InfBits &b, uint32_t n) {
    b.buf >>= n;
    b.cnt -= n;
}

INF_FN uint32_t inf_rev(uint32_t code, uint32_t len) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < len; i++) r |= ((code >> i) & 1u) << (len - 1u - i);
    return r;
}

// Canonical Huffman tables of lens[0, nsym) (nsym <= sym_cap).  Lane 0 counts and sorts (a few hundred LDS operations),
// every lane judges the counts, the lanes fill the fast table.
INF_FN uint32_t inf_build(InfState *S, const uint8_t *lens, uint32_t nsym, uint16_t *fast, uint32_t fast_bits, uint16_t *sym,
                          uint32_t sym_cap, uint16_t *cnt, uint16_t *off, uint16_t *first, uint32_t kind, uint32_t lane, uint32_t nl) {
    if (nsym > sym_cap) return INF_E_LENGTHS;
    INF_SYNC();
    if (lane == 0) {
        for (uint32_t l = 0; l < 16; l++) cnt[l] = 0;
        for (uint32_t s = 0; s < nsym; s++) cnt[lens[s] & 15u]++;
        uint32_t o = 0, code = 0;
        off[0] = first[0] = S->run[0] = 0;
        for (uint32_t l = 1; l < 16; l++) {
            off[l] = (uint16_t)o;
            S->run[l] = (uint16_t)o;
            first[l] = (uint16_t)code;
            o += cnt[l];
            code = (code + cnt[l]) << 1;
        }
        for (uint32_t s = 0; s < nsym; s++) {
            const uint32_t l = lens[s] & 15u;
            if (!l) continue;
            const uint32_t r = S->run[l];
            if (r < sym_cap) sym[r] = (uint16_t)s;
            S->run[l] = (uint16_t)(r + 1u);
        }
    }
    INF_SYNC();
    int32_t left = 1;
    uint32_t max = 0, used = 0;
    for (uint32_t l = 1; l < 16; l++) {
        const uint32_t c = INF_UNI(cnt[l]);
        left = (left << 1) - (int32_t)c;
        if (left < 0) return INF_E_OVERSUB;
        if (c) max = l;
        used += c;
    }
    if (max == 0) {
        if (kind != INF_KIND_DIST) return INF_E_INCOMPLETE;  // (no distance code at all is fine until one is used)
    } else if (left > 0 && (kind == INF_KIND_CODES || max != 1u)) {
        return INF_E_INCOMPLETE;
    }
    const uint32_t size = 1u << fast_bits;
    for (uint32_t i = lane; i < size; i += nl) fast[i] = 0;
    INF_SYNC();
    if (used > sym_cap) used = sym_cap;
    for (uint32_t i = lane; i < used; i += nl) {
        const uint32_t s = sym[i];
        if (s >= nsym) continue;
        const uint32_t l = lens[s] & 15u;
        if (!l || l > fast_bits) continue;
        const uint32_t code = (uint32_t)first[l] + (i - (uint32_t)off[l]);
        const uint32_t r = inf_rev(code, l) & ((1u << l) - 1u);
        for (uint32_t j = r; j < size; j += 1u << l) fast[j] = (uint16_t)((s << 4) | l);
    }
    INF_SYNC();
    return INF_OK;
}

// the next symbol, INF_SYM_INPUT when the buffered bits end inside its code, INF_SYM_INVALID when no code matches
INF_FN uint32_t inf_decode(const uint16_t *fast, uint32_t fast_bits, const uint16_t *cnt, const uint16_t *sym, uint32_t sym_cap, InfBits &b) {
    const uint32_t e = INF_UNI(fast[(uint32_t)b.buf & ((1u << fast_bits) - 1u)]);
    if (e) {
        const uint32_t l = e & 15u;
        if (l > b.cnt) return INF_SYM_INPUT;
        inf_drop(b, l);
        return e >> 4;
    }
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t len = 1; len < 16; len++) {
        if (len > b.cnt) return INF_SYM_INPUT;
        code |= (uint32_t)(b.buf >> (len - 1u)) & 1u;
        const uint32_t c = INF_UNI(cnt[len]);
        if (code < first + c) {
            const uint32_t i = index + (code - first);
            if (i >= sym_cap) return INF_SYM_INVALID;
            const uint32_t s = INF_UNI(sym[i]);
            inf_drop(b, len);
            return s;
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return INF_SYM_INVALID;
}

// pay[0, len) -> out[0, isize); the status without the CRC
INF_FN uint32_t inf_member(InfState *S, const uint8_t *pay, uint32_t len, uint8_t *out, uint32_t isize, uint32_t lane, uint32_t nl) {
    InfBits b = {0, 0, 0, 0};
    inf_load_window(S, pay, len, b, lane, nl);
    uint32_t opos = 0, last = 0;
    do {
        inf_refill(S, pay, len, b, lane, nl);
        if (b.cnt < 3u) return INF_E_INPUT;
        last = (uint32_t)b.buf & 1u;
        const uint32_t type = ((uint32_t)b.buf >> 1) & 3u;
        inf_drop(b, 3u);
        if (type == 3u) return INF_E_BTYPE;
        if (type == 0u) {
            inf_drop(b, b.cnt & 7u);
            inf_refill(S, pay, len, b, lane, nl);
            if (b.cnt < 32u) return INF_E_INPUT;
            const uint32_t n = (uint32_t)b.buf & 0xFFFFu, nn = ((uint32_t)b.buf >> 16) & 0xFFFFu;
            inf_drop(b, 32u);
            if (n != (nn ^ 0xFFFFu)) return INF_E_STORED;
            b.pos -= b.cnt >> 3;  // (the whole bytes still buffered go back to the payload)
            b.buf = 0;
            b.cnt = 0;
            if (b.pos > len || n > len - b.pos) return INF_E_INPUT;
            if (n > isize - opos) return INF_E_OUT_OVER;
            for (uint32_t i = lane; i < n; i += nl) out[opos + i] = pay[b.pos + i];
            opos += n;
            b.pos += n;
            continue;
        }
        uint32_t nlit, ndist;
        if (type == 1u) {
            nlit = 288u;
            ndist = 32u;
            INF_SYNC();
            for (uint32_t i = lane; i < 320u; i += nl) S->lens[i] = (uint8_t)(i < 144u ? 8u : i < 256u ? 9u : i < 280u ? 7u : i < 288u ? 8u : 5u);
        } else {
            inf_refill(S, pay, len, b, lane, nl);
            if (b.cnt < 14u) return INF_E_INPUT;
            nlit = ((uint32_t)b.buf & 31u) + 257u;
            ndist = (((uint32_t)b.buf >> 5) & 31u) + 1u;
            const uint32_t ncl = (((uint32_t)b.buf >> 10) & 15u) + 4u;
            inf_drop(b, 14u);
            if (nlit > 286u || ndist > 30u) return INF_E_LENGTHS;
            INF_SYNC();
            for (uint32_t i = 0; i < 19u; i++) {
                // the order of the code-length code lengths (16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15), five bits each
                const uint32_t at = i < 12u ? (uint32_t)((0x022CAA324E804A30ull >> (5u * i)) & 31u)
                                            : (uint32_t)((0x3C2E1346Cull >> (5u * (i - 12u))) & 31u);
                uint32_t v = 0;
                if (i < ncl) {
                    if (b.cnt < 3u) inf_refill(S, pay, len, b, lane, nl);
                    if (b.cnt < 3u) return INF_E_INPUT;
                    v = (uint32_t)b.buf & 7u;
                    inf_drop(b, 3u);
                }
                if (lane == 0 && at < 19u) S->cl[at] = (uint8_t)v;
            }
            uint32_t rc = inf_build(S, S->cl, 19u, S->dist_fast, INF_CL_BITS, S->dist_sym, 32u, S->dist_cnt, S->dist_off, S->dist_first,
                                    INF_KIND_CODES, lane, nl);
            if (rc) return rc;
            const uint32_t total = nlit + ndist;  // <= 316
            uint32_t n = 0, prev = 0;
            while (n < total) {
                if (b.cnt < 22u) inf_refill(S, pay, len, b, lane, nl);
                const uint32_t s = inf_decode(S->dist_fast, INF_CL_BITS, S->dist_cnt, S->dist_sym, 32u, b);
                if (s == INF_SYM_INPUT) return INF_E_INPUT;
                if (s > 18u) return INF_E_LENGTHS;
                if (s < 16u) {
                    if (lane == 0) S->lens[n] = (uint8_t)s;
                    n++;
                    prev = s;
                    continue;
                }
                const uint32_t eb = s == 16u ? 2u : s == 17u ? 3u : 7u;
                if (b.cnt < eb) return INF_E_INPUT;
                const uint32_t rep = (s == 18u ? 11u : 3u) + ((uint32_t)b.buf & ((1u << eb) - 1u));
                inf_drop(b, eb);
                if (s == 16u && n == 0) return INF_E_LENGTHS;
                if (rep > total - n) return INF_E_LENGTHS;
                const uint32_t val = s == 16u ? prev : 0u;
                for (uint32_t i = lane; i < rep; i += nl) S->lens[n + i] = (uint8_t)val;
                n += rep;
                prev = val;
            }
            INF_SYNC();
            if (INF_UNI(S->lens[256]) == 0) return INF_E_LENGTHS;
        }
        uint32_t rc = inf_build(S, S->lens, nlit, S->lit_fast, INF_LIT_BITS, S->lit_sym, 288u, S->lit_cnt, S->lit_off, S->lit_first, INF_KIND_LIT, lane, nl);
        if (rc) return rc;
        rc = inf_build(S, S->lens + nlit, ndist, S->dist_fast, INF_DIST_BITS, S->dist_sym, 32u, S->dist_cnt, S->dist_off, S->dist_first,
                       INF_KIND_DIST, lane, nl);
        if (rc) return rc;
        for (;;) {
            if (b.cnt < 48u) inf_refill(S, pay, len, b, lane, nl);  // (a symbol takes at most 15 + 5 + 15 + 13 bits)
            uint32_t s = inf_decode(S->lit_fast, INF_LIT_BITS, S->lit_cnt, S->lit_sym, 288u, b);
            if (s == INF_SYM_INPUT) return INF_E_INPUT;
            if (s == INF_SYM_INVALID) return INF_E_LITLEN;
            if (s < 256u) {
                if (opos >= isize) return INF_E_OUT_OVER;
                if (lane == 0) out[opos] = (uint8_t)s;
                opos++;
                continue;
            }
            if (s == 256u) break;
            if (s >= 286u) return INF_E_LITLEN;
            s -= 257u;
            uint32_t eb = s < 8u || s == 28u ? 0u : (s >> 2) - 1u;
            if (b.cnt < eb) return INF_E_INPUT;
            const uint32_t length = (s == 28u ? 258u : s < 8u ? 3u + s : 3u + ((4u + (s & 3u)) << eb)) + ((uint32_t)b.buf & ((1u << eb) - 1u));
            inf_drop(b, eb);
            const uint32_t d = inf_decode(S->dist_fast, INF_DIST_BITS, S->dist_cnt, S->dist_sym, 32u, b);
            if (d == INF_SYM_INPUT) return INF_E_INPUT;
            if (d >= 30u) return INF_E_DIST;
            eb = d < 4u ? 0u : (d >> 1) - 1u;
            if (b.cnt < eb) return INF_E_INPUT;
            const uint32_t dist = (d < 4u ? 1u + d : 1u + ((2u + (d & 1u)) << eb)) + ((uint32_t)b.buf & ((1u << eb) - 1u));
            inf_drop(b, eb);
            if (dist > opos) return INF_E_FAR;
            if (length > isize - opos) return INF_E_OUT_OVER;
            // The source lies wholly before opos (a copy that overlaps itself repeats its first `dist` bytes), so no lane
            // reads what this match writes; the bytes earlier symbols stored are ordered before these loads by INF_SYNC.
            INF_SYNC();
            const uint8_t *src = out + (opos - dist);
            for (uint32_t i = lane; i < length; i += nl) out[opos + i] = src[dist >= length ? i : i % dist];
            opos += length;
        }
    } while (!last);
    inf_drop(b, b.cnt & 7u);
    if ((len - b.pos) + (b.cnt >> 3) != 0u) return INF_E_TRAILING;
    if (opos != isize) return INF_E_OUT_SHORT;
    return INF_OK;
}

// ---- CRC32 (the gzip polynomial, reflected) ----------------------------------------------------------------------------
INF_FN void inf_crc_table(InfState *S, uint32_t lane, uint32_t nl) {
    INF_SYNC();
    for (uint32_t n = lane; n < 256u; n += nl) {
        uint32_t c = n;
        for (uint32_t k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        S->crc_tab[n] = c;
    }
    INF_SYNC();
}

// a(x) * b(x) mod P (zlib's multmodp)
INF_FN uint32_t inf_multmodp(uint32_t a, uint32_t b) {
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1u)) == 0) break;
        }
        m >>= 1;
        b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}

// x^(8n) mod P by squaring
INF_FN uint32_t inf_x8n(uint32_t n) {
    uint32_t sq = 1u << 30;  // x^1
    for (uint32_t k = 0; k < 3; k++) sq = inf_multmodp(sq, sq);  // x^8
    uint32_t p = 1u << 31;  // x^0
    while (n) {
        if (n & 1u) p = inf_multmodp(sq, p);
        n >>= 1;
        if (n) sq = inf_multmodp(sq, sq);
    }
    return p;
}

// Slice `part` of out[0, isize) (INF_CRC_PARTS equal slices): its CRC32 times x^(8 * bytes behind the slice).  The XOR of
// all parts is the CRC32 of the whole (zlib's crc32_combine, applied to every slice at once).
INF_FN uint32_t inf_crc_part(const InfState *S, const uint8_t *out, uint32_t isize, uint32_t part) {
    const uint32_t slice = (isize + INF_CRC_PARTS - 1u) / INF_CRC_PARTS;
    const uint32_t lo = part * slice < isize ? part * slice : isize;
    const uint32_t hi = lo + slice < isize ? lo + slice : isize;
    if (hi == lo) return 0;
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t i = lo; i < hi; i++) c = S->crc_tab[(c ^ out[i]) & 255u] ^ (c >> 8);
    c = ~c;
    return hi < isize ? inf_multmodp(inf_x8n(isize - hi), c) : c;
}

// ---- line count beside the CRC (the member-sharded open counts lines per member and throws the text away) ---------------
enum { INF_FL_CR = 1u, INF_FL_HIGH = 2u };  // a '\r' seen, a byte >= 0x80 seen (FL_CR / FL_HIGH of the streamed ingest)

// inf_crc_part of slice `part` that also adds the slice's '\n' bytes to nl and ORs INF_FL_* into flags: the one walk over
// the output serves both.  The slice bounds are inf_crc_part's, so the loop is bounded by isize.
INF_FN uint32_t inf_crc_count_part(const InfState *S, const uint8_t *out, uint32_t isize, uint32_t part, uint32_t &nl, uint32_t &flags) {
    const uint32_t slice = (isize + INF_CRC_PARTS - 1u) / INF_CRC_PARTS;
    const uint32_t lo = part * slice < isize ? part * slice : isize;
    const uint32_t hi = lo + slice < isize ? lo + slice : isize;
    if (hi == lo) return 0;
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t i = lo; i < hi; i++) {
        const uint32_t b = out[i];
        c = S->crc_tab[(c ^ b) & 255u] ^ (c >> 8);
        nl += b == 0x0Au ? 1u : 0u;
        flags |= (b == 0x0Du ? (uint32_t)INF_FL_CR : 0u) | (b >= 0x80u ? (uint32_t)INF_FL_HIGH : 0u);
    }
    c = ~c;
    return hi < isize ? inf_multmodp(inf_x8n(isize - hi), c) : c;
}

#endif  // VS_INFLATE_CORE_H
