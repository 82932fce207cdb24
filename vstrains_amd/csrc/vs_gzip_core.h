// One plain gzip stream (RFC 1952 members of RFC 1951 deflate, as gzip, pigz and a sequencer write them) decoded in
// parallel, as ONE text for the device and the host in the manner of vs_inflate_core.h, whose bit buffer, table builder
// and symbol decoder it uses.  The method is the two-stage one of pugz and rapidgzip:
//
//   find      every bit offset is tested for the start of a non-final dynamic block: a cheap filter per lane
//             (gz_candidate_cheap: BFINAL = 0, BTYPE = 2, HLIT <= 29, HDIST <= 29, a complete code-length code), then the
//             full header by the whole wavefront (gz_candidate_full: both codes build, lens[256] != 0).  Some candidates
//             are SELECTED as run starts; the stream's known first block is one more.
//   count     gz_run<false> from every start: the run decodes blocks until an end-of-block leaves the bit position on a
//             selected start (GZ_LANDED), the input ends behind a member's trailer (GZ_END), something is wrong, or -- every
//             run but the first -- it has read its span of input (gz_span_bits, GZ_E_SPAN; counted again without the bound
//             if the chain reaches it, so a false candidate's run costs a span at most, not the payload).  It
//             writes nothing: lengths need no history.  Following "landed on" from the known start gives the chain; runs
//             off it (false candidates, which the true decoder never ends a block on) are dropped.
//   decode    gz_run<true> of every chain run into 16-bit symbols: a value below 256 is a byte, 0x8000 | j is byte j of
//             the 32 KiB in front of the run (j = 32767 is the byte just before it).  A match whose source lies inside
//             the run copies symbols, markers included.
//   windows   the 32 KiB in front of run i + 1 is the last 32 KiB of (the 32 KiB in front of run i, run i resolved).
//   resolve   gz_resolve_bytes: symbols become bytes; CRC32 per segment (a run cut at the member ends inside it), combined
//             over the chain with the x^(8n) multiply and compared with every member's trailer (gz_check_members).
//
// Bounds (the contract, not error handling):
//   payload   as in vs_inflate_core.h bytes enter the bit buffer only from [0, len); gz_peek tests every byte index;
//             every loop consumes at least one bit per turn (a symbol, a stored block, a header byte) or is counted by a
//             header field, so a run ends with the payload at the latest, and one a false candidate started one block
//             behind its span of input (gz_span_bits);
//   symbols   a literal, a match and a stored copy test opos (+ length) against cap BEFORE the first symbol is written, a
//             match source is an index in [opos - dist, opos) of the run or a marker, never an address in front of it;
//   members   a trailer is recorded only below mem_cap; a back-reference in front of the first byte of a member that
//             began inside the run is INF_E_FAR there, one that reaches in front of a member that began before the run is
//             found when the marker is resolved (hist_valid);
//   tables    as in vs_inflate_core.h.
#ifndef VS_GZIP_CORE_H
#define VS_GZIP_CORE_H
#include <vector>

#include "vs_inflate_core.h"

enum {
    GZ_E_HEADER = 15,  // what follows a member is no gzip member header (magic, CM != 8, reserved FLG bits)
    GZ_E_ISIZE = 16,   // a member's ISIZE differs from its text's length mod 2^32
    GZ_E_SPAN = 17     // a counted run read more than its span of input without landing (counted again, unbounded, if the chain reaches it)
};
// The span of input a counted run other than the first may read, in bits, for a finder span of `span` compressed bytes: 64 of
// them, 64 KiB at least.  A run a false candidate started ends at its first error or here; a true run this long (a long
// stretch without a dynamic block) is counted a second time without the bound when the chain reaches it.
INF_FN uint32_t gz_span_bits(uint32_t span) { return 8u * (span > 1024u ? 64u * (span > 0x40000u ? 0x40000u : span) : 65536u); }
enum { GZ_LANDED = 0, GZ_END = 1, GZ_FAILED = 2 };  // how a run ended

#define GZ_HIST 32768u
#define GZ_MARK 0x8000u
#define GZ_MAX_BYTES 0x10000000u  // compressed bytes of one call: bit offsets stay below 2^31
#define GZ_SPAN_BYTES 2048u       // "every candidate": compressed bytes per wavefront of the finder ...
#define GZ_SPAN_CAP 64u           // ... and the starts one span can hand on (further ones are candidates, not starts)

struct GzRun {  // what a run reports (both forms)
    uint32_t status, how;
    uint32_t end_bit;  // where it stopped reading
    uint32_t out_len;  // symbols
    uint32_t nmem;     // member trailers passed
    uint32_t tail;     // symbols since the last member began inside the run (out_len when none did)
};
struct GzMember {
    uint32_t text_end;  // run-relative: the member's text ends in front of this symbol
    uint32_t crc, isize;
};
struct GzChainRun {  // a run of the chain, as decode, windows and resolve take it
    uint32_t start_bit;
    uint32_t off, len;       // its symbols, and its text, at [off, off + len)
    uint32_t mem_off, nmem;  // its member records
    uint32_t hist_valid;     // bytes of the 32 KiB in front of it that belong to the member it starts in
};

#if defined(__HIP_DEVICE_COMPILE__)
#define GZ_BALLOT(x) ((uint64_t)__builtin_amdgcn_ballot_w64(x))
#else
#define GZ_BALLOT(x) ((uint64_t)((x) ? 1u : 0u))
#endif

// n <= 32 bits at bit offset `bit`, bytes beyond the payload read as 0 (the callers test the offset first)
INF_FN uint32_t gz_peek(const uint8_t *pay, uint32_t len, uint32_t bit, uint32_t n) {
    const uint32_t at = bit >> 3;
    uint64_t v = 0;
    for (uint32_t i = 0; i < 5u; i++)
        if (at + i < len) v |= (uint64_t)pay[at + i] << (8u * i);
    v >>= bit & 7u;
    return n >= 32u ? (uint32_t)v : (uint32_t)v & ((1u << n) - 1u);
}

// step one of the candidate test, for one lane: 13 header bits and the completeness of the code-length code
INF_FN bool gz_candidate_cheap(const uint8_t *pay, uint32_t len, uint32_t bit) {
    const uint64_t end = (uint64_t)len * 8u;
    if ((uint64_t)bit + 17u > end) return false;
    const uint32_t h = gz_peek(pay, len, bit, 17u);
    if ((h & 7u) != 4u) return false;  // BFINAL 0, BTYPE 2 (bits 1 and 2, LSB first)
    if (((h >> 3) & 31u) > 29u || ((h >> 8) & 31u) > 29u) return false;
    const uint32_t ncl = ((h >> 13) & 15u) + 4u;
    if ((uint64_t)bit + 17u + 3u * ncl > end) return false;
    uint32_t kraft = 0;
    for (uint32_t i = 0; i < ncl; i += 10u) {
        const uint32_t m = ncl - i < 10u ? ncl - i : 10u;
        uint32_t w = gz_peek(pay, len, bit + 17u + 3u * i, 3u * m);
        for (uint32_t k = 0; k < m; k++, w >>= 3)
            if (w & 7u) kraft += 128u >> (w & 7u);
    }
    return kraft == 128u;
}

// the bit buffer at bit offset `bit` of the payload; false when the payload ends before it
INF_FN bool gz_seek(InfState *S, const uint8_t *pay, uint32_t len, uint32_t bit, InfBits &b, uint32_t lane, uint32_t nl) {
    b.buf = 0;
    b.cnt = 0;
    b.pos = bit >> 3;
    b.win = 0;
    if (b.pos > len) return false;
    inf_load_window(S, pay, len, b, lane, nl);
    inf_refill(S, pay, len, b, lane, nl);
    if (b.cnt < (bit & 7u)) return false;
    inf_drop(b, bit & 7u);
    return true;
}

// The header of a dynamic block behind its three type bits: the two tables built, or the first thing wrong.  This is the
// section of inf_member, word for word, and a COPY on purpose: inf_member is left exactly as it is, because k_inflate and
// k_inflate_count are built from it and their register allocation has proved sensitive to how the decoder is cut into
// routines (vs_inflate_count.hip: a second caller in one file took k_inflate from 72 VGPRs to 248 and into scratch).
// Whether inf_member could call this routine at no cost to those kernels has not been tried; whoever changes the header
// rules changes both places, and the corpus of tests/bgzf_util.py and tests/gzip_cases.py runs through both.
INF_FN uint32_t gz_dynamic_header(InfState *S, const uint8_t *pay, uint32_t len, InfBits &b, uint32_t lane, uint32_t nl) {
    inf_refill(S, pay, len, b, lane, nl);
    if (b.cnt < 14u) return INF_E_INPUT;
    const uint32_t nlit = ((uint32_t)b.buf & 31u) + 257u;
    const uint32_t ndist = (((uint32_t)b.buf >> 5) & 31u) + 1u;
    const uint32_t ncl = (((uint32_t)b.buf >> 10) & 15u) + 4u;
    inf_drop(b, 14u);
    if (nlit > 286u || ndist > 30u) return INF_E_LENGTHS;
    INF_SYNC();
    for (uint32_t i = 0; i < 19u; i++) {
        const uint32_t at = i < 12u ? (uint32_t)((0x022CAA324E804A30ull >> (5u * i)) & 31u) : (uint32_t)((0x3C2E1346Cull >> (5u * (i - 12u))) & 31u);
        uint32_t v = 0;
        if (i < ncl) {
            if (b.cnt < 3u) inf_refill(S, pay, len, b, lane, nl);
            if (b.cnt < 3u) return INF_E_INPUT;
            v = (uint32_t)b.buf & 7u;
            inf_drop(b, 3u);
        }
        if (lane == 0 && at < 19u) S->cl[at] = (uint8_t)v;
    }
    uint32_t rc = inf_build(S, S->cl, 19u, S->dist_fast, INF_CL_BITS, S->dist_sym, 32u, S->dist_cnt, S->dist_off, S->dist_first, INF_KIND_CODES, lane, nl);
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
    rc = inf_build(S, S->lens, nlit, S->lit_fast, INF_LIT_BITS, S->lit_sym, 288u, S->lit_cnt, S->lit_off, S->lit_first, INF_KIND_LIT, lane, nl);
    if (rc) return rc;
    return inf_build(S, S->lens + nlit, ndist, S->dist_fast, INF_DIST_BITS, S->dist_sym, 32u, S->dist_cnt, S->dist_off, S->dist_first, INF_KIND_DIST, lane, nl);
}

// step two, by all lanes: the whole header at `bit` is one the decoder takes (`bit` is wave-uniform)
INF_FN bool gz_candidate_full(InfState *S, const uint8_t *pay, uint32_t len, uint32_t bit, uint32_t lane, uint32_t nl) {
    InfBits b;
    if (!gz_seek(S, pay, len, bit, b, lane, nl)) return false;
    if (b.cnt < 3u || ((uint32_t)b.buf & 7u) != 4u) return false;
    inf_drop(b, 3u);
    return gz_dynamic_header(S, pay, len, b, lane, nl) == INF_OK;
}

// The candidates among the bit offsets [lo, hi) that are >= min_bit, in ascending order: list[0 .. min(count, cap)), and
// count of all of them (first_only: the search stops at the first).  lo, hi, min_bit, cap are wave-uniform.
INF_FN uint32_t gz_find_span(InfState *S, const uint8_t *pay, uint32_t len, uint32_t lo, uint32_t hi, uint32_t min_bit, uint32_t *list,
                             uint32_t cap, bool first_only, uint32_t lane, uint32_t nl) {
    uint32_t count = 0;
    for (uint32_t base = lo; base < hi; base += nl) {
        const uint32_t p = base + lane;
        uint64_t mask = GZ_BALLOT(p < hi && p >= min_bit && gz_candidate_cheap(pay, len, p));
        while (mask) {
            const uint32_t j = (uint32_t)__builtin_ctzll(mask);
            mask &= mask - 1u;
            if (!gz_candidate_full(S, pay, len, base + j, lane, nl)) continue;
            if (count < cap && lane == 0) list[count] = base + j;
            count++;
            if (first_only) return count;
        }
    }
    return count;
}

// whether `bit` is one of the sorted starts (wave-uniform)
INF_FN bool gz_is_start(const uint32_t *starts, uint32_t n, uint32_t bit) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (INF_UNI(starts[mid]) < bit) lo = mid + 1u;
        else hi = mid;
    }
    return lo < n && INF_UNI(starts[lo]) == bit;
}

// one whole byte of a member header through the bit buffer (which is byte-aligned there); false when the payload ends
INF_FN bool gz_byte(InfState *S, const uint8_t *pay, uint32_t len, InfBits &b, uint32_t &v, uint32_t lane, uint32_t nl) {
    if (b.cnt < 8u) inf_refill(S, pay, len, b, lane, nl);
    if (b.cnt < 8u) return false;
    v = (uint32_t)b.buf & 255u;
    inf_drop(b, 8u);
    return true;
}

// CRC32 of one more byte, bit by bit (member headers only: a few bytes per member)
INF_FN uint32_t gz_crc_byte(uint32_t c, uint32_t v) {
    c ^= v;
    for (uint32_t k = 0; k < 8u; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    return c;
}

// a member header (RFC 1952: FEXTRA, FNAME, FCOMMENT of any length, FHCRC verified as zlib verifies it)
INF_FN uint32_t gz_member_header(InfState *S, const uint8_t *pay, uint32_t len, InfBits &b, uint32_t lane, uint32_t nl) {
    uint32_t h[10], v = 0, c = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < 10u; i++) {
        if (!gz_byte(S, pay, len, b, h[i], lane, nl)) return INF_E_INPUT;
        c = gz_crc_byte(c, h[i]);
    }
    if (h[0] != 0x1Fu || h[1] != 0x8Bu || h[2] != 8u || (h[3] & 0xE0u)) return GZ_E_HEADER;
    if (h[3] & 4u) {
        uint32_t lo = 0, hi = 0;
        if (!gz_byte(S, pay, len, b, lo, lane, nl) || !gz_byte(S, pay, len, b, hi, lane, nl)) return INF_E_INPUT;
        c = gz_crc_byte(gz_crc_byte(c, lo), hi);
        for (uint32_t i = 0, n = lo | (hi << 8); i < n; i++) {
            if (!gz_byte(S, pay, len, b, v, lane, nl)) return INF_E_INPUT;
            c = gz_crc_byte(c, v);
        }
    }
    for (uint32_t f = 8u; f <= 16u; f <<= 1)  // FNAME, FCOMMENT: zero-terminated
        if (h[3] & f) do {
                if (!gz_byte(S, pay, len, b, v, lane, nl)) return INF_E_INPUT;
                c = gz_crc_byte(c, v);
            } while (v);
    if (h[3] & 2u) {
        uint32_t lo = 0, hi = 0;
        if (!gz_byte(S, pay, len, b, lo, lane, nl) || !gz_byte(S, pay, len, b, hi, lane, nl)) return INF_E_INPUT;
        if ((lo | (hi << 8)) != (~c & 0xFFFFu)) return GZ_E_HEADER;
    }
    return INF_OK;
}

// A run from bit offset start_bit of pay[0, len), which lies at a block header inside a member.  WRITE: its symbols to
// sym[0, cap) and its member trailers to mem[0, mem_cap); the COUNT form (WRITE = false) touches neither.  Both forms take
// the same decisions from the same bits, so a chain run decoded with cap = the counted out_len stops where it was counted.
template <bool WRITE>
INF_FN void gz_run(InfState *S, const uint8_t *pay, uint32_t len, uint32_t start_bit, const uint32_t *starts, uint32_t nstarts, uint16_t *sym,
                   uint32_t cap, GzMember *mem, uint32_t mem_cap, GzRun &r, uint32_t lane, uint32_t nl, uint32_t span_bits = 0) {
    // span_bits (0: none; tested at block boundaries, so a run ends one block behind it at the latest): GZ_E_SPAN
    const uint32_t NONE = 0xFFFFFFFFu;
    uint32_t opos = 0, nmem = 0, mstart = NONE, st = INF_OK, how = GZ_FAILED;
    bool first = true;
    InfBits b;
    if (!gz_seek(S, pay, len, start_bit, b, lane, nl)) st = INF_E_INPUT;
    while (st == INF_OK) {
        if (!first && gz_is_start(starts, nstarts, b.pos * 8u - b.cnt)) {
            how = GZ_LANDED;
            break;
        }
        if (span_bits && b.pos * 8u - b.cnt - start_bit > span_bits) { st = GZ_E_SPAN; break; }
        first = false;
        inf_refill(S, pay, len, b, lane, nl);
        if (b.cnt < 3u) { st = INF_E_INPUT; break; }
        const uint32_t last = (uint32_t)b.buf & 1u, type = ((uint32_t)b.buf >> 1) & 3u;
        inf_drop(b, 3u);
        if (type == 3u) { st = INF_E_BTYPE; break; }
        if (type == 0u) {
            inf_drop(b, b.cnt & 7u);
            inf_refill(S, pay, len, b, lane, nl);
            if (b.cnt < 32u) { st = INF_E_INPUT; break; }
            const uint32_t n = (uint32_t)b.buf & 0xFFFFu, nn = ((uint32_t)b.buf >> 16) & 0xFFFFu;
            inf_drop(b, 32u);
            if (n != (nn ^ 0xFFFFu)) { st = INF_E_STORED; break; }
            b.pos -= b.cnt >> 3;
            b.buf = 0;
            b.cnt = 0;
            if (b.pos > len || n > len - b.pos) { st = INF_E_INPUT; break; }
            if (n > cap - opos) { st = INF_E_OUT_OVER; break; }
            if (WRITE)
                for (uint32_t i = lane; i < n; i += nl) sym[opos + i] = pay[b.pos + i];
            opos += n;
            b.pos += n;
        } else {
            if (type == 1u) {
                INF_SYNC();
                for (uint32_t i = lane; i < 320u; i += nl) S->lens[i] = (uint8_t)(i < 144u ? 8u : i < 256u ? 9u : i < 280u ? 7u : i < 288u ? 8u : 5u);
                st = inf_build(S, S->lens, 288u, S->lit_fast, INF_LIT_BITS, S->lit_sym, 288u, S->lit_cnt, S->lit_off, S->lit_first, INF_KIND_LIT, lane, nl);
                if (st == INF_OK)
                    st = inf_build(S, S->lens + 288u, 32u, S->dist_fast, INF_DIST_BITS, S->dist_sym, 32u, S->dist_cnt, S->dist_off, S->dist_first, INF_KIND_DIST, lane, nl);
            } else {
                st = gz_dynamic_header(S, pay, len, b, lane, nl);
            }
            while (st == INF_OK) {
                if (b.cnt < 48u) inf_refill(S, pay, len, b, lane, nl);
                uint32_t s = inf_decode(S->lit_fast, INF_LIT_BITS, S->lit_cnt, S->lit_sym, 288u, b);
                if (s == INF_SYM_INPUT) { st = INF_E_INPUT; break; }
                if (s == INF_SYM_INVALID) { st = INF_E_LITLEN; break; }
                if (s < 256u) {
                    if (opos >= cap) { st = INF_E_OUT_OVER; break; }
                    if (WRITE && lane == 0) sym[opos] = (uint16_t)s;
                    opos++;
                    continue;
                }
                if (s == 256u) break;
                if (s >= 286u) { st = INF_E_LITLEN; break; }
                s -= 257u;
                uint32_t eb = s < 8u || s == 28u ? 0u : (s >> 2) - 1u;
                if (b.cnt < eb) { st = INF_E_INPUT; break; }
                const uint32_t length = (s == 28u ? 258u : s < 8u ? 3u + s : 3u + ((4u + (s & 3u)) << eb)) + ((uint32_t)b.buf & ((1u << eb) - 1u));
                inf_drop(b, eb);
                const uint32_t d = inf_decode(S->dist_fast, INF_DIST_BITS, S->dist_cnt, S->dist_sym, 32u, b);
                if (d == INF_SYM_INPUT) { st = INF_E_INPUT; break; }
                if (d >= 30u) { st = INF_E_DIST; break; }
                eb = d < 4u ? 0u : (d >> 1) - 1u;
                if (b.cnt < eb) { st = INF_E_INPUT; break; }
                const uint32_t dist = (d < 4u ? 1u + d : 1u + ((2u + (d & 1u)) << eb)) + ((uint32_t)b.buf & ((1u << eb) - 1u));
                inf_drop(b, eb);
                if (mstart != NONE && dist > opos - mstart) { st = INF_E_FAR; break; }  // (mstart == NONE: dist <= 32768, a marker at worst)
                if (length > cap - opos) { st = INF_E_OUT_OVER; break; }
                if (WRITE) {
                    // as in inf_member the source lies wholly before opos; what lies before the run is named, not read
                    INF_SYNC();
                    for (uint32_t i = lane; i < length; i += nl) {
                        const int32_t k = (int32_t)opos - (int32_t)dist + (int32_t)(dist >= length ? i : i % dist);
                        sym[opos + i] = k >= 0 ? sym[k] : (uint16_t)(GZ_MARK | (uint32_t)((int32_t)GZ_HIST + k));
                    }
                }
                opos += length;
            }
            if (st != INF_OK) break;
        }
        if (!last) continue;
        // the member's trailer, and the next member's header if bytes follow
        inf_drop(b, b.cnt & 7u);
        uint32_t t[8];
        for (uint32_t i = 0; i < 8u && st == INF_OK; i++)
            if (!gz_byte(S, pay, len, b, t[i], lane, nl)) st = INF_E_INPUT;
        if (st != INF_OK) break;
        if (WRITE && nmem < mem_cap && lane == 0) {
            mem[nmem].text_end = opos;
            mem[nmem].crc = t[0] | (t[1] << 8) | (t[2] << 16) | (t[3] << 24);
            mem[nmem].isize = t[4] | (t[5] << 8) | (t[6] << 16) | (t[7] << 24);
        }
        nmem++;
        mstart = opos;
        inf_refill(S, pay, len, b, lane, nl);
        if (b.cnt == 0) {  // (refill leaves no bit only when the payload has none)
            how = GZ_END;
            break;
        }
        st = gz_member_header(S, pay, len, b, lane, nl);
    }
    r.status = st;
    r.how = st == INF_OK ? how : (uint32_t)GZ_FAILED;
    r.end_bit = b.pos * 8u - b.cnt;
    r.out_len = opos;
    r.nmem = nmem;
    r.tail = mstart == NONE ? opos : opos - mstart;
}

// The 32 KiB in front of the next run from those in front of this one (hist) and this run's symbols: byte k for
// k = first, first + step, ... into next[] (which may not alias hist).  The device keeps hist in LDS and calls
// gz_window_byte itself.
INF_FN uint8_t gz_window_byte(const uint8_t *hist, const uint16_t *sym, uint32_t len, uint32_t k) {
    if (len < GZ_HIST && k < GZ_HIST - len) return hist[k + len];
    const uint32_t s = sym[len - GZ_HIST + k];  // (len >= GZ_HIST - k here)
    return s < 256u ? (uint8_t)s : hist[s & (GZ_HIST - 1u)];
}

// Symbols of one chain run to bytes, by the lanes: out[0, len) from sym[0, len) and the 32 KiB in front (hist).  A marker
// that names a byte in front of the member the run starts in (more than hist_valid back) is written as 0 and reported:
// returns this lane's verdict, 1 for such a marker; the caller ORs the lanes' (INF_E_FAR).
INF_FN uint32_t gz_resolve_bytes(const uint16_t *sym, const uint8_t *hist, uint32_t hist_valid, uint8_t *out, uint32_t len, uint32_t lane,
                                 uint32_t nl) {
    uint32_t bad = 0;
    for (uint32_t i = lane; i < len; i += nl) {
        const uint32_t s = sym[i];
        uint8_t v = (uint8_t)s;
        if (s >= 256u) {
            const uint32_t j = s & (GZ_HIST - 1u);
            if (GZ_HIST - j > hist_valid) bad = 1u, v = 0;
            else v = hist[j];
        }
        out[i] = v;
    }
    return bad;
}

// The bounds of segment k of a run with nmem member records (clamped into [0, len], ascending): segment k is
// [mem[k - 1].text_end, mem[k].text_end), the first starts at 0, the last runs to len.  CRC32 is taken per segment.
INF_FN void gz_segment(const GzMember *mem, uint32_t nmem, uint32_t len, uint32_t k, uint32_t &lo, uint32_t &hi) {
    lo = k ? INF_UNI(mem[k - 1u].text_end) : 0u;
    hi = k < nmem ? INF_UNI(mem[k].text_end) : len;
    if (hi > len) hi = len;
    if (lo > hi) lo = hi;
}

// ---- the host's part: the first header, the chain, the trailers -----------------------------------------------------------

// the first member's header in plain bytes: the bit offset of the first block to *start, or the status
inline uint32_t gz_first_header(const uint8_t *p, uint64_t n, uint32_t *start) {
    if (n < 10u) return INF_E_INPUT;
    if (p[0] != 0x1Fu || p[1] != 0x8Bu || p[2] != 8u || (p[3] & 0xE0u)) return GZ_E_HEADER;
    uint64_t at = 10u;
    if (p[3] & 4u) {
        if (at + 2u > n) return INF_E_INPUT;
        at += 2u + ((uint64_t)p[at] | ((uint64_t)p[at + 1u] << 8));
    }
    for (uint32_t f = 8u; f <= 16u; f <<= 1)
        if (p[3] & f) {
            while (at < n && p[at]) at++;
            at++;
        }
    if (at > n) return INF_E_INPUT;
    if (p[3] & 2u) {
        if (at + 2u > n) return INF_E_INPUT;
        uint32_t c = 0xFFFFFFFFu;
        for (uint64_t i = 0; i < at; i++) c = gz_crc_byte(c, p[i]);
        if (((uint32_t)p[at] | ((uint32_t)p[at + 1u] << 8)) != (~c & 0xFFFFu)) return GZ_E_HEADER;
        at += 2u;
    }
    if (at >= GZ_MAX_BYTES) return INF_E_INPUT;
    *start = (uint32_t)at * 8u;
    return INF_OK;
}

// The run starts of a window: the known first one and, of the finder's spans (count[s] candidates, list[s * cap ..] the
// first min(count[s], cap) of them), every listed candidate behind it.  Ascending, because the spans are.
inline void gz_collect_starts(uint32_t start0, const uint32_t *count, const uint32_t *list, uint32_t spans, uint32_t cap, std::vector<uint32_t> &starts,
                              uint64_t &candidates) {
    starts.assign(1, start0);
    candidates = 0;
    for (uint32_t s = 0; s < spans; s++) {
        candidates += count[s];
        for (uint32_t i = 0; i < count[s] && i < cap; i++)
            if (list[(size_t)s * cap + i] > starts.back()) starts.push_back(list[(size_t)s * cap + i]);
    }
}

// the index of the start at `bit` (one of starts)
inline size_t gz_start_index(const std::vector<uint32_t> &starts, uint32_t bit) {
    size_t lo = 0, hi = starts.size();
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2u;
        if (starts[mid] < bit) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

struct GzPlan {
    std::vector<GzChainRun> chain;
    uint64_t text = 0, members = 0;
    uint32_t status = INF_OK;  // of the first failing chain run
    uint32_t bad_run = 0;      // its place in the chain
    uint32_t next_bit = 0;     // where the run behind the chain starts (the failing one; the payload's end when none fails)
    uint32_t valid_end = 0;    // hist_valid of that run
    bool capped = false;       // the chain stops in front of a good run whose text no longer fits text_cap (status stays 0)
};

#define GZ_TEXT_MAX 0xFFFF0000u  // symbols of one plan: offsets into the symbol buffer and the text are 32-bit

// The chain through res[0, starts.size()) from run 0.  Bounded by the run count: every run ends behind its own start.
// text_cap <= GZ_TEXT_MAX: the chain is the longest prefix whose text fits it (capped: the rest stays compressed for a
// later plan, which starts at next_bit); a FIRST run that alone does not fit is INF_E_OUT_OVER.
inline void gz_plan_chain(const std::vector<uint32_t> &starts, const GzRun *res, GzPlan &P, uint32_t valid = 0, uint32_t text_cap = GZ_TEXT_MAX) {
    P = GzPlan();
    for (size_t i = 0; i < starts.size();) {
        const GzRun &r = res[i];
        const bool over = r.status == INF_E_OUT_OVER || (r.status == INF_OK && P.text + r.out_len > text_cap);
        if (r.status != INF_OK || over) {
            if (over && !P.chain.empty()) P.capped = true;
            else P.status = over ? (uint32_t)INF_E_OUT_OVER : r.status;
            P.bad_run = (uint32_t)P.chain.size();
            P.next_bit = starts[i];
            P.valid_end = valid;
            return;
        }
        GzChainRun c = {starts[i], (uint32_t)P.text, r.out_len, (uint32_t)P.members, r.nmem, valid};
        P.chain.push_back(c);
        P.text += r.out_len;
        P.members += r.nmem;
        const uint64_t v = r.nmem ? r.tail : (uint64_t)valid + r.out_len;
        valid = v > GZ_HIST ? GZ_HIST : (uint32_t)v;
        P.next_bit = r.end_bit;
        P.valid_end = valid;
        if (r.how == GZ_END) return;
        size_t lo = i + 1u, hi = starts.size();  // the start it landed on
        while (lo < hi) {
            const size_t mid = lo + (hi - lo) / 2u;
            if (starts[mid] < r.end_bit) lo = mid + 1u;
            else hi = mid;
        }
        if (lo >= starts.size() || starts[lo] != r.end_bit) break;
        i = lo;
    }
    P.status = INF_E_INPUT;  // (a chain that does not end on GZ_END: not reached with runs of gz_run)
    P.bad_run = (uint32_t)P.chain.size();
}

// Every member's CRC32 and ISIZE against its trailer: seg_crc holds, chain run after chain run, the nmem + 1 segment CRCs
// of gz_resolve; mem the member records in chain order; crc and bytes the open member's so far (a stream in windows:
// they go from call to call, 0 at the start).  0, INF_E_CRC or GZ_E_ISIZE (zlib's order: the CRC first).
inline uint32_t gz_check_members(const GzPlan &P, const GzMember *mem, const uint32_t *seg_crc, uint32_t &crc, uint64_t &bytes) {
    for (size_t c = 0; c < P.chain.size(); c++) {
        const GzChainRun &run = P.chain[c];
        const GzMember *m = mem + run.mem_off;
        for (uint32_t k = 0; k <= run.nmem; k++) {
            uint32_t lo, hi;
            gz_segment(m, run.nmem, run.len, k, lo, hi);
            crc = inf_multmodp(inf_x8n(hi - lo), crc) ^ seg_crc[run.mem_off + c + k];
            bytes += hi - lo;
            if (k == run.nmem) break;
            if (crc != m[k].crc) return INF_E_CRC;
            if ((uint32_t)bytes != m[k].isize) return GZ_E_ISIZE;
            crc = 0;
            bytes = 0;
        }
    }
    return INF_OK;
}

struct GzInfo {
    uint64_t candidates = 0, selected = 0, chain_runs = 0, dropped = 0, members = 0, status = 0, bad_run = 0, text = 0;
    uint64_t recounted = 0;  // chain runs that hit their span of input and were counted again without it
};

// The whole path on one lane: data[0, n) -> text (empty unless the status is 0).  gran: compressed bytes per selected
// start, 0 = every candidate.  This is what the kernels of vs_gzip.hip do, step for step, with the same routines.
inline void gz_inflate_one_lane(const uint8_t *data, uint64_t n, uint32_t gran, std::vector<uint8_t> &text, GzInfo &info) {
    info = GzInfo();
    text.clear();
    uint32_t start0 = 0;
    if (n > GZ_MAX_BYTES) {
        info.status = INF_E_ARG;
        return;
    }
    if ((info.status = gz_first_header(data, n, &start0)) != INF_OK) return;
    const uint32_t len = (uint32_t)n, span = gran ? gran : GZ_SPAN_BYTES, cap = gran ? 1u : GZ_SPAN_CAP;
    const uint32_t spans = (len + span - 1u) / span;
    InfState *S = new InfState();
    std::vector<uint32_t> count(spans), list((size_t)spans * cap), starts;
    for (uint32_t s = 0; s < spans; s++) {
        const uint64_t hi = ((uint64_t)s + 1u) * span * 8u;
        count[s] = gz_find_span(S, data, len, s * span * 8u, hi < (uint64_t)len * 8u ? (uint32_t)hi : len * 8u, start0 + 1u, list.data() + (size_t)s * cap, cap,
                                gran != 0, 0, 1);
    }
    gz_collect_starts(start0, count.data(), list.data(), spans, cap, starts, info.candidates);
    info.selected = starts.size() - 1u;
    std::vector<GzRun> res(starts.size());
    for (size_t i = 0; i < starts.size(); i++)
        gz_run<false>(S, data, len, starts[i], starts.data(), (uint32_t)starts.size(), nullptr, GZ_TEXT_MAX, nullptr, 0, res[i], 0, 1,
                      i ? gz_span_bits(span) : 0u);
    GzPlan P;
    gz_plan_chain(starts, res.data(), P);
    while (P.status == GZ_E_SPAN) {  // (bounded by the run count: a run counted without the bound never reports it)
        const size_t i = gz_start_index(starts, P.next_bit);
        gz_run<false>(S, data, len, starts[i], starts.data(), (uint32_t)starts.size(), nullptr, GZ_TEXT_MAX, nullptr, 0, res[i], 0, 1);
        info.recounted++;
        gz_plan_chain(starts, res.data(), P);
    }
    if (P.capped) P.status = INF_E_OUT_OVER;  // (a whole buffer is delivered whole or not at all)
    info.chain_runs = P.chain.size();
    info.dropped = starts.size() - P.chain.size();
    info.members = P.members;
    info.status = P.status;
    info.bad_run = P.bad_run;
    if (P.status == INF_OK) {
        uint16_t *sym = new uint16_t[P.text ? P.text : 1u];  // exactly sized
        GzMember *mem = new GzMember[P.members ? P.members : 1u];
        uint8_t *out = new uint8_t[P.text ? P.text : 1u];
        std::vector<uint32_t> seg(P.members + P.chain.size());
        std::vector<uint8_t> hist(GZ_HIST, 0), next(GZ_HIST);
        inf_crc_table(S, 0, 1);
        for (size_t c = 0; c < P.chain.size() && info.status == INF_OK; c++) {
            const GzChainRun &run = P.chain[c];
            GzRun r;
            gz_run<true>(S, data, len, run.start_bit, starts.data(), (uint32_t)starts.size(), sym + run.off, run.len, mem + run.mem_off, run.nmem, r, 0, 1);
            if (r.status != INF_OK || r.out_len != run.len || r.nmem != run.nmem) {
                info.status = r.status != INF_OK ? r.status : (uint32_t)INF_E_OUT_SHORT;
                info.bad_run = c;
                break;
            }
            if (gz_resolve_bytes(sym + run.off, hist.data(), run.hist_valid, out + run.off, run.len, 0, 1)) {
                info.status = INF_E_FAR;
                info.bad_run = c;
                break;
            }
            for (uint32_t k = 0; k <= run.nmem; k++) {
                uint32_t lo, hi, crc = 0;
                gz_segment(mem + run.mem_off, run.nmem, run.len, k, lo, hi);
                for (uint32_t part = 0; part < INF_CRC_PARTS; part++) crc ^= inf_crc_part(S, out + run.off + lo, hi - lo, part);
                seg[run.mem_off + c + k] = crc;
            }
            for (uint32_t k = 0; k < GZ_HIST; k++) next[k] = gz_window_byte(hist.data(), sym + run.off, run.len, k);
            hist.swap(next);
        }
        uint32_t crc = 0;
        uint64_t bytes = 0;
        if (info.status == INF_OK) info.status = gz_check_members(P, mem, seg.data(), crc, bytes);
        if (info.status == INF_OK) {
            text.assign(out, out + P.text);
            info.text = P.text;
        }
        delete[] out;
        delete[] mem;
        delete[] sym;
    }
    delete S;
}
#endif  // VS_GZIP_CORE_H
