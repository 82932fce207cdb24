// Reading pe_info / st_info text back into cells, one source for the kernels of vs_info_read.hip and their host twin
// (vs_info_read_host): the rule of one line, the lookup of a node name, and what a window of text hands on to the next.
// Plain C++: a host compiler takes this header as it is.  It restates what vs_info_parse (vs_info.hip) does with an
// unordered_map on the host threads; that function keeps its own code.
//
// THE LINE (process_pe_info, utils/VStrains_IO.py:603-612: `line[:-1].split(":")[:3]`, int() of the third field).  The
// caller hands over the line's bytes minus its last character, [lo, hi).  The first three ':'-separated fields are taken,
// fields behind the third are ignored.  The count is an optionally signed decimal integer that fits int64
// (-9223372036854775808 is a count, 9223372036854775808 is malformed).  The count is judged BEFORE the ids are looked up:
// a line with an unknown id and a bad count is malformed, not skipped.
//
// THE NAMES.  An open-address table of 2^bits slots, at most half of them used, linear probing.  A slot holds the hash of
// the name's bytes and the node position (IR_EMPTY: free).  The hash is
//     h = 0;  for every byte b of the name:  h = h * 31 + b   (mod 2^32)
// and the first slot probed is (h * 0x9E3779B1 mod 2^32) >> (32 - bits).  A hit is confirmed byte for byte against the
// name blob, never credited on the hash alone.  A name listed twice keeps its LAST position (a dict built in order).
//
// THE WINDOW.  Text is taken in windows; a window's buffer always begins at a line start.  IrScan is what one pass over
// the buffer gives (k_info_scan, or ir_scan_host): the '\r' / >= 0x80 flags, the newlines, the first line start that holds
// a '\n' (the "first empty line" of IO.py:603, where the text ends), and the last '\n'.  ir_limit says in front of which
// position a line must START to be parsed in this window; the bytes behind the last '\n' are carried to the front of the
// next buffer.
//
// Bounds (the contract): a text byte is read only through the reader, which tests the position against the buffer; a
// table index is masked to the table; a node position and every name-blob index are tested against n and blob_bytes.
#ifndef VS_INFO_READ_CORE_H
#define VS_INFO_READ_CORE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define IR_FN __host__ __device__ inline
#else
#define IR_FN inline
#endif

enum { IR_CELL = 0, IR_SKIPPED = 1, IR_MALFORMED = 2 };  // what a line is
#define IR_EMPTY 0xFFFFFFFFu
#define IR_NONE 0xFFFFFFFFu

struct IrSlot {
    uint32_t hash, pos;
};

// Every pointer is device memory in a kernel and host memory in the twin.
struct IrNames {
    const uint8_t *blob;    // the names back to back
    const uint64_t *off;    // [n + 1] offsets into blob, off[0] = 0
    const IrSlot *table;    // [1 << bits]
    uint64_t blob_bytes;
    uint32_t n, bits;
};

IR_FN uint32_t ir_hash_step(uint32_t h, uint8_t b) { return h * 31u + (uint32_t)b; }
IR_FN uint32_t ir_first_slot(uint32_t h, uint32_t bits) { return (uint32_t)(h * 0x9E3779B1u) >> (32u - bits); }
// the smallest table for n names: at least 2 slots, at most half of them used
IR_FN uint32_t ir_table_bits(uint32_t n) {
    uint32_t bits = 1;
    while (bits < 31u && (1ull << bits) < 2ull * n) bits++;
    return bits;
}

// name i of (blob, off) into the table (host: the build).  false when the table is full or the name lies outside the blob.
inline bool ir_table_insert(IrSlot *table, uint32_t bits, const uint8_t *blob, const uint64_t *off, uint64_t blob_bytes, uint32_t i) {
    if (off[i + 1] < off[i] || off[i + 1] > blob_bytes) return false;
    const uint64_t len = off[i + 1] - off[i];
    uint32_t h = 0;
    for (uint64_t k = 0; k < len; k++) h = ir_hash_step(h, blob[off[i] + k]);
    const uint32_t mask = (1u << bits) - 1u;
    uint32_t s = ir_first_slot(h, bits);
    for (uint32_t probes = 0; probes <= mask; probes++, s = (s + 1u) & mask) {
        if (table[s].pos == IR_EMPTY) {
            table[s].hash = h, table[s].pos = i;
            return true;
        }
        if (table[s].hash != h) continue;
        const uint32_t j = table[s].pos;
        if (off[j + 1] - off[j] != len) continue;
        bool same = true;
        for (uint64_t k = 0; k < len && same; k++) same = blob[off[j] + k] == blob[off[i] + k];
        if (same) {  // listed twice: the last position stays
            table[s].pos = i;
            return true;
        }
    }
    return false;
}

// the node whose name is the text [a, b), or IR_EMPTY.  rd(x): the text byte at x.
template <class Reader>
IR_FN uint32_t ir_lookup(const IrNames &nm, const Reader &rd, uint64_t a, uint64_t b) {
    uint32_t h = 0;
    for (uint64_t x = a; x < b; x++) h = ir_hash_step(h, rd(x));
    const uint32_t mask = (1u << nm.bits) - 1u;
    uint32_t s = ir_first_slot(h, nm.bits);
    for (uint32_t probes = 0; probes <= mask; probes++, s = (s + 1u) & mask) {
        const IrSlot slot = nm.table[s];
        if (slot.pos == IR_EMPTY) return IR_EMPTY;
        if (slot.hash != h || slot.pos >= nm.n) continue;
        const uint64_t lo = nm.off[slot.pos], hi = nm.off[slot.pos + 1u];
        if (hi < lo || hi > nm.blob_bytes || hi - lo != b - a) continue;
        bool same = true;
        for (uint64_t k = 0; k < b - a && same; k++) same = nm.blob[lo + k] == rd(a + k);
        if (same) return slot.pos;
    }
    return IR_EMPTY;
}

// the line [lo, hi) (its last character already dropped): IR_CELL and (*r, *c, *val), IR_SKIPPED or IR_MALFORMED
template <class Reader>
IR_FN int ir_parse_line(const IrNames &nm, const Reader &rd, uint64_t lo, uint64_t hi, uint32_t *r, uint32_t *c, int64_t *val) {
    uint64_t c1 = lo;
    while (c1 < hi && rd(c1) != ':') c1++;
    if (c1 >= hi) return IR_MALFORMED;
    uint64_t c2 = c1 + 1u;
    while (c2 < hi && rd(c2) != ':') c2++;
    if (c2 >= hi) return IR_MALFORMED;
    uint64_t q = c2 + 1u;
    bool minus = false;
    if (q < hi) {
        const uint8_t s = rd(q);
        if (s == '+' || s == '-') minus = s == '-', q++;
    }
    if (q >= hi || rd(q) == ':') return IR_MALFORMED;  // no digit
    uint64_t mag = 0;
    for (; q < hi; q++) {
        const uint8_t ch = rd(q);
        if (ch == ':') break;  // fields behind the third are ignored
        if (ch < '0' || ch > '9') return IR_MALFORMED;
        const uint64_t d = (uint64_t)(ch - '0');
        if (mag > (0x8000000000000000ull - d) / 10u) return IR_MALFORMED;  // beyond int64
        mag = mag * 10u + d;
    }
    if (!minus && mag > 0x7FFFFFFFFFFFFFFFull) return IR_MALFORMED;
    *val = minus ? (int64_t)(0ull - mag) : (int64_t)mag;
    const uint32_t u = ir_lookup(nm, rd, lo, c1);
    if (u == IR_EMPTY) return IR_SKIPPED;
    const uint32_t v = ir_lookup(nm, rd, c1 + 1u, c2);
    if (v == IR_EMPTY) return IR_SKIPPED;
    *r = u, *c = v;
    return IR_CELL;
}

// ---- the window -----------------------------------------------------------------------------------------------------------
struct IrScan {
    uint32_t flags;     // bit 0: a '\r', bit 1: a byte >= 0x80
    uint32_t newlines;
    uint32_t empty;     // the smallest line start that holds a '\n', IR_NONE: none
    uint32_t nl_end;    // one past the largest '\n', 0: none
};

// A line of the buffer [0, size) is parsed in this window when it starts in front of the limit.  Not the last window: the
// lines that end in it, up to the empty line.  The last window: every line up to the empty line (a final line without a
// '\n' too; it loses its last character all the same).
IR_FN uint32_t ir_limit(const IrScan &s, uint32_t size, bool last) {
    const uint32_t whole = last ? size : s.nl_end;
    return s.empty < whole ? s.empty : whole;
}

// where the line that starts at p ends: *stop = one past its last kept byte, i.e. the position of the character dropped
// (its '\n', or the last byte of a buffer that ends without one)
template <class Reader>
IR_FN uint32_t ir_line_stop(const Reader &rd, uint32_t p, uint32_t size) {
    uint32_t q = p;
    while (q < size && rd(q) != '\n') q++;
    return q < size ? q : size - 1u;
}

// The walk over the windows of one text.  A buffer holds `carry` bytes of the line cut by the window before it, then new
// text, `window` bytes at the most; it always begins at a line start, `base` is the text offset of its first byte.
struct IrWalk {
    uint32_t window, carry;
    uint64_t base;
    bool parsing;  // false once the empty line or a malformed line was met: later windows are scanned, not parsed
};
IR_FN IrWalk ir_walk_begin(uint32_t window) {
    IrWalk w = {window, 0u, 0ull, true};
    return w;
}
// new bytes the next buffer has room for; 0: the line carried alone fills a window (the file is the host reader's)
IR_FN uint32_t ir_walk_room(const IrWalk &w) { return w.window - w.carry; }
// in front of which position of the buffer [0, size) a line must start to be parsed now
IR_FN uint32_t ir_walk_limit(const IrWalk &w, const IrScan &s, uint32_t size, bool last) { return w.parsing ? ir_limit(s, size, last) : 0u; }
// the window is done: what the next buffer begins with
IR_FN void ir_walk_next(IrWalk &w, const IrScan &s, uint32_t size, bool malformed) {
    if (malformed || s.empty != IR_NONE) w.parsing = false;
    const uint32_t keep = w.parsing ? size - s.nl_end : 0u;  // the bytes behind the last '\n'
    w.base += size - keep;
    w.carry = keep;
}

struct IrHostReader {
    const uint8_t *p;
    uint64_t size;
    uint8_t operator()(uint64_t x) const { return x < size ? p[x] : (uint8_t)0; }
};

inline IrScan ir_scan_host(const uint8_t *p, uint32_t size) {
    IrScan s = {0u, 0u, IR_NONE, 0u};
    for (uint32_t x = 0; x < size; x++) {
        const uint8_t b = p[x];
        if (b == '\r') s.flags |= 1u;
        if (b >= 0x80u) s.flags |= 2u;
        if (b == '\n') {
            s.newlines++;
            s.nl_end = x + 1u;
            if (s.empty == IR_NONE && (x == 0 || p[x - 1u] == '\n')) s.empty = x;
        }
    }
    return s;
}

#endif
